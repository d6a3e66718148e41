// The context of librdm_hip and what hangs off it alone: version, create / destroy, last error, scratch release, the deterministic
// and stream setters, the retrieval database entries (kernels in knn.hip), the RCCL wrappers, the per-launch profiler's entries and
// the box calibration probe.
#include <dlfcn.h>

#include "host.h"

const char* rdm_version(void) { return "rdm_hip 0.1 (gfx950)"; }

int rdm_ctx_create(int device_id, rdm_ctx** out) {
    if (!out) return -1;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -4;      // no HIP device: fail loudly, there is no CPU path
    if (device_id < 0 || device_id >= n) return -1;
    DevGuard guard(device_id);
    rdm_ctx* c = new rdm_ctx();
    c->device = device_id;
    {   // zero page + identity matrix (the residual-as-K-columns operand of the linear GEMMs, igemm.hip)
        const size_t bytes = RDM_EYE_OFFSET + (size_t)RDM_EYE_N * RDM_EYE_N * 2;
        std::vector<uint16_t> host(bytes / 2, 0);
        for (int i = 0; i < RDM_EYE_N; i++) host[RDM_EYE_OFFSET / 2 + (size_t)i * RDM_EYE_N + i] = 0x3F80;   // bf16 1.0
        if (hipMalloc(&c->zero_page, bytes) != hipSuccess || hipMemcpy(c->zero_page, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { delete c; return -2; }
    }
    *out = c;
    return 0;
}

void rdm_ctx_destroy(rdm_ctx* c) {
    if (!c) return;
    if (c->comm) rdm_comm_destroy(c);
    DevGuard guard(c->device);
    hipDeviceSynchronize();
    c->unet.release(); c->vq.release(); c->vqenc.release(); c->clip.release(); c->rarm.release();
    void* ptrs[] = {c->zero_page, c->eye3, c->gn_partial, c->samp, c->splitk_ws, c->wfrag_tmp, c->bwd_tmp, c->nn_bias};      // the context's own buffers
    for (void* p : ptrs) if (p) hipFree(p);
    c->drop_frags();
    knn_free(c->db);
    delete c;
}

const char* rdm_last_error(rdm_ctx* c) { return c ? c->err : "null context"; }

// The grow-only work buffers (backward scratch: K-major operand copies + up to 256 MB of fp32 weight-gradient planes per conv -- over
// 1 GB for the 576 -> 192 block at 64 x 64 and batch 64 --, split-K planes, per-call weight re-packs, sampler scratch) are kept between
// calls so that steady-state steps allocate nothing; a caller switching from training back to sampling hands them back here.  They
// are re-created on demand.
int rdm_release_scratch(rdm_ctx* c) {
    RDM_ENTER(c);
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    char** bufs[] = {&c->bwd_tmp, &c->wfrag_tmp, &c->splitk_ws, &c->samp};
    size_t* sizes[] = {&c->bwd_tmp_bytes, &c->wfrag_tmp_bytes, &c->splitk_ws_bytes, &c->samp_bytes};
    for (int i = 0; i < 4; i++) { if (*bufs[i]) { (void)hipFree(*bufs[i]); *bufs[i] = nullptr; } *sizes[i] = 0; }
    return 0;
}
int rdm_set_deterministic(rdm_ctx* c, int on) { if (!c) return -1; c->deterministic = on != 0; return 0; }
int rdm_get_deterministic(rdm_ctx* c) { return c ? (c->deterministic ? 1 : 0) : -1; }
// The neighbour bias (rdm_hip.h): validated on the host, kept as [rows | rows zero rows][k] on the device (host.h: nn_bias).  A refused
// bias changes nothing.
int rdm_set_neighbour_bias(rdm_ctx* c, const float* bias, int rows, int k) {
    RDM_ENTER(c);
    if (!bias) { c->nn_bias_rows = c->nn_bias_k = 0; return 0; }       // (the buffer stays for the next bias)
    if (rows < 1 || k < 1 || k > 256 || (long long)rows * k > (1ll << 24)) return c->fail(-1, "rdm_set_neighbour_bias: bad shape rows=%d k=%d (rows >= 1, 1 <= k <= 256)", rows, k);
    for (int b = 0; b < rows; b++) {
        bool any = false;
        for (int j = 0; j < k; j++) {
            const float v = bias[(size_t)b * k + j];
            if (v != v) return c->fail(-1, "rdm_set_neighbour_bias: bias[%d][%d] is NaN", b, j);
            if (v == INFINITY) return c->fail(-1, "rdm_set_neighbour_bias: bias[%d][%d] is +inf (finite values and -inf only)", b, j);
            any = any || v != -INFINITY;
        }
        if (!any) return c->fail(-1, "rdm_set_neighbour_bias: row %d has no finite entry (a sample must keep at least one neighbour)", b);
    }
    const size_t n = (size_t)rows * k;
    std::vector<float> host(2 * n, 0.f);
    std::copy(bias, bias + n, host.begin());
    // a forward already queued on the stream may still read the previous copy
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    c->nn_bias_rows = c->nn_bias_k = 0;              // (nothing is in force if the copy below fails half-way)
    RDM_TRY(ensure_bytes(c, (char**)&c->nn_bias, &c->nn_bias_bytes, 2 * n * sizeof(float)));
    hipError_t e = hipMemcpyAsync(c->nn_bias, host.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);       // host goes out of scope
    RDM_CHECK_HIP(c, e);
    c->nn_bias_rows = rows; c->nn_bias_k = k;
    return 0;
}
int rdm_get_neighbour_bias(rdm_ctx* c, int* rows, int* k) {
    if (!c) return -1;
    if (rows) *rows = c->nn_bias_rows;
    if (k) *k = c->nn_bias_k;
    return c->nn_bias_rows ? 1 : 0;
}
int rdm_set_stream(rdm_ctx* c, void* s) {
    RDM_ENTER(c);
    if ((hipStream_t)s != c->stream) {      // work queued (and derived weight copies packed) on the old stream completes before the new one is used
        RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
        c->stream = (hipStream_t)s;
    }
    return 0;
}

// ---- retrieval (kernels in knn.hip)
int rdm_db_load(rdm_ctx* c, const void* emb, long long n, int dim, int dtype, int is_device) {
    RDM_ENTER(c);
    if (!c || !emb) return -1;
    const char* msg = knn_load(c->db, emb, n, dim, dtype, is_device, c->stream);
    return msg ? c->fail(-5, "rdm_db_load: %s", msg) : 0;
}
long long rdm_db_size(rdm_ctx* c) { return c ? c->db.n : -1; }
static int knn_entry(rdm_ctx* c, const float* q, int b, int k, uint32_t* idx_out, float* score_out, double* score64_out, rdm_knn_stages* stages = nullptr,
                     const KnnFilter* filt = nullptr) {
    RDM_ENTER(c);
    if (!c || !q || !idx_out) return c ? c->fail(-1, "null argument") : -1;
    const bool prof = (c->prof >> RDM_PROF_KNN) & 1u;
    if (prof) {     // whole search (query prep + database scan + candidate merge); work = bytes of the database passes
        rdm_ctx::ProfRec r; r.a = c->prof_event(); r.b = c->prof_event(); r.kind = RDM_PROF_KNN;
        r.flops = (double)((b + 63) / 64) * (double)c->db.n * c->db.dim * 2.0;
        r.tag = "knn"; r.d0 = b; r.d1 = k; r.d2 = c->db.dim;
        hipEventRecord(r.a, c->stream); c->prof_recs.push_back(r);
    }
    const char* msg = knn_search(c->db, q, b, k, idx_out, score_out, score64_out, c->stream, stages, filt);
    if (prof) hipEventRecord(c->prof_recs.back().b, c->stream);
    return msg ? c->fail(-5, filt ? "rdm_knn_filtered: %s" : "rdm_knn: %s", msg) : 0;
}
int rdm_knn(rdm_ctx* c, const float* q, int b, int k, uint32_t* idx_out, float* score_out) { return knn_entry(c, q, b, k, idx_out, score_out, nullptr); }
int rdm_knn_f64(rdm_ctx* c, const float* q, int b, int k, uint32_t* idx_out, double* score_out) { return knn_entry(c, q, b, k, idx_out, nullptr, score_out); }
int rdm_knn_last_fallback(rdm_ctx* c) { return c ? c->db.last_fallbacks : -1; }
int rdm_knn_select(long long n, int dim, int b, int k, rdm_knn_form* out) {
    if (!out) return -1;
    *out = rdm_knn_form{};
    return knn_select(n, dim, b, k, out) ? -1 : 0;
}
int rdm_op_knn_stages(rdm_ctx* c, const float* q, int b, int k, uint32_t* idx_out, float* score_out, rdm_knn_stages* stages) {
    if (c && !stages) return c->fail(-1, "rdm_op_knn_stages: null argument");
    return knn_entry(c, q, b, k, idx_out, score_out, nullptr, stages);
}
// ---- filtered retrieval: the filter is an argument of the call, nothing of it stays on the context
int rdm_knn_mask_words(long long n) { return (int)knn_mask_words(n); }
int rdm_knn_filtered(rdm_ctx* c, const float* q, int b, int k, const uint64_t* allow, int n_masks, const int32_t* mask_of_query, uint32_t* idx_out,
                     float* score_out) {
    const KnnFilter f{allow, n_masks, mask_of_query};
    return knn_entry(c, q, b, k, idx_out, score_out, nullptr, nullptr, &f);
}
int rdm_knn_filtered_f64(rdm_ctx* c, const float* q, int b, int k, const uint64_t* allow, int n_masks, const int32_t* mask_of_query, uint32_t* idx_out,
                         double* score_out) {
    const KnnFilter f{allow, n_masks, mask_of_query};
    return knn_entry(c, q, b, k, idx_out, nullptr, score_out, nullptr, &f);
}
int rdm_op_knn_stages_filtered(rdm_ctx* c, const float* q, int b, int k, const uint64_t* allow, int n_masks, const int32_t* mask_of_query,
                               uint32_t* idx_out, float* score_out, rdm_knn_stages* stages) {
    if (c && !stages) return c->fail(-1, "rdm_op_knn_stages_filtered: null argument");
    const KnnFilter f{allow, n_masks, mask_of_query};
    return knn_entry(c, q, b, k, idx_out, score_out, nullptr, stages, &f);
}
int rdm_op_row_mask(rdm_ctx* c, const int64_t* rows, long long n_rows, long long n, int invert, uint64_t* bits_out) {
    RDM_ENTER(c);
    if (!bits_out || (!rows && n_rows > 0)) return c->fail(-1, "rdm_op_row_mask: null argument");
    const char* msg = knn_row_mask(rows, n_rows, n, invert, bits_out, c->stream);
    return msg ? c->fail(-5, "rdm_op_row_mask: %s", msg) : 0;
}
int rdm_op_row_mask_count(rdm_ctx* c, const uint64_t* allow, int n_masks, long long n, long long* counts_out) {
    RDM_ENTER(c);
    if (!allow || !counts_out) return c->fail(-1, "rdm_op_row_mask_count: null argument");
    const char* msg = knn_row_mask_count(allow, n_masks, n, counts_out, c->stream);
    return msg ? c->fail(-5, "rdm_op_row_mask_count: %s", msg) : 0;
}
int rdm_db_rows(rdm_ctx* c, long long row0, long long rows, void* out_f16) {
    RDM_ENTER(c);
    if (!out_f16) return c->fail(-1, "rdm_db_rows: null argument");
    const char* msg = knn_rows(c->db, row0, rows, out_f16, c->stream);
    return msg ? c->fail(-5, "rdm_db_rows: %s", msg) : 0;
}
int rdm_db_gather(rdm_ctx* c, const uint32_t* idx, long long n_idx, float* out) {
    RDM_ENTER(c);
    if (!c || !idx || !out) return -1;
    const char* msg = knn_gather(c->db, idx, n_idx, out, c->stream);
    return msg ? c->fail(-5, "rdm_db_gather: %s", msg) : 0;
}

// ------------------------------------------------------------------------------------ RCCL wrappers (include/rdm_hip.h, multi-GPU)
// RCCL is resolved at run time: the ABI types are spelled out here (ncclUniqueId = 128 bytes, ncclComm_t = pointer, ncclInt8 = 0)
namespace {
struct RcclId { char b[128]; };
typedef int (*fn_get_id)(RcclId*);
typedef int (*fn_init_rank)(void**, int, RcclId, int);
typedef int (*fn_all_gather)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*fn_all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_destroy)(void*);
typedef const char* (*fn_errstr)(int);
struct RcclFns { fn_get_id get_id; fn_init_rank init_rank; fn_all_gather all_gather; fn_all_reduce all_reduce; fn_destroy destroy; fn_errstr errstr; };
int rccl_load(rdm_ctx* c, RcclFns& f) {
    if (!c->rccl_lib) {
        c->rccl_lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!c->rccl_lib) c->rccl_lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!c->rccl_lib) return c->fail(-5, "rdm_comm: cannot load librccl.so (%s)", dlerror());
    }
    f.get_id = (fn_get_id)dlsym(c->rccl_lib, "ncclGetUniqueId"); f.init_rank = (fn_init_rank)dlsym(c->rccl_lib, "ncclCommInitRank");
    f.all_gather = (fn_all_gather)dlsym(c->rccl_lib, "ncclAllGather"); f.destroy = (fn_destroy)dlsym(c->rccl_lib, "ncclCommDestroy");
    f.all_reduce = (fn_all_reduce)dlsym(c->rccl_lib, "ncclAllReduce");
    f.errstr = (fn_errstr)dlsym(c->rccl_lib, "ncclGetErrorString");
    if (!f.get_id || !f.init_rank || !f.all_gather || !f.destroy) return c->fail(-5, "rdm_comm: librccl.so lacks the expected entry points");
    return 0;
}
}  // namespace
int rdm_comm_unique_id(rdm_ctx* c, void* id128) {
    RDM_ENTER(c);
    if (!id128) return c->fail(-1, "rdm_comm_unique_id: null id buffer");
    RcclFns f{}; RDM_TRY(rccl_load(c, f));
    RcclId id; const int r = f.get_id(&id);
    if (r != 0) return c->fail(-5, "ncclGetUniqueId failed: %s", f.errstr ? f.errstr(r) : "?");
    memcpy(id128, id.b, 128);
    return 0;
}
int rdm_comm_init(rdm_ctx* c, const void* id128, int rank, int world) {
    RDM_ENTER(c);
    if (!id128 || world < 1 || rank < 0 || rank >= world) return c->fail(-1, "rdm_comm_init: bad arguments (rank %d of %d)", rank, world);
    if (c->comm) return c->fail(-1, "rdm_comm_init: communicator already initialised (rdm_comm_destroy first)");
    RcclFns f{}; RDM_TRY(rccl_load(c, f));
    RcclId id; memcpy(id.b, id128, 128);
    void* comm = nullptr; const int r = f.init_rank(&comm, world, id, rank);
    if (r != 0) return c->fail(-5, "ncclCommInitRank failed: %s", f.errstr ? f.errstr(r) : "?");
    c->comm = comm; c->comm_world = world;
    return 0;
}
int rdm_comm_all_gather(rdm_ctx* c, const void* send, void* recv, size_t nbytes) {
    RDM_ENTER(c);
    if (!c->comm) return c->fail(-1, "rdm_comm_all_gather: no communicator (rdm_comm_init)");
    if (!send || !recv) return c->fail(-1, "rdm_comm_all_gather: null buffer");
    RcclFns f{}; RDM_TRY(rccl_load(c, f));
    const int r = f.all_gather(send, recv, nbytes, /*ncclInt8*/ 0, c->comm, c->stream);
    if (r != 0) return c->fail(-5, "ncclAllGather failed: %s", f.errstr ? f.errstr(r) : "?");
    return 0;
}
int rdm_comm_all_reduce_f32(rdm_ctx* c, float* buf, size_t count, int average) {
    RDM_ENTER(c);
    if (!c->comm) return c->fail(-1, "rdm_comm_all_reduce_f32: no communicator (rdm_comm_init)");
    if (!buf) return c->fail(-1, "rdm_comm_all_reduce_f32: null buffer");
    RcclFns f{}; RDM_TRY(rccl_load(c, f));
    if (!f.all_reduce) return c->fail(-5, "rdm_comm: librccl.so lacks ncclAllReduce");
    const int r = f.all_reduce(buf, buf, count, /*ncclFloat32*/ 7, /*ncclSum*/ 0, c->comm, c->stream);
    if (r != 0) return c->fail(-5, "ncclAllReduce failed: %s", f.errstr ? f.errstr(r) : "?");
    if (average && c->comm_world > 1) RDM_CHECK_HIP(c, launch_scale_f32(buf, (long long)count, 1.0f / (float)c->comm_world, c->stream));
    return 0;
}
int rdm_comm_destroy(rdm_ctx* c) {
    RDM_ENTER(c);
    if (!c->comm) return 0;
    RcclFns f{}; RDM_TRY(rccl_load(c, f));
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    f.destroy(c->comm); c->comm = nullptr; c->comm_world = 0;
    return 0;
}

// ---- profiler
int rdm_prof_enable(rdm_ctx* c, int kind_mask) {
    if (!c) return -1;
    c->prof = (unsigned)kind_mask;
    return 0;
}
int rdm_prof_collect(rdm_ctx* c, int kind, long long* launches, double* ms, double* flops) {
    RDM_ENTER(c);
    if (!c) return -1;
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    long long n = 0; double t = 0, f = 0;
    for (auto& r : c->prof_recs) {
        if (r.kind != kind) continue;
        float e = 0; hipEventElapsedTime(&e, r.a, r.b);
        n++; t += e; f += r.flops;
    }
    if (launches) *launches = n; if (ms) *ms = t; if (flops) *flops = f;
    return 0;
}
int rdm_prof_dump(rdm_ctx* c, const char* path) {
    RDM_ENTER(c);
    if (!c || !path) return -1;
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    FILE* f = fopen(path, "w");
    if (!f) return c->fail(-1, "rdm_prof_dump: cannot open %s", path);
    fprintf(f, "kind,tag,d0,d1,d2,ms,work\n");
    for (auto& r : c->prof_recs) {
        float e = 0; hipEventElapsedTime(&e, r.a, r.b);
        fprintf(f, "%d,%s,%d,%d,%d,%.6f,%.6e\n", r.kind, r.tag ? r.tag : "", r.d0, r.d1, r.d2, e, r.flops);
    }
    fclose(f);
    return 0;
}
int rdm_prof_reset(rdm_ctx* c) {
    RDM_ENTER(c);
    if (!c) return -1;
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    for (auto& r : c->prof_recs) { c->prof_pool.push_back(r.a); c->prof_pool.push_back(r.b); }
    c->prof_recs.clear();
    return 0;
}

// Box calibration (calib.hip): fixed probes, independent of every product kernel.  buf: caller's device scratch.
int rdm_calib_probe(rdm_ctx* c, void* buf, size_t buf_bytes, double mfma_ms, size_t stream_bytes, int stream_reps, double* mfma_tflops, double* stream_gbps) {
    RDM_ENTER(c);
    if (!buf || buf_bytes < (1u << 20) || buf_bytes < 2 * stream_bytes || stream_bytes % 16 || stream_reps < 1 || !(mfma_ms > 0))
        return c->fail(-2, "rdm_calib_probe: buf must hold max(1 MiB, 2 * stream_bytes), stream_bytes a multiple of 16, stream_reps >= 1, mfma_ms > 0");
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    RDM_CHECK_HIP(c, run_calib_probes(buf, mfma_ms, stream_bytes, stream_reps, mfma_tflops, stream_gbps, c->stream));
    return 0;
}
