// Exact brute-force cosine top-k over the CLIP-embedding database held in HBM (host interface).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdm_hip.h"

struct KnnDb {
    long long n = 0; int dim = 0;
    void* dbn = nullptr;        // fp16 [n_pad, dim] normalised rows (n_pad = n rounded up to 256; tail rows zero)
    void* raw = nullptr;        // raw embeddings in the caller's dtype [n, dim]
    int raw_dtype = 0;          // 0 fp16, 1 fp32
    // search scratch
    void* scratch = nullptr; size_t scratch_bytes = 0;
    void* zero_page = nullptr;  // 256 zero bytes on the database's device (source of padding lanes)
    int last_fallbacks = 0;     // 1 if the last search needed the exact fallback pass for at least one query
};

// What knn_search does for (n, dim, b, k): scan path, list length, re-scored prefix, lists per block, queries per launch and the
// score-error bound eps the merge's certificate runs with.  The ONE statement of that choice: knn_search launches what it says
// and rdm_knn_select reports it.  Host only.  nullptr, or why the search would refuse the arguments.
const char* knn_select(long long n, int dim, int b, int k, rdm_knn_form* out);

// all return nullptr on success, or a static error string
const char* knn_load(KnnDb& db, const void* emb, long long n, int dim, int dtype, int is_device, hipStream_t st);
// Per-query row filter of one search (rdm_knn_filtered): allow [dev] [n_masks, knn_mask_words(n)], bit r % 64 of word r / 64 = row r may
// be returned; mask_of_query [host] [b] or nullptr (every query uses mask 0).  An argument of the call: nothing of it is kept.
struct KnnFilter { const uint64_t* allow; int n_masks; const int32_t* mask_of_query; };
long long knn_mask_words(long long n);      // words per mask: n rounded up to the scans' 256-row tile, / 64
// stages: nullptr (rdm_knn), or where to copy every intermediate result of ONE query group (rdm_op_knn_stages); the launches are the same.
// filt: nullptr (the unfiltered scan kernels), or the filter (their filtered instantiations; the exact fallback tests the same bits)
const char* knn_search(KnnDb& db, const float* q, int b, int k, uint32_t* idx_out, float* score_out, double* score64_out, hipStream_t st,
                       rdm_knn_stages* stages = nullptr, const KnnFilter* filt = nullptr);
// one mask from a list of row indices [dev] (duplicates allowed; invert: the complement within [0, n)); an index outside [0, n) is an error
const char* knn_row_mask(const int64_t* rows, long long n_rows, long long n, int invert, uint64_t* bits_out, hipStream_t st);
const char* knn_row_mask_count(const uint64_t* allow, int n_masks, long long n, long long* counts_out /*host*/, hipStream_t st);
const char* knn_gather(KnnDb& db, const uint32_t* idx, long long n_idx, float* out, hipStream_t st);
const char* knn_rows(KnnDb& db, long long row0, long long rows, void* out_f16, hipStream_t st);     // normalised rows [row0, row0 + rows)
void knn_free(KnnDb& db);
