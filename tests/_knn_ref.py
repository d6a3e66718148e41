"""References, error bounds and input builders for the stages of the retrieval search (csrc/knn.hip), all on the CPU in float64.

The search promises the oracle's answer (oracle/retrieval.py: exact products, fp64 accumulation, top-k by score descending then index
ascending) and keeps the promise with a certificate: the scan scores every row approximately, and the merge proves from those scores that
no dropped row can reach the k-th exact score -- or hands the query to an exact pass.  The proof needs |approximate - exact| <= eps.
eps_bound(path, dim) derives that bound term by term; the CPU suite holds the library's eps (rdm_knn_select) to it for every path and
dim, the GPU suite holds every candidate score the scans produce to it.

Scan paths (rdm_hip.h RDM_KNN_SCAN_*): "generic" scores sum_j (hi_j + lo_j) d_j with both fp16 words of the query, "d512" and "bulk"
score sum_j hi_j d_j.  hi = fp16(q^), lo = fp16(q^ - hi); d_j are the stored fp16 values, so every product is exact in fp32.

Terms of eps_bound (U16 = 2^-11 is fp16's unit roundoff, U32 = 2^-24 fp32's):
  hi_word       hi-word paths: |q^_j - hi_j| <= U16 |q^_j|, so the score moves by <= U16 sum |q^_j d_j| <= U16 (unit vectors).
  accumulation  fp32 accumulation of P exact products with partial sums <= 1: P * U32 when every step rounds to nearest, doubled
                because the MFMA documents neither its rounding nor its order.  P = dim (hi-word paths) or 2 dim (hi + lo).
  lo_tail       hi + lo path: where lo_j is an fp16 subnormal (|lo_j| < 2^-14, absolute spacing 2^-24) hi + lo misses q^_j by <= 2^-25;
                sum_j 2^-25 |d_j| <= sqrt(dim) 2^-25.
  lo_residual   hi + lo path: where lo_j is normal it misses by <= U16 |lo_j| <= U16^2 |q^_j|, in sum <= 2^-22.
lo_tail and lo_residual hold only if the f16 MFMA takes subnormal INPUTS at their value.  Nothing documents that for gfx950; the lo words
of the hi-word worst case below are ALL subnormal, so test_gpu_knn_stages.py observes it: a flushing MFMA would show that case's
4.7e-4 on the generic path.  MEASURED records what an MI355X showed: 4.2e-7, the subnormal lo words count.

Normalised rows: the definition is d = fp16(fp32(x / n)), n = fp32(sqrt(sum x^2)) with the sum in fp64.  The kernel adds the squares in
another order than numpy, so its n may be the neighbouring fp32 (one ulp = 2^-23 relative), and the fp32 quotient then moves by that
plus its own rounding (2^-24): within NORM_REL = 2^-22 of the float64 value x / sqrt(sum x^2).  norm_rows64 therefore gives for every
element the fp16 roundings of the float64 value scaled by (1 -+ NORM_REL): where both agree the kernel's value must be that bit pattern,
where they differ (the float64 value sits within NORM_REL of a rounding boundary) it must be one of the two neighbours.

Normalised queries: q^ = fp32(q / n), n = fp32(sqrt(sum q^2 in fp64)): two roundings of <= 2^-24 relative each, so the DEFINITION lies
within QN_REL = 2^-23 |q^| of the float64 value -- one fp32 ulp at the top of a binade, up to 1.5 spacings at its bottom (the oracle's
own normalize_queries shows 1.3 spacings on random data, test_knn_cpu.py).  The kernel is held to QN_REL against float64 and, more
sharply, to the bit pattern of the definition evaluated with the fp32 norm it shares with numpy.
"""
import math

import numpy as np

from oracle import retrieval as oret

U16 = 2.0 ** -11
U32 = 2.0 ** -24
NORM_REL = 2.0 ** -22
QN_REL = 2.0 ** -23
ROWS = 256                                    # rows per tile of every scan
PATHS = ("generic", "d512", "bulk")
HI_WORD_PATHS = ("d512", "bulk")
EMPTY = 0xffffffff

# Recorded on an MI355X by tests/test_gpu_knn_stages.py (printed there; assertions are against eps_bound, never against these).
# (path, dim) -> (worst |candidate score - exact fp64 score|, worst |candidate score - the path's own fp64 reference|, smallest certificate
# margin min(tau - theta - eps) with the library's eps), the errors over the random, ragged-tail and hi-word worst-case inputs, the margin
# over the random inputs (k = 4 and 28, 1 to 4097 rows, 1 to 512 queries).  What they show:
#   * the accumulation error is 1e-7 to 1.4e-6, two to three orders below the doubled P * 2^-24 allowance;
#   * the hi-word scans reach 4.688e-4 on the 247-hot case: inside 2^-11 + accumulation (5.49e-4), outside the 2.4e-4 + 6.1e-5 the library
#     assumed before;
#   * the hi + lo scan shows 4.2e-7 on the same case at dim 256, whose lo words are all fp16 subnormals: the f16 MFMA of gfx950 takes
#     subnormal inputs at their value (a flush would show 4.7e-4);
#   * random data certifies everywhere with margins of 4e-3 to 3e-2, i.e. 7 to 50 times the eps it runs with: the larger eps costs no
#     fallback on such data.
MEASURED = {
    ("generic", 64): (9.579e-08, 7.513e-08, 2.652e-02),
    ("generic", 256): (4.194e-07, 2.215e-07, 9.567e-03),
    ("generic", 4096): (1.190e-06, 1.424e-06, 3.673e-03),
    ("d512", 512): (4.688e-04, 2.615e-07, 1.122e-02),
    ("bulk", 512): (4.688e-04, 2.043e-07, 6.822e-03),
    ("bulk", 64): (1.329e-04, 7.500e-08, 1.599e-02),
}


def eps_terms(path, dim):
    assert path in PATHS and dim % 64 == 0
    if path in HI_WORD_PATHS:
        return {"hi_word": U16, "accumulation": 2.0 * dim * U32}
    return {"accumulation": 2.0 * (2 * dim) * U32, "lo_tail": math.sqrt(dim) * 2.0 ** -25, "lo_residual": U16 * U16}


def eps_bound(path, dim):
    """Derived bound on |approximate - exact| score of a scan path."""
    return sum(eps_terms(path, dim).values())


def accumulation_bound(path, dim):
    """Bound on |device score - the path's own exact-arithmetic score| (path_score): the fp32 accumulation alone."""
    return eps_terms(path, dim)["accumulation"]


def expected_path(n, dim, b):
    """The documented rule: bulk iff b >= 128 and at least 16 tiles; else the dim-512 scan at dim 512; else the generic one."""
    if b >= 128 and (n + ROWS - 1) // ROWS >= 16:
        return "bulk"
    return "d512" if dim == 512 else "generic"


# ---------------------------------------------------------------------------------------------------------------- references
def split_hi_lo(qn):
    """qn f32 -> (hi, lo) fp16: hi = fp16(qn), lo = fp16(qn - float(hi)) (the subtraction is exact in fp32)."""
    qn = np.asarray(qn, dtype=np.float32)
    hi = qn.astype(np.float16)
    lo = (qn - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def exact_scores(qn, dbn):
    """The oracle's score (oracle/retrieval.py): exact products, fp64 accumulation.  [B, N]."""
    return np.asarray(qn, dtype=np.float32).astype(np.float64) @ np.asarray(dbn).astype(np.float64).T


def path_scores(path, qn, dbn):
    """What a scan path computes, in exact arithmetic: sum (hi + lo) d, or sum hi d.  [B, N] float64."""
    hi, lo = split_hi_lo(qn)
    w = hi.astype(np.float64)
    if path == "generic":
        w = w + lo.astype(np.float64)
    return w @ np.asarray(dbn).astype(np.float64).T


def norm_rows64(x):
    """-> (lo, hi) uint16 bit patterns [n, dim] between which the normalised row must lie (see the module docstring); zero rows -> zeros."""
    x64 = np.asarray(x).astype(np.float32).astype(np.float64)
    n = np.sqrt((x64 ** 2).sum(axis=1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(n > 0, x64 / n, 0.0)
    a = (v * (1.0 - NORM_REL)).astype(np.float16)
    b = (v * (1.0 + NORM_REL)).astype(np.float16)
    return a.view(np.uint16), b.view(np.uint16)


def norm_queries64(q):
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    return q64 / np.sqrt((q64 ** 2).sum(axis=1, keepdims=True))


def oracle_dbn(x):
    """oracle/retrieval.py normalize_db with the zero row defined as zeros (the kernel's choice; the oracle divides 0 by 0)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = oret.normalize_db(np.asarray(x))
    d[~np.isfinite(d.astype(np.float32)).all(axis=1)] = 0
    return d


def topk(dbn, qn, k):
    return oret.exact_topk(dbn, qn, k, f64=True)


def background(rng, n, dim):
    return (rng.standard_normal((n, dim), dtype=np.float32) * 0.45).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------- input builders
def hi_word_worst_case(n, dim, seed=0, hot=247):
    """Queries whose hi word misses them by nearly half an fp16 ulp in EVERY non-zero entry, against the rows that turn that into score:
    1 / sqrt(247) = 1042.48 * 2^-14 sits 0.48 ulp from fp16, so with `hot` = 247 equal-magnitude entries and the row fp16(q^),
    exact - hi-word score = 247 * 2.99e-5 * 0.0636 = 4.69e-4 of the 4.88e-4 the hi-word term allows; the lo words (2.99e-5 < 2^-14) are
    fp16 subnormals.  Query 0: all entries +; query 1: alternating signs; rows 0..3 of the database: fp16(q^_0), fp16(q^_1), and their
    negatives (error of the other sign); random background after them.  -> (db fp16 [n, dim], q f32 [2, dim])."""
    assert dim >= hot and n >= 4
    rng = np.random.default_rng(seed)
    pos = np.arange(hot) * dim // hot
    q = np.zeros((2, dim), np.float32)
    q[0, pos] = 1.0
    q[1, pos] = np.where(np.arange(hot) % 2 == 0, 1.0, -1.0)
    qn = oret.normalize_queries(q)
    db = background(rng, n, dim)
    rows = qn.astype(np.float16)
    db[0], db[1], db[2], db[3] = rows[0], rows[1], -rows[0], -rows[1]
    # the property this builder exists for, in the fp64 reference
    dbn = oracle_dbn(db)
    assert np.array_equal(dbn[:2].view(np.uint16), rows.view(np.uint16))                  # normalising fp16(q^) gives it back
    ex, hi = exact_scores(qn, dbn[:4]), path_scores("d512", qn, dbn[:4])
    for j in range(2):
        assert ex[j, j] - hi[j, j] >= 4.6e-4 and hi[j, j + 2] - ex[j, j + 2] >= 4.6e-4, (ex - hi)
    assert np.abs(ex - hi).max() <= eps_terms("d512", dim)["hi_word"]
    lo = split_hi_lo(qn)[1].astype(np.float64)[:, pos]
    assert (np.abs(lo) < 2.0 ** -14).all() and (np.abs(lo) > 2.9e-5).all()                # subnormal, and nearly half an ulp of hi
    assert np.abs(ex - path_scores("generic", qn, dbn[:4])).max() <= eps_terms("generic", dim)["lo_tail"]
    return db, q


OVERFLOW_STRIDES = (1, 4, 8, 16, 32)
OVERFLOW_TOP = 28
OVERFLOW_GAP = 2.5e-3             # ladder step of the planted cosines; the exact scores come out >= 2e-3 apart (asserted)


def overflow_case(n, dim, tile, stride, seed=0):
    """A full 256-row tile (`tile`) of planted rows whose exact scores against the query are pairwise >= 2e-3 apart and far above the
    background; the best 28 of all planted rows sit at rows t0 + stride * j (t0 = tile * 256; beyond the tile for the wide strides).
    Row i is a_i u + sqrt(1 - a_i^2) w_i with w_i orthogonal to u, a = 0.95, 0.95 - 2.5e-3, ...; the background is random with 9/10 of its
    component along u taken out.  Eight or more of the best 28 in the rows of ONE lane fill that lane's 8-entry list with rows the
    answer needs (its tail reaches tau), whatever the lane layout is.  -> (db fp16, q f32 [1, dim], planted rows by descending score)."""
    rng = np.random.default_rng(seed)
    t0 = tile * ROWS
    top = [t0 + stride * j for j in range(OVERFLOW_TOP)]
    assert top[-1] < n and t0 + ROWS <= n
    rest = [r for r in range(t0, t0 + ROWS) if r not in set(top)]
    rng.shuffle(rest)
    planted = np.array(top + rest)
    u = rng.standard_normal(dim)
    u /= np.linalg.norm(u)
    g = rng.standard_normal((n, dim))
    g -= 0.9 * (g @ u)[:, None] * u[None]
    db = g * 0.45
    a = 0.95 - OVERFLOW_GAP * np.arange(len(planted))
    w = rng.standard_normal((len(planted), dim))
    w -= (w @ u)[:, None] * u[None]
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    db[planted] = 0.45 * (a[:, None] * u[None] + np.sqrt(1 - a[:, None] ** 2) * w)
    db = db.astype(np.float16)
    q = (3.0 * u[None]).astype(np.float32)
    s = exact_scores(oret.normalize_queries(q), oracle_dbn(db))[0]
    sp = s[planted]
    assert (sp[:-1] - sp[1:] >= 2e-3).all(), (sp[:-1] - sp[1:]).min()
    others = np.delete(s, planted)
    assert others.size == 0 or sp[-1] - others.max() >= 0.05, (sp[-1], others.max())
    return db, q, planted


def tie_flood_case(n, dim, seed=0, ties=600):
    """`ties` bit-identical rows (fewer in a small database): two tiles packed with them, the rest spread over every other tile; the query
    is that row, so all of them score highest, bit-equal, and the answer is the k lowest indices.  -> (db, q, sorted tie rows)."""
    rng = np.random.default_rng(seed)
    db = background(rng, n, dim)
    ntiles = (n + ROWS - 1) // ROWS
    packed = [t for t in (1, ntiles - 2) if 0 <= t < ntiles and (t + 1) * ROWS <= n]
    rows = set()
    for t in packed:
        rows |= set(range(t * ROWS, (t + 1) * ROWS))
    others = [t for t in range(ntiles) if t not in packed]
    want = min(ties, n // 2 + len(rows)) - len(rows)
    j = 0
    while want > 0 and others:
        t = others[j % len(others)]
        r = t * ROWS + (37 * (j // len(others)) + 5 * t) % min(ROWS, n - t * ROWS)
        if r not in rows:
            rows.add(r); want -= 1
        j += 1
        if j > 100000:
            break
    rows = np.array(sorted(rows))
    v = db[rows[0]].copy()
    db[rows] = v
    q = v.astype(np.float32)[None]
    s = exact_scores(oret.normalize_queries(q), oracle_dbn(db))[0]
    assert (s[rows] == s[rows[0]]).all() and np.delete(s, rows).max() < s[rows[0]] - 0.1
    assert len({int(r) // ROWS for r in rows}) == ntiles or n < 2 * ROWS
    return db, q, rows


def all_negative_case(n, dim, seed=0):
    """Rows c u + noise with c > 0 and the query -u: every real score is < 0, so a zero-padded row of the ragged last tile (score 0) wins
    wherever a scan scores it.  n = 1 (mod 256).  -> (db, q)."""
    assert n % ROWS == 1
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(dim)
    u /= np.linalg.norm(u)
    c = rng.uniform(0.3, 1.0, n)
    db = (0.45 * (c[:, None] * u[None] + 0.5 * rng.standard_normal((n, dim)) / math.sqrt(dim))).astype(np.float16)
    q = (-2.0 * u[None]).astype(np.float32)
    s = exact_scores(oret.normalize_queries(q), oracle_dbn(db))
    assert s.max() < -0.1
    return db, q


def normalisation_edges(n, dim, dtype, seed=0):
    """Rows for the normalisation kernel: random ones, and (where n allows) a zero row, a row of fp16 max-magnitude entries, a row of fp16
    subnormal entries, a one-hot row.  dtype np.float16 or np.float32 (the fp32 rows carry values fp16 cannot hold exactly)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, dim)) * 0.45).astype(np.float32)
    if dtype == np.float16:
        x = x.astype(np.float16).astype(np.float32)
    special = [np.zeros(dim, np.float32),
               np.where(np.arange(dim) % 3 == 0, -65504.0, 65504.0).astype(np.float32),
               (rng.integers(-1023, 1024, dim) * 2.0 ** -24).astype(np.float32),
               np.eye(1, dim, dim // 2, dtype=np.float32)[0] * -3.0]
    for j, row in enumerate(special[:max(0, n - 1)]):
        x[n - 1 - j] = row
    if n > 1:
        assert not x[n - 1].any()
    return x.astype(dtype)
