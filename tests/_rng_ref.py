"""A numpy restatement of the library's counter-based noise generator (include/rdm_hip.h "device noise"): Philox4x32-10 in uint64
arithmetic and Box-Muller in float64 from the same exact uniforms.  The reference of tests/test_device_noise_cpu.py and
tests/test_gpu_device_noise.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key increments
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two -> four uint32 arrays, broadcast together."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]              # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def block_words(seed, row, step, stream, block):
    """The library's layout: key = (seed lo, seed hi), counter = (block, step, row, stream) -> uint32 [..., 4]."""
    seed = int(seed) & (2 ** 64 - 1)
    return np.stack(philox4x32_10((block, step, row, stream), (seed & MASK, seed >> 32)), axis=-1)


def words(seed, row0, B, per_row, step, stream):
    """uint32 [B, per_row]: element e of row b takes word e & 3 of block e >> 2 of row row0 + b."""
    nblk = (per_row + 3) // 4
    w = block_words(seed, (row0 + np.arange(B, dtype=np.uint64))[:, None], step, stream, np.arange(nblk, dtype=np.uint64)[None, :])
    return w.reshape(B, nblk * 4)[:, :per_row]


def uniforms(w):
    """u = ((w >> 9) + 0.5) 2^-23: exact in fp32 and in fp64, strictly inside (0, 1)."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(seed, row0, B, per_row, step, stream, swap=False):
    """float64 Box-Muller of the word pairs (w0, w1), (w2, w3): element 2h = r cos(2 pi u2), 2h + 1 = r sin(2 pi u2), r = sqrt(-2 ln u1).
    -> (z [B, per_row], r [B, per_row]: each element's own radius).  swap: sin and cos exchanged (a near miss for the tests)."""
    nblk = (per_row + 3) // 4
    u = uniforms(words(seed, row0, B, nblk * 4, step, stream)).reshape(B, nblk * 2, 2)
    r = np.sqrt(-2.0 * np.log(u[..., 0]))
    a = 2.0 * np.pi * u[..., 1]
    c, s = (np.sin(a), np.cos(a)) if swap else (np.cos(a), np.sin(a))
    z = np.stack([r * c, r * s], axis=-1).reshape(B, nblk * 4)[:, :per_row]
    return z, np.repeat(r, 2, axis=-1).reshape(B, nblk * 4)[:, :per_row]
