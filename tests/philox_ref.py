"""Host model of the dropout keep masks: Philox4x32-10 and the counter each mask element draws from.

Independent of the package (nothing is imported from ``egopack_amd``): numpy integer arithmetic only, so every comparison with
a kernel's mask is ``torch.equal`` / ``numpy.array_equal`` -- there is no tolerance.

The contract:

  generator   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011), multipliers 0xD2511F53 /
              0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; the library's counter is (ctr & 0xffffffff, ctr >> 32, 0, 0),
              its key (seed & 0xffffffff, seed >> 32)
  keep        float32(r >> 8) * 2^-24 >= float32(p): r >> 8 < 2^24 is exact in f32 and so is the power-of-two scale
  rows        element (row, c) of a [rows, cols] LayerNorm + dropout launch: word c % 4 of counter
              offset + row * S + c // 4, S = row_stride(cols)
  flat        element i of a flat dropout launch: word i % 4 of counter offset + i // 4

``offset`` is the launch's host offset plus the device offset word, modulo 2^64 (uint64 arithmetic, as on the device).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF


# ---- scalar: plain Python integers, one counter at a time (the transcription the known answers are checked on) ------------------
def philox4x32_10_scalar(counter, key):
    """counter (c0, c1, c2, c3), key (k0, k1) -> (r0, r1, r2, r3), all 32-bit words."""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter)
    k0, k1 = (int(k) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox_u64_scalar(ctr, seed):
    """The library's wrapper: a 64-bit counter in the two low counter words, a 64-bit seed as the key."""
    ctr, seed = int(ctr) & MASK64, int(seed) & MASK64
    return philox4x32_10_scalar((ctr & MASK32, ctr >> 32, 0, 0), (seed & MASK32, seed >> 32))


# ---- vectorised: numpy uint64 lanes that hold 32-bit words (a 32 x 32 product fits) -----------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (or scalars) of 32-bit counter words, key words k0 / k1 -> uint32 array [..., 4]."""
    u = lambda v: np.asarray(v, dtype=np.uint64) & np.uint64(MASK32)
    c0, c1, c2, c3 = np.broadcast_arrays(u(c0), u(c1), u(c2), u(c3))
    k0, k1 = u(k0), u(k1)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_u64(ctr, seed):
    """uint64 counter array of any shape -> uint32 words [..., 4] (the library's wrapper, vectorised)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    seed = int(seed) & MASK64
    zero = np.zeros_like(ctr)
    return philox4x32_10(ctr & np.uint64(MASK32), ctr >> np.uint64(32), zero, zero, seed & MASK32, seed >> 32)


def keep_from_words(words, p):
    """uint32 random words -> uint8 keep flags."""
    u = (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(p)).astype(np.uint8)


# ---- which counter an element uses ------------------------------------------------------------------------------------------------
def row_stride(cols):
    """Counters between two rows of a LayerNorm + dropout launch."""
    if not 1 <= cols <= 4096:
        raise ValueError(f"row width {cols}: the row LayerNorm kernels take 1 .. 4096 columns")
    return 64 if cols <= 256 else 256 if cols <= 1024 else 1024


def _u64(v):
    return np.uint64(int(v) & MASK64)


def row_counters(offset, rows, cols):
    """uint64 [rows, ceil(cols / 4)]: the counters the launch draws (modulo 2^64)."""
    with np.errstate(over="ignore"):
        r = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(row_stride(cols))
        return _u64(offset) + r + np.arange((cols + 3) // 4, dtype=np.uint64)[None, :]


def flat_counters(offset, n):
    with np.errstate(over="ignore"):
        return _u64(offset) + np.arange((n + 3) // 4, dtype=np.uint64)


def keep_mask_rows(seed, offset, rows, cols, p):
    """uint8 [rows, cols] keep mask of ``row_layernorm(x[rows, cols], ..., p, training=True)`` at ``offset``."""
    words = philox_u64(row_counters(offset, rows, cols), seed)  # [rows, groups, 4]
    return keep_from_words(words.reshape(rows, -1)[:, :cols], p)


def keep_mask_flat(seed, offset, n, p):
    """uint8 [n] keep mask of ``dropout(x, p)`` over n elements at ``offset``."""
    return keep_from_words(philox_u64(flat_counters(offset, n), seed).reshape(-1)[:n], p)


# ---- which counters a launch consumes, as intervals (no wrap: offsets of real runs are far below 2^64) ------------------------------
def row_intervals(offset, rows, cols):
    """[(lo, hi)) per row, as Python integers."""
    s, g = row_stride(cols), (cols + 3) // 4
    return [(int(offset) + r * s, int(offset) + r * s + g) for r in range(rows)]


def flat_intervals(offset, n):
    return [(int(offset), int(offset) + (n + 3) // 4)]


def span(intervals):
    return min(a for a, _ in intervals), max(b for _, b in intervals)


def disjoint(intervals):
    """No two of the half-open intervals share a counter."""
    last = None
    for a, b in sorted(intervals):
        if last is not None and a < last:
            return False
        last = b
    return True
