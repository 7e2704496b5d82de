"""Host model of the seeded categorical sampler (include/egopack_sample.h).

Independent of the package, like tests/philox_ref.py, which it imports: numpy only.  It predicts

  counters   sample k of (batch ordinal b, row r, head h) draws word k & 3 of counter (b << 40) | (r << 16) | (h << 8) | (k >> 2)
  key        the user's seed XOR KEY_SALT ("LTA_SAMP"): the dropout streams use the process seed itself as their key
  uniforms   float32(word >> 8) * 2^-24 -- exact in f32, so the host value IS the device value
  samples    an fp64 CDF sampler: the smallest live class c with cdf64_c > u (live: exp(x_c - max) > 0 in fp64; a row with a NaN
             or without a finite maximum gives -1)

and carries the two fixed distributions of the chi-square tests with their bounds.
"""
import numpy as np

from tests import philox_ref as PR

KEY_SALT = 0x4C54415F53414D50
B_BITS, R_BITS, H_BITS, KQ_BITS = 24, 24, 8, 8  # the fields of a counter, from the top; K <= 1024 -> k >> 2 < 2^8


def key(seed):
    return (int(seed) ^ KEY_SALT) & PR.MASK64


def counter(b, r, h, k):
    """The counter of one sample, as a Python integer (fields checked)."""
    if not (0 <= b < 1 << B_BITS and 0 <= r < 1 << R_BITS and 0 <= h < 1 << H_BITS and 0 <= k < 1024):
        raise ValueError(f"counter field out of range: b={b} r={r} h={h} k={k}")
    return (b << 40) | (r << 16) | (h << 8) | (k >> 2)


def words(seed, b, row0, rows, h, K):
    """uint32 [rows, K]: the random word of every sample of a launch over rows [row0, row0 + rows)."""
    if rows == 0 or K == 0:
        return np.zeros((rows, K), np.uint32)
    counter(b, row0, h, 0), counter(b, row0 + rows - 1, h, K - 1)  # (the range checks)
    r = (np.arange(rows, dtype=np.uint64) + np.uint64(row0)) << np.uint64(16)
    kq = np.arange(K, dtype=np.uint64) >> np.uint64(2)
    ctr = np.uint64((b << 40) | (h << 8)) | r[:, None] | kq[None, :]
    w = PR.philox_u64(ctr, key(seed))  # [rows, K, 4]
    lane = np.broadcast_to((np.arange(K) & 3)[None, :, None], (rows, K, 1))
    return np.take_along_axis(w, lane, axis=2)[..., 0]


def uniform_from_words(w):
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def uniforms(seed, b, row0, rows, h, K):
    """float32 [rows, K] in [0, 1)."""
    return uniform_from_words(words(seed, b, row0, rows, h, K))


def cdf64(logits):
    """(cdf float64 [rows, C], live bool [rows, C], valid bool [rows]) of float64 logits (-inf allowed)."""
    x = np.asarray(logits, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.max(np.where(np.isnan(x), -np.inf, x), axis=1)
        valid = np.isfinite(m) & ~np.isnan(x).any(axis=1)
        e = np.exp(x - np.where(valid, m, 0.0)[:, None])
        e = np.where(valid[:, None], e, 0.0)
        e[:, :1] = np.where(valid[:, None], e[:, :1], 1.0)  # (a placeholder distribution for invalid rows: never returned)
        cdf = np.cumsum(e, axis=1) / e.sum(axis=1, keepdims=True)
    return cdf, e > 0, valid


def sample64(logits, u):
    """int64 [rows, K]: the smallest live c with cdf64_c > u; the largest live c if there is none; -1 for an invalid row."""
    cdf, live, valid = cdf64(logits)
    u = np.asarray(u, dtype=np.float64)
    rows, K = u.shape
    ok = live[:, None, :] & (cdf[:, None, :] > u[:, :, None])  # [rows, K, C]
    first = np.argmax(ok, axis=2)
    last_live = live.shape[1] - 1 - np.argmax(live[:, ::-1], axis=1)
    out = np.where(ok.any(axis=2), first, last_live[:, None]).astype(np.int64)
    out[~valid] = -1
    return out


def on_grid(x):
    """Values rounded to the 2^-10 grid: with |x| <= 8 every difference x - max is exact in f32."""
    return np.round(np.asarray(x, dtype=np.float64) * 1024.0) / 1024.0


# ---- the chi-square cases: 4096 rows x K = 8 of ONE fixed distribution --------------------------------------------------------------
CHI_ROWS, CHI_K, CHI_SEED, CHI_ORDINAL = 4096, 8, 20240607, 3
CHI_LOGITS = {
    7: on_grid([0.0, -1.0, 1.5, -2.5, 0.75, -0.25, 2.0]),
    115: on_grid([((c * 37) % 115) / 115.0 * 3.0 - 1.5 for c in range(115)]),
}
# scipy.stats.chi2.ppf(1 - 1e-6, C - 1) for C = 7 and C = 115
CHI_BOUND = {7: 38.25833637714585, 115: 200.65036320850285}


def chi_probs(C):
    cdf, _, _ = cdf64(CHI_LOGITS[C][None, :])
    return np.diff(np.concatenate([[0.0], cdf[0]]))


def chi_square(samples, C):
    """Pearson's statistic of int samples (any shape) against chi_probs(C)."""
    n = samples.size
    counts = np.bincount(np.asarray(samples).reshape(-1), minlength=C).astype(np.float64)
    assert counts.shape[0] == C, "a sample outside [0, C)"
    expect = chi_probs(C) * n
    return float(((counts - expect) ** 2 / expect).sum())


# ---- what a launch with the optional outputs must satisfy (numpy arrays; the GPU tests and the guard-band cases share it) ------------
def tolerance(C):
    """|f32 CDF - fp64 CDF| of a C-class row: C terms of f32 accumulation in any association ((C - 1) * 2^-24 relative to the
    running sum, numerator and denominator) plus a few ulp of expf -- (C + 8) * 2^-23."""
    return (C + 8) * 2.0 ** -23


def check_launch(samples, lo, hi, total, logits, u):
    """``samples`` int64 [rows, K] with the optional outputs lo / hi / total (f32 [rows, K]) of a launch over ``logits`` (float64
    [rows, C], the values the device saw) and the host uniforms ``u`` (f32 [rows, K]).  Asserts

      exact      lo <= t < hi for EVERY sample of a valid row, t = fl32(u * total): the selection and the Philox stream bit for
                 bit, and no sample took the fallback; the sample is a live class; an invalid row is all -1
      tolerance  lo / total and hi / total within tolerance(C) of the fp64 CDF around the sample
      host       the sample IS the fp64 model's wherever u is farther than tolerance(C) from every CDF boundary; elsewhere it is
                 the model's sample or an adjacent live class

    and returns (number of samples inside the tolerance band of a boundary, number of samples of valid rows)."""
    samples, u = np.asarray(samples), np.asarray(u, dtype=np.float32)
    lo, hi, total = (np.asarray(a, dtype=np.float32) for a in (lo, hi, total))
    cdf, live, valid = cdf64(logits)
    rows, C = cdf.shape
    assert samples.shape == u.shape == lo.shape == hi.shape == total.shape and samples.shape[0] == rows
    assert (samples[~valid] == -1).all(), "an invalid row must be -1 in all K samples"
    if not valid.any():
        return 0, 0
    s, u, lo, hi, total, cdf, live = samples[valid], u[valid], lo[valid], hi[valid], total[valid], cdf[valid], live[valid]
    assert s.min() >= 0 and s.max() < C, "a sample outside [0, C)"
    r = np.arange(s.shape[0])[:, None]
    assert live[r, s].all(), "a class with e_c == 0 was returned"
    # exact
    t = u * total  # (float32 * float32: one rounded product)
    assert t.dtype == np.float32
    bad = ~((lo <= t) & (t < hi))
    assert not bad.any(), f"{int(bad.sum())} sample(s) outside lo <= t < hi (first: {np.argwhere(bad)[0].tolist()})"
    # tolerance
    tol = tolerance(C)
    cdf_hi = cdf[r, s]
    cdf_lo = np.where(s > 0, cdf[r, np.maximum(s - 1, 0)], 0.0)  # (dead classes add exactly 0 in fp64: cdf[c - 1] = cdf[previous live])
    err = max(float(np.abs(hi.astype(np.float64) / total - cdf_hi).max()), float(np.abs(lo.astype(np.float64) / total - cdf_lo).max()))
    assert err <= tol, f"f32 CDF off the fp64 CDF by {err:.3e} > (C + 8) * 2^-23 = {tol:.3e}"
    return _compare_with_model(s, u, cdf, live, tol)


def _compare_with_model(s, u, cdf, live, tol):
    rows, C = cdf.shape
    u64 = u.astype(np.float64)
    ok = live[:, None, :] & (cdf[:, None, :] > u64[:, :, None])
    last_live = C - 1 - np.argmax(live[:, ::-1], axis=1)
    host = np.where(ok.any(axis=2), np.argmax(ok, axis=2), last_live[:, None])
    dist = np.where(live[:, None, :], np.abs(cdf[:, None, :] - u64[:, :, None]), np.inf).min(axis=2)
    near = dist <= tol
    assert (s[~near] == host[~near]).all(), "a sample away from every CDF boundary differs from the fp64 model"
    rank = np.cumsum(live, axis=1) - 1  # index among the live classes
    r = np.arange(rows)[:, None]
    assert (np.abs(rank[r, s] - rank[r, host]) <= 1).all(), "a sample near a boundary is neither the model's nor an adjacent live class"
    return int(near.sum()), int(near.size)
