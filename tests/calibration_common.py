"""The host models of the temperature calibration (include/egopack_calibrate.h), shared by tests/test_calibration_cpu.py,
tests/test_gpu_calibration.py and tests/test_gpu_bounds_calibration.py.  No GPU.

  1. ``rows_model``: F, F' and F'' row by row in float64 from the ROUNDED inputs -- bf16 logits widened, beta as the f32 word the
     launches read -- and nothing else rounded: the exact values the kernels approximate.
  2. ``rows_f32``: the same row arithmetic restated in plain f32 torch (one product, max + log-sum-exp, exp, two sums).  Its error
     against (1) over the family of test inputs is what fixes the tolerances of the GPU statistics test (``measure_f32_error``,
     asserted in tests/test_calibration_cpu.py: TOL = 4 x the measured worst, plus 2^-25 per row for the q24 rounding).
  3. ``newton_step``: the rule of egk_temp_newton in float64, statement for statement (numpy scalars: IEEE double, nothing fused).
"""
import math

import numpy as np
import torch

Q24 = float(1 << 24)
BIG = float(1 << 39)  # a row value of this magnitude (or no finite number) leaves the row out
T_RANGE = (0.05, 20.0)
BETA_MIN, BETA_MAX = float(np.float32(1.0 / T_RANGE[1])), float(np.float32(1.0 / T_RANGE[0]))  # (the f32 words the launches take)
STOP = float(np.float32(1e-6))
ITERATIONS = 16

# ---- the inputs -------------------------------------------------------------------------------------------------------------------
STATS_C = (1, 2, 115, 478, 513, 1030)   # 513: the first row that does not fit the register path
STATS_ROWS = (1, 5, 257, 8200)          # 8200 > 2048 x 4: the strided row loop
STATS_BETAS = (1.0 / 20.0, 1.0, 20.0)
FIT_C = (2, 115, 478)
FIT_BETAS = (0.25, 1.0, 3.0)
FIT_ROWS = 257


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def logits(rows, C, seed, dtype=torch.float32):
    """bf16-representable N(0, s^2) logits, s = 1 in the even rows and 4 in the odd ones, as ``dtype``."""
    g = gen(seed)
    z = torch.randn(rows, C, generator=g)
    z[1::2] *= 4.0
    return z.to(torch.bfloat16).to(dtype)


def labels_mixed(rows, C, seed):
    """Random labels with -1 and >= C entries among them (about one row in six is ignored)."""
    g = gen(seed + 1)
    y = torch.randint(0, C, (rows,), generator=g)
    u = torch.rand(rows, generator=g)
    y[u < 0.10] = -1
    y[(u >= 0.10) & (u < 0.16)] = C + 3
    return y


def labels_from(z, beta_true, seed):
    """One label per row drawn from softmax(beta_true z)."""
    p = torch.softmax(beta_true * widen(z), dim=1)
    return torch.multinomial(p, 1, generator=gen(seed + 2)).reshape(-1)


def stats_problem(C, rows, dtype=torch.float32):
    seed = 1000 * C + rows
    return logits(rows, C, seed, dtype), labels_mixed(rows, C, seed)


def fit_problem(C, beta_true, dtype=torch.float32, rows=FIT_ROWS):
    seed = 77 * C + int(100 * beta_true)
    z = logits(rows, C, seed, dtype)
    return z, labels_from(z, beta_true, seed)


def widen(z):
    return z.detach().cpu().to(torch.float64)


def beta32(beta):
    """The f32 word a launch reads, as a python float."""
    return float(np.float32(beta))


# ---- 1. the float64 model -----------------------------------------------------------------------------------------------------------
def rows_model(z, y, beta):
    """(nll, d1, d2, valid) per row in float64: ``z`` [N, C] (any float type, widened), ``y`` int64 [N], ``beta`` the f32 word.
    Ignored rows (y < 0 or y >= C) hold zeros and valid = False.  A class of probability 0 adds nothing to m and d2."""
    z, b = widen(z), beta32(beta)
    N, C = z.shape
    y = y.detach().cpu().to(torch.int64)
    valid = (y >= 0) & (y < C)
    yy = torch.where(valid, y, torch.zeros_like(y))
    x = b * z
    lse = torch.logsumexp(x, dim=1)
    p = torch.exp(x - lse[:, None])
    live = p > 0
    zf = torch.where(live, z, torch.zeros_like(z))
    m = (p * zf).sum(1)
    zy = z.gather(1, yy[:, None]).reshape(-1)
    nll = lse - b * zy
    d1 = m - zy
    d2 = (p * torch.where(live, z - m[:, None], torch.zeros_like(z)) ** 2).sum(1)
    zero = torch.zeros_like(nll)
    return torch.where(valid, nll, zero), torch.where(valid, d1, zero), torch.where(valid, d2, zero), valid


def counted(nll, d1, d2, valid):
    """The valid rows the launch does not leave out: all three values finite and below 2^39 in magnitude."""
    fits = lambda v: torch.isfinite(v) & (v.abs() < BIG)
    return valid & fits(nll) & fits(d1) & fits(d2)


def sums_model(z, y, beta):
    """dict: F, F1, F2 (float64 sums over the counted rows), A0, A1, A2 (the sums of the magnitudes), valid, ignored, left_out."""
    nll, d1, d2, valid = rows_model(z, y, beta)
    use = counted(nll, d1, d2, valid)
    s = lambda v: float(v[use].sum())
    return dict(F=s(nll), F1=s(d1), F2=s(d2), A0=s(nll.abs()), A1=s(d1.abs()), A2=s(d2.abs()), valid=int(valid.sum()),
                ignored=int((~valid).sum()), left_out=int((valid & ~use).sum()), counted=int(use.sum()))


def acc_model(z, y, beta):
    """The int64 accumulator the float64 row values would give: [llrint(v 2^24) sums, valid, ignored, left out, 0, 0]."""
    nll, d1, d2, valid = rows_model(z, y, beta)
    use = counted(nll, d1, d2, valid)
    q = lambda v: int(torch.round(v[use] * Q24).to(torch.int64).sum())
    return [q(nll), q(d1), q(d2), int(valid.sum()), int((~valid).sum()), int((valid & ~use).sum()), 0, 0]


# ---- 2. the f32 restatement and the tolerances -----------------------------------------------------------------------------------------
def rows_f32(z, y, beta):
    """The row arithmetic in plain f32 torch on the CPU (the widened logits as f32): (nll, d1, d2) as float64 copies of the f32 row
    values, zeros in ignored rows."""
    z = z.detach().cpu().to(torch.float32)
    b = torch.tensor(beta32(beta), dtype=torch.float32)
    N, C = z.shape
    y = y.detach().cpu().to(torch.int64)
    valid = (y >= 0) & (y < C)
    yy = torch.where(valid, y, torch.zeros_like(y))
    x = b * z
    mx = x.max(dim=1).values
    lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(1))
    p = torch.exp(x - lse[:, None])
    m = (p * z).sum(1)
    zy = z.gather(1, yy[:, None]).reshape(-1)
    nll = lse - b * zy
    d1 = m - zy
    d2 = (p * (z - m[:, None]) ** 2).sum(1)
    zero = torch.zeros(N, dtype=torch.float64)
    return tuple(torch.where(valid, v.double(), zero) for v in (nll, d1, d2))


def measure_f32_error(cases):
    """The worst |sum of the f32 row values - float64 sum| / sum of |float64 row value| of nll, d1 and d2 over ``cases``, an iterable of
    (z, y, beta): three floats."""
    worst = [0.0, 0.0, 0.0]
    for z, y, beta in cases:
        ref = rows_model(z, y, beta)
        got = rows_f32(z, y, beta)
        for i in range(3):
            den = float(ref[i].abs().sum())
            if den > 0:
                worst[i] = max(worst[i], abs(float(got[i].sum()) - float(ref[i].sum())) / den)
    return worst


def stats_family(rows=STATS_ROWS):
    """The statistics test's inputs: every (C, rows, beta) of its grid (f32 and bf16 logits hold the same values, and a padded
    leading dimension changes no value)."""
    for C in STATS_C:
        for r in rows:
            z, y = stats_problem(C, r)
            for beta in STATS_BETAS:
                yield z, y, beta


# Measured by tests/test_calibration_cpu.py::test_the_f32_restatement_fixes_the_tolerances over stats_family() (asserted there: the
# measurement stays at or below these figures, and above half of them).  Entry i: nll, d1, d2.  The worst d2 is a peaked one-row
# case (beta = 20), where z - m cancels; d2 only steers the Newton step.
F32_MEASURED = (1.3e-7, 3.6e-6, 1.1e-4)
TOL = tuple(4.0 * v for v in F32_MEASURED)  # the factor 4: the kernel's other summation order and its expf


def acc_bound(i, abs_sum, rows):
    """The admitted |acc[i] / 2^24 - float64 sum|: TOL_i x the sum of the rows' magnitudes, plus 2^-25 per row for the q24 rounding."""
    return TOL[i] * abs_sum + rows * 2.0 ** -25


# ---- 3. the Newton rule ----------------------------------------------------------------------------------------------------------------
def newton_init(b0=1.0, beta_min=BETA_MIN, beta_max=BETA_MAX):
    return [float(np.float32(b0)), float(beta_min), float(beta_max), 0.0, 0.0, 0.0, 0.0, 0.0]


def newton_step(acc, state, beta_min=BETA_MIN, beta_max=BETA_MAX, stop=STOP):
    """One launch of egk_temp_newton for one head: (new state -- a list of 8 python floats --, the f32 beta word as a float or None
    when the head wrote none).  ``acc``: 8 python ints."""
    f = np.float64
    st = [f(v) for v in state]
    if st[5] != 0.0:
        return [float(v) for v in st], None
    b, lo, hi, lo_seen, hi_seen = st[0], st[1], st[2], st[3], st[4]
    st[6] = st[6] + f(1.0)
    done = lambda: ([float(v) for v in st], None)
    if int(acc[3]) - int(acc[5]) <= 0:
        st[5] = f(4.0)
        return done()
    F1, F2 = f(int(acc[1])) / f(Q24), f(int(acc[2])) / f(Q24)
    if F1 > 0.0:
        hi, hi_seen = b, f(1.0)
        st[2], st[4] = hi, hi_seen
        if b <= f(beta_min):
            st[5] = f(2.0)
            return done()
    else:
        lo, lo_seen = b, f(1.0)
        st[1], st[3] = lo, lo_seen
        if b >= f(beta_max):
            st[5] = f(3.0)
            return done()
    if F2 > 0.0:
        prop = b - F1 / F2
    else:
        prop = f(-math.inf) if F1 > 0.0 else f(math.inf)
    nb = prop
    if prop >= hi:
        nb = np.sqrt(lo * hi) if hi_seen != 0.0 else hi
    elif prop <= lo:
        nb = np.sqrt(lo * hi) if lo_seen != 0.0 else lo
    nbf = np.float32(nb)
    nbd = f(nbf)
    rel = np.abs(nbd - b) / b
    st[0], st[7] = nbd, rel
    if rel <= f(stop):
        st[5] = f(1.0)
    return [float(v) for v in st], float(nbf)


def fit_model(z, y, iterations=ITERATIONS, b0=1.0, beta_min=BETA_MIN, beta_max=BETA_MAX, stop=STOP):
    """The whole fit on the host from the float64 model's integers: the final state (8 floats)."""
    st = newton_init(b0, beta_min, beta_max)
    for _ in range(iterations):
        if st[5] != 0.0:
            break
        st, _ = newton_step(acc_model(z, y, st[0]), st, beta_min, beta_max, stop)
    return st
