"""Host model of include/egopack_topk.h in numpy, written from the definitions (not from the kernel), and the input builders the
GPU tests of the launch share.

The order of a row is the one of tests/class_report_common.py (``order``: imported, not copied): entry j is its j-th class, -1
beyond the row's C classes.  The probabilities are the float64 softmax, prob64 = exp(x - logsumexp64(x)), gathered at the entries
(0 beyond C).  A row with a NaN (or without a finite maximum) has NaN in every probability."""
import numpy as np
import torch

from tests.class_report_common import order

CS = (1, 2, 7, 63, 64, 65, 115, 478, 513, 1025)  # 63 / 64 / 65: the lane edge; 513 and 1025: beyond the register-resident rows
KS = (1, 2, 5, 16, 64)
ROWS = (0, 1, 4, 5, 9, 77)                       # 4 / 5: the four-waves-per-workgroup edge
PROB_TOL = dict(rtol=1e-5, atol=1e-6)            # tests/test_gpu_kernels.py: the f32 cross entropy's


def widen(x: torch.Tensor) -> np.ndarray:
    """The f32 values the launch orders: the tensor itself, or a bf16 tensor widened."""
    return x.detach().float().cpu().numpy()


def topk_order(x: np.ndarray, k: int) -> np.ndarray:
    """int64 [N, k]: the first k classes of every row, -1 beyond C."""
    x = np.asarray(x, dtype=np.float32)
    N, C = x.shape
    out = np.full((N, k), -1, dtype=np.int64)
    if N:
        out[:, :min(k, C)] = order(x)[:, :k]
    return out


def logsumexp64(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=1, keepdims=True) if x.shape[0] else np.zeros((0, 1))
        return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def prob64(x: np.ndarray) -> np.ndarray:
    """float64 [N, C] softmax."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(x - logsumexp64(x)[:, None])


def model(x: np.ndarray, k: int):
    """(idx int64 [N, k], prob float64 [N, k], lse float64 [N])."""
    idx = topk_order(x, k)
    p = prob64(x)
    N = idx.shape[0]
    got = np.zeros((N, k), dtype=np.float64)
    if N:
        rows = np.arange(N)[:, None]
        got = np.where(idx >= 0, p[rows, np.maximum(idx, 0)], 0.0)
    return idx, got, logsumexp64(x)


def special_rows(C: int, g) -> torch.Tensor:
    """f32 [9, C]: a NaN planted in a grid row; -inf entries in a grid row; a row of all equal values; a row of -0 and +0; a row
    of NaN only; a tie row with two NaNs; -inf and NaN mixed; a plain grid row; a tie row with -inf entries.  (Column 0 of the
    rows with -inf stays finite, so that the row has a distribution.)"""
    from tests.class_report_common import logits
    nan, inf = float("nan"), float("inf")
    x = logits(9, C, g)
    x[5] = logits(1, C, g, ties=True)[0]
    x[8] = logits(1, C, g, ties=True)[0]
    pick = lambda: int(torch.randint(0, C, (1,), generator=g))
    x[0, pick()] = nan
    x[2] = 0.5
    x[3] = 0.0
    x[3, 0::2] = -0.0
    x[4] = nan
    x[5, pick()] = nan
    x[5, pick()] = nan
    for r in (1, 6, 8):
        dead = torch.rand(C, generator=g) < 0.34
        dead[0] = False
        if C > 1:
            dead[C - 1] = True
        x[r, dead] = -inf
    x[6, pick()] = nan
    return x
