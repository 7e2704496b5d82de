"""Host model of include/egopack_retrieval.h in numpy, written from the definitions (not from the kernel), and the input builders
the GPU tests of the launch share.

``wins``: the sources of a row are its k listed bank rows in list order, then the node's own activation row; per channel the winner
starts as source 0 with best = -inf and source j takes over only with v > best (a NaN never does).  ``dist``: the reference's
formulas (models/graphONE/graphONE.py, __compute_edges) in float64 from the f32 values.

The bound of ``dist`` against that float64 value (``dist_bound``): each of the launch's sums is H / 64 sequential f32 additions per
lane (of four-term groups) and six reduction levels; Cauchy-Schwarz bounds the error of the dot product relative to |f| |p|, the two
norms carry the same relative error, and the square roots, the product, the quotient and the subtraction add a handful of roundings:
(H / 64 + 16) * 2^-24, absolute for the cosine distance (a value in [0, 2]), relative for l2."""
import numpy as np
import torch

ROWS = (1, 5, 67)            # not a multiple of the four waves of a workgroup
HS = (8, 64, 200, 1024)      # 8: fewer lanes than a wave; 200: a lane tail inside a 256-column step; 1024: four steps
KS = (1, 4, 32)
U = 2.0 ** -24


def dist_bound(H: int) -> float:
    return (H / 64 + 16) * U


def widen(x: torch.Tensor) -> np.ndarray:
    """The f32 values the launch reads: the tensor itself, or a bf16 tensor widened."""
    return x.detach().float().cpu().numpy()


def wins_model(f_act: np.ndarray, bank: np.ndarray, nn: np.ndarray) -> np.ndarray:
    """int32 [N, k + 1]."""
    f_act, bank = np.asarray(f_act, dtype=np.float32), np.asarray(bank, dtype=np.float32)
    N, H = f_act.shape
    k = nn.shape[1]
    best = np.full((N, H), -np.inf, dtype=np.float32)
    arg = np.zeros((N, H), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(k + 1):
            v = bank[nn[:, j]] if j < k else f_act
            win = v > best
            best, arg = np.where(win, v, best), np.where(win, j, arg)
    return np.stack([(arg == j).sum(axis=1) for j in range(k + 1)], axis=1).astype(np.int32)


def dist_model(f: np.ndarray, bank: np.ndarray, nn: np.ndarray, distance: str) -> np.ndarray:
    """float64 [N, k]."""
    f, p = np.asarray(f, dtype=np.float64), np.asarray(bank, dtype=np.float64)[nn]  # [N, H], [N, k, H]
    with np.errstate(invalid="ignore", divide="ignore"):
        if distance == "l2":
            return np.sqrt(((f[:, None, :] - p) ** 2).sum(-1)) / 4096
        return 1 - (f[:, None, :] * p).sum(-1) / (np.sqrt((f * f).sum(-1))[:, None] * np.sqrt((p * p).sum(-1)))


def lists(N: int, K: int, k: int, g) -> torch.Tensor:
    """int64 [N, k]: k different bank rows per node, every entry in 0 .. K - 1."""
    return torch.rand(N, K, generator=g).argsort(1)[:, :k].contiguous()


def grid(rows: int, cols: int, g) -> torch.Tensor:
    """f32 values on the half-integer grid -2 .. 2 (bf16-representable): most channels have tied sources."""
    return torch.randint(-4, 5, (rows, cols), generator=g).float() / 2
