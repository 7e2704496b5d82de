"""Host model of include/egopack_class_report.h in numpy, written from the definitions (not from the kernel), and the input
builders the GPU tests of the report share.

Ranking of a row: classes sorted by (-value, index) with a NaN below -inf (NaNs among themselves by index); top1 is the first,
top2 the second (none when C == 1).  A row whose label t is < 0 or >= C counts as ignored and touches nothing else; otherwise
    counts[0] += 1,  confusion[t, top1] += 1,  top2[t, top1] += 1 when top1 != t and top2 == t,
    loss_q24[t] += rint(loss * 2^24) for a loss that is finite and whose product is below 2^63 in magnitude, else counts[2] += 1.
The per-row f32 loss is GIVEN to the model (the GPU test takes it from ops.cross_entropy on the same tensors: the report forms
its loss with the same row function, so the fixed-point sums must agree in every bit)."""
import numpy as np
import torch

Q24 = float(1 << 24)


def order(x: np.ndarray) -> np.ndarray:
    """[N, C] class indices of every row from best to worst."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    neg = np.where(nan, 0.0, -x.astype(np.float64)) + 0.0  # (-0.0 + 0.0 = +0.0: the two zeros tie)
    idx = np.broadcast_to(np.arange(x.shape[1]), x.shape)
    return np.lexsort((idx, neg, nan.astype(np.int8)), axis=-1)  # (last key first: non-NaN, then the value, then the index)


def loss_q(loss_rows: np.ndarray):
    """(q int64, ok bool) per row of an f32 loss vector."""
    loss = np.asarray(loss_rows, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        q = loss * np.float32(Q24)
        ok = np.isfinite(q) & (np.abs(q) < np.float32(2.0 ** 63))
    return np.rint(np.where(ok, q, 0).astype(np.float64)).astype(np.int64), ok


def model(x, y, loss_rows=None, want_top2=True):
    """(confusion [C, C], top2 [C, C], loss_q24 [C], counts [4]) as int64 numpy arrays for logits x [N, C], labels y [N] and the
    per-row f32 losses (None: no loss sums, no non-finite count)."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.int64)
    N, C = x.shape
    conf, top2 = np.zeros((C, C), np.int64), np.zeros((C, C), np.int64)
    q24, counts = np.zeros(C, np.int64), np.zeros(4, np.int64)
    valid = (y >= 0) & (y < C)
    counts[0], counts[1] = int(valid.sum()), int((~valid).sum())
    if N == 0:
        return conf, top2, q24, counts
    o = order(x)
    t, t1 = y[valid], o[valid, 0]
    np.add.at(conf, (t, t1), 1)
    if C > 1 and want_top2:
        t2 = o[valid, 1]
        m = (t1 != t) & (t2 == t)
        np.add.at(top2, (t[m], t1[m]), 1)
    if loss_rows is not None:
        q, ok = loss_q(np.asarray(loss_rows)[valid])
        np.add.at(q24, t[ok], q[ok])
        counts[2] = int((~ok).sum())
    return conf, top2, q24, counts


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def logits(rows, C, g, ties=False):
    """f32 [rows, C]: a few thousand distinct values on a 2^-10 grid, or integers in -2 .. 2 (ties for first and second place)."""
    if ties:
        return torch.randint(-2, 3, (rows, C), generator=g).float()
    return torch.randint(-8192, 8193, (rows, C), generator=g).float() / 1024.0


def labels(rows, C, g):
    """int64 [rows, 2]: column 0 holds the labels (rows 3, 10, 17, .. -1; row 1 the out-of-range value C when there are at least
    five rows -- the smallest batches keep all their rows), column 1 a poison."""
    y = torch.full((rows, 2), -5, dtype=torch.int64)
    y[:, 0] = torch.randint(0, C, (rows,), generator=g)
    y[3::7, 0] = -1
    if rows >= 5:
        y[1, 0] = C
    return y


def padded(x, pad=4):
    """``x`` as a [rows, C] view of a [rows, C + pad] tensor whose padding holds NaN (same device as x)."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


class State:
    """The four int64 accumulators of one head on a device, zeroed (or pre-filled)."""

    def __init__(self, C, device, fill=0):
        self.C = C
        self.confusion = torch.full((C, C), fill, dtype=torch.int64, device=device)
        self.top2 = torch.full((C, C), fill, dtype=torch.int64, device=device)
        self.loss_q24 = torch.full((C,), fill, dtype=torch.int64, device=device)
        self.counts = torch.full((4,), fill, dtype=torch.int64, device=device)

    def tensors(self):
        return [self.confusion, self.top2, self.loss_q24, self.counts]


def assert_state(state, ref, what="", fill=0):
    for name, got, want in zip(("confusion", "top2", "loss_q24", "counts"), state.tensors(), ref):
        want = torch.from_numpy(np.asarray(want)) + fill
        got = got.cpu()
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{what} {name}: {bad.shape[0]} of {got.numel()} cells differ, first at {bad[0].tolist()}: got "
                                 f"{got[tuple(bad[0])].item()}, expected {want[tuple(bad[0])].item()}")
