"""Host model of include/egopack_action.h in numpy, written from the definitions (not from the kernel), and the input builders the
tests of the two launches share.

``model`` takes the launch's own ``lse`` as input -- how a log-sum-exp is summed is the row function's business, checked apart
(bit for bit against ``egk_topk_softmax``'s, and against float64 at ``topk_common.PROB_TOL``) -- and forms in f32, one rounding per
operation: x = z (or fl(beta z)), a = fl(x_v - lse_v), b = fl(y_n - lse_n), the FULL [Cv, Cn] table s = fl(a + b), and the order by
a lexicographic sort over (score, the verb's place in its head's order, the noun's place in its head's order); a NaN score is below
-inf and all NaN scores tie.  The order of a head is ``class_report_common.order`` (imported, not copied).  Pairs, ``logp`` and
``rank`` of the launch are compared with the model's bit for bit.  ``levenshtein`` is the plain-Python edit distance over tokens."""
import numpy as np
import torch

from tests.class_report_common import order
from tests.topk_common import logsumexp64

f32 = np.float32


def scaled(z: np.ndarray, beta) -> np.ndarray:
    """x of a head: the f32 logits, or fl(beta * z) as one f32 product per element."""
    z = np.asarray(z, dtype=f32)
    return z if beta is None else (f32(beta) * z).astype(f32)


def places(x: np.ndarray) -> np.ndarray:
    """int64 [N, C]: the place of every class in its row's order (0 = best)."""
    o = order(x)
    p = np.empty_like(o)
    np.put_along_axis(p, o, np.broadcast_to(np.arange(x.shape[1]), x.shape), axis=1)
    return p


def table(zv, zn, lse, beta=None):
    """(s f32 [N, Cv, Cn], the verbs' places [N, Cv], the nouns' places [N, Cn])."""
    xv, xn = scaled(zv, None if beta is None else beta[0]), scaled(zn, None if beta is None else beta[1])
    lse = np.asarray(lse, dtype=f32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (xv - lse[:, :1]).astype(f32)
        b = (xn - lse[:, 1:]).astype(f32)
        s = (a[:, :, None] + b[:, None, :]).astype(f32)
    return s, places(xv), places(xn)


def pair_order(s_row: np.ndarray, pv_row: np.ndarray, pn_row: np.ndarray) -> np.ndarray:
    """The flat indices v * Cn + n of one row's pairs from best to worst."""
    Cv, Cn = s_row.shape
    nan = np.isnan(s_row)
    neg = np.where(nan, 0.0, -s_row.astype(np.float64)) + 0.0  # (the two zeros tie)
    pv = np.broadcast_to(pv_row[:, None], (Cv, Cn))
    pn = np.broadcast_to(pn_row[None, :], (Cv, Cn))
    return np.lexsort((pn.reshape(-1), pv.reshape(-1), neg.reshape(-1), nan.reshape(-1).astype(np.int8)))  # (last key first)


def model(zv, zn, lse, k: int, labels=None, beta=None):
    """(pair int64 [N, k, 2], logp f32 [N, k], rank int32 [N] | None, the full orders: a list of flat-index arrays)."""
    s, pv, pn = table(zv, zn, lse, beta)
    N, Cv, Cn = s.shape
    pair = np.full((N, k, 2), -1, dtype=np.int64)
    logp = np.full((N, k), -np.inf, dtype=f32)
    rank = None if labels is None else np.full(N, -1, dtype=np.int32)
    orders = []
    for r in range(N):
        o = pair_order(s[r], pv[r], pn[r])
        orders.append(o)
        m = min(k, Cv * Cn)
        pair[r, :m, 0], pair[r, :m, 1] = o[:m] // Cn, o[:m] % Cn
        logp[r, :m] = s[r].reshape(-1)[o[:m]]
        if labels is not None:
            yv, yn = int(labels[0][r]), int(labels[1][r])
            if 0 <= yv < Cv and 0 <= yn < Cn:
                rank[r] = int(np.nonzero(o == yv * Cn + yn)[0][0])
    return pair, logp, rank, orders


def lse32(zv, zn, beta=None) -> np.ndarray:
    """f32 [N, 2]: the float64 log-sum-exps of both heads, rounded -- a stand-in for the launch's where there is no launch."""
    xv, xn = scaled(zv, None if beta is None else beta[0]), scaled(zn, None if beta is None else beta[1])
    return np.stack([logsumexp64(xv), logsumexp64(xn)], 1).astype(f32)


def prob64(zv, zn, pair, beta=None) -> np.ndarray:
    """float64 [N, k]: exp of the float64 log-probability of every exported pair (0 for a (-1, -1) entry)."""
    xv, xn = scaled(zv, None if beta is None else beta[0]).astype(np.float64), scaled(zn, None if beta is None else beta[1]).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        lv, ln = xv - logsumexp64(xv)[:, None], xn - logsumexp64(xn)[:, None]
        rows = np.arange(pair.shape[0])[:, None]
        live = pair[:, :, 0] >= 0
        s = lv[rows, np.maximum(pair[:, :, 0], 0)] + ln[rows, np.maximum(pair[:, :, 1], 0)]
        return np.where(live, np.exp(s), 0.0)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def grid(rows: int, C: int, g) -> torch.Tensor:
    """f32 [rows, C]: multiples of 0.25 in [-1.5, 1.5] (bf16 values too) -- thirteen values, so ties dominate."""
    return torch.randint(-6, 7, (rows, C), generator=g).float() / 4.0


def smooth(rows: int, C: int, g) -> torch.Tensor:
    """f32 [rows, C]: bf16-representable values in about [-8, 8] on a 2^-4 grid, few ties."""
    return torch.randint(-128, 129, (rows, C), generator=g).float() / 16.0


def pair_labels(rows: int, Cv: int, Cn: int, g) -> torch.Tensor:
    """int64 [rows, 3]: verb labels in column 0, noun labels in column 2, a poison between them.  Row 1 has a negative verb, row 2
    a noun label of Cn (out of range), row 3 both -1, when there are that many rows."""
    y = torch.full((rows, 3), -7, dtype=torch.int64)
    y[:, 0] = torch.randint(0, Cv, (rows,), generator=g)
    y[:, 2] = torch.randint(0, Cn, (rows,), generator=g)
    if rows > 1:
        y[1, 0] = -1
    if rows > 2:
        y[2, 2] = Cn
    if rows > 3:
        y[3, 0], y[3, 2] = -1, -1
    return y


def levenshtein(a, b) -> int:
    """The edit distance between two token sequences (any hashable tokens: a pair token is a tuple)."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def edit_model(pred_v, pred_n, label_v, label_n) -> np.ndarray:
    """int32 [N, K, 3] of pred [N, Z, K] and label [N, Z] (integer arrays): verb, noun and action distances."""
    pv, pn, lv, ln = (np.asarray(t) for t in (pred_v, pred_n, label_v, label_n))
    N, Z, K = pv.shape
    out = np.zeros((N, K, 3), dtype=np.int32)
    for n in range(N):
        for k in range(K):
            out[n, k, 0] = levenshtein(pv[n, :, k].tolist(), lv[n].tolist())
            out[n, k, 1] = levenshtein(pn[n, :, k].tolist(), ln[n].tolist())
            out[n, k, 2] = levenshtein(list(zip(pv[n, :, k].tolist(), pn[n, :, k].tolist())), list(zip(lv[n].tolist(), ln[n].tolist())))
    return out


def futures(N: int, Z: int, K: int, g, n_verbs: int = 3, n_nouns: int = 2):
    """(pred_v, pred_n int64 [N, Z, K], label_v, label_n int64 [N, Z]) from few classes, so that partial matches (verb right, noun
    wrong) are frequent; future 0 of sequence 0 is the label itself (distance 0)."""
    pv, pn = torch.randint(0, n_verbs, (N, Z, K), generator=g), torch.randint(0, n_nouns, (N, Z, K), generator=g)
    lv, ln = torch.randint(0, n_verbs, (N, Z), generator=g), torch.randint(0, n_nouns, (N, Z), generator=g)
    if N and K:
        pv[0, :, 0], pn[0, :, 0] = lv[0], ln[0]
    return pv, pn, lv, ln
