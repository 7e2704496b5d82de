"""Host model of the edge-drop launches (include/egopack_edge_drop.h), built on tests/philox_ref.py.

Nothing is imported from ``egopack_amd`` at module level: numpy integer arithmetic for the keep bits (every comparison with the
device's bits is exact), float64 for the two launches.

  edge j -> i          (a, b) = (min(i, j), max(i, j)) in symmetric mode, (i, j) otherwise
  counter, key         offset + word + a (mod 2^64),  seed ^ (b << 32)
  keep                 word 0 of Philox4x32-10 under philox_ref.keep_from_words; with keep_self an edge i -> i is always kept
  a launch's counters  [offset + word, offset + word + rows): ``intervals``; the caller reserves rows + 64 (``reserved``)
"""
import numpy as np
import torch

from tests import philox_ref as PR

SYMMETRIC, KEEP_SELF = 1, 2


def flags_of(symmetric: bool, keep_self: bool) -> int:
    return (SYMMETRIC if symmetric else 0) | (KEEP_SELF if keep_self else 0)


def keep_edges(dst, src, seed, offset, p, symmetric=True, keep_self=True, word=0):
    """uint8 [E]: the keep bit of every edge src[e] -> dst[e]."""
    i, j = np.asarray(dst, dtype=np.int64), np.asarray(src, dtype=np.int64)
    a, b = (np.minimum(i, j), np.maximum(i, j)) if symmetric else (i, j)
    base = (int(offset) + int(word)) & PR.MASK64
    with np.errstate(over="ignore"):
        ctr = np.uint64(base) + a.astype(np.uint64)
    key_lo = np.full(i.shape, int(seed) & PR.MASK32, dtype=np.uint64)
    key_hi = (np.uint64((int(seed) >> 32) & PR.MASK32) ^ b.astype(np.uint64)) & np.uint64(PR.MASK32)  # seed ^ (b << 32): the high word
    zero = np.zeros_like(ctr)
    words = PR.philox4x32_10(ctr & np.uint64(PR.MASK32), ctr >> np.uint64(32), zero, zero, key_lo, key_hi)
    keep = PR.keep_from_words(words[..., 0], p)
    if keep_self:
        keep = np.where(i == j, np.uint8(1), keep)
    return keep.astype(np.uint8)


def rows_of(rowptr):
    rp = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), rp[1:] - rp[:-1])


def keep_fwd(graph, seed, offset, p, symmetric=True, keep_self=True, word=0):
    """Keep bits in the order of ``graph.col`` (row = destination, col = source)."""
    return keep_edges(rows_of(graph.rowptr.cpu().numpy()), graph.col.cpu().numpy(), seed, offset, p, symmetric, keep_self, word)


def keep_bwd(graph, seed, offset, p, symmetric=True, keep_self=True, word=0):
    """Keep bits in the order of ``graph.t_col`` (row = source, t_col = destination)."""
    return keep_edges(graph.t_col.cpu().numpy(), rows_of(graph.t_rowptr.cpu().numpy()), seed, offset, p, symmetric, keep_self, word)


def thin(edge_index, seed, offset, p, symmetric=True, keep_self=True, word=0):
    """The kept edges of ``edge_index`` [2, E] (row 0 = source, row 1 = destination), in its order.  ``build_csr`` sorts stably, so
    the thinned graph lists the kept edges of every row in the order the full graph lists them, in BOTH orientations."""
    ei = edge_index.cpu().numpy()
    k = keep_edges(ei[1], ei[0], seed, offset, p, symmetric, keep_self, word).astype(bool)
    return edge_index[:, torch.from_numpy(k)]


def edge_set(dst, src, keep):
    k = np.asarray(keep).astype(bool)
    return set(zip(np.asarray(dst)[k].tolist(), np.asarray(src)[k].tolist()))


def intervals(offset, rows, word=0):
    """The counters one launch may draw, as a half-open interval of Python integers."""
    return [(int(offset) + int(word), int(offset) + int(word) + int(rows))]


def reserved(rows):
    """Counters the caller reserves per launch: ``ops._next_rng(4 * rows)``."""
    return int(rows) + 64


# ---- float64 models of the two launches ------------------------------------------------------------------------------------------
def fwd_model(x, graph, keep):
    """(out float64 [rows, cols], cnt int64 [rows]): the mean over the kept in-edges, 0 for a row without one."""
    x = x.double().cpu()
    k = torch.from_numpy(np.asarray(keep).astype(bool))
    dst = torch.from_numpy(rows_of(graph.rowptr.cpu().numpy()))[k]
    src = graph.col.cpu().long()[k]
    out = torch.zeros_like(x)
    out.index_add_(0, dst, x[src])
    cnt = torch.bincount(dst, minlength=x.shape[0])
    return out / cnt.clamp(min=1).double()[:, None], cnt


def bwd_model(dout, graph, keep_t, cnt, gate=None):
    """dx float64: sum over the kept transposed edges j -> i of dout[i] / cnt[i], gated by gate[j] > 0."""
    dout = dout.double().cpu()
    k = torch.from_numpy(np.asarray(keep_t).astype(bool))
    src = torch.from_numpy(rows_of(graph.t_rowptr.cpu().numpy()))[k]
    dst = graph.t_col.cpu().long()[k]
    dx = torch.zeros_like(dout)
    dx.index_add_(0, src, dout[dst] / cnt.clamp(min=1).double()[dst][:, None])
    if gate is not None:
        dx = torch.where(gate.double().cpu() > 0, dx, torch.zeros_like(dx))
    return dx


def inv_deg_bits(cnt):
    """f32 [rows]: 1 / cnt correctly rounded, 0 where cnt == 0."""
    c = np.asarray(cnt, dtype=np.float32)
    with np.errstate(divide="ignore"):
        return torch.from_numpy(np.where(c > 0, np.float32(1.0) / c, np.float32(0.0)).astype(np.float32))


def mean_ref(x, edge_index, rows):
    """Differentiable float64 mean aggregation over ``edge_index`` (autograd reference on a thinned graph)."""
    src, dst = edge_index[0].long().to(x.device), edge_index[1].long().to(x.device)
    out = torch.zeros((rows, x.shape[1]), dtype=x.dtype, device=x.device).index_add(0, dst, x[src])
    cnt = torch.bincount(dst, minlength=rows).clamp(min=1).to(x.dtype)
    return out / cnt[:, None]


# ---- the graphs of the GPU tests: (edge_index [2, E], rows) ------------------------------------------------------------------------
def band_graph():
    """Two sequences, a band of 9 nodes (radius 2) and an LTA graph of 12, plus 3 isolated rows: the graph of
    test_csr_mean_aggregate_fwd_bwd (tests/test_gpu_kernels.py)."""
    from egopack_amd import data
    e1 = data.radius_band_edges(torch.arange(9) - 4, 2)
    y = torch.ones(12, 2, dtype=torch.long)
    y[:2] = -1
    e2 = data.lta_connectivity_edges(torch.arange(12), y, 1.5) + 9
    return torch.cat([e1, e2], dim=1), 9 + 12 + 3


def lta_graph():
    """An LTA graph of 34 nodes (the last input clip fans out to the 32 forecast nodes) in which node 2 has 31 in-edges: its two
    band neighbours and the nodes 4 .. 32."""
    from egopack_amd import data
    T = 34
    y = torch.ones(T, 2, dtype=torch.long)
    y[:2] = -1
    ei = data.lta_connectivity_edges(torch.arange(T), y, 1.5)
    fan_in = torch.stack([torch.arange(4, 33), torch.full((29,), 2)])
    return torch.cat([ei, fan_in], dim=1), T


def wrap_graph():
    """Row 3 has 70 in-edges, row 5 has 70 out-edges (the 64-edge batch wraps in both orientations), plus self loops."""
    n = 80
    others = torch.arange(8, 78)
    ein = torch.stack([others, torch.full_like(others, 3)])
    eout = torch.stack([torch.full_like(others, 5), others])
    loops = torch.stack([torch.arange(0, n, 7), torch.arange(0, n, 7)])
    return torch.cat([ein, eout, loops], dim=1), n


def single_graph():
    """rows = 1 with a self loop only."""
    return torch.zeros(2, 1, dtype=torch.long), 1


GRAPHS = {"band": band_graph, "lta": lta_graph, "wrap": wrap_graph, "single": single_graph}
