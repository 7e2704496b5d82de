"""Round-once property of the bf16 instantiations (host only: no GPU, no library).

DESIGN.md section 2.2: in ``bf16`` mode a row kernel loads bf16, computes in f32 and rounds exactly once, at its store.  On
bf16-representable inputs the bf16 instantiation of a kernel must therefore write the bf16 rounding of what its f32 instantiation
writes.  ``check_round_once`` states that for one pair of tensors, ``check_same_f32`` handles the outputs that carry no storage
rounding.  The rest of this file is what tests/test_round_once_cpu.py and tests/test_gpu_round_once.py share: the shapes, the
inputs (a seed per case) and a plain-torch model of every op that runs in f32 or f64.

The cap of ``check_round_once``: the two instantiations run the same f32 operations in the same order and can differ only where the
compiler contracts a multiply-add in one and not in the other -- a few f32 ulps, about 1e-6 relative.  A bf16 step is 2^-8
relative, so a value sits within that noise of a rounding midpoint with probability of order 1e-3; a systematic relative error of
1e-4 moves about 2 % of the roundings (1.8 % measured on normal values).  1 % separates the two by an order of magnitude on each side.
"""
import math

import torch
import torch.nn.functional as F

BF = torch.bfloat16
CAP = 0.01        # share of elements whose rounding may differ from the rounded f32 twin, per tensor
INPUT_CAP = 0.001  # the same share between an f32 and an f64 evaluation of the reference: a tenth of the cap


def gen(seed):
    return torch.Generator().manual_seed(seed)


def r16(t):
    """The nearest bf16-representable f32 values."""
    return t.to(BF).float()


def bracket(r):
    """The two bf16 values (as f32) that bracket every element of the f32 tensor ``r``: toward zero and away from zero; equal
    where ``r`` is representable.  The spacing of bf16 halves below a power of two: the bit pattern takes care of that."""
    bits = r.contiguous().view(torch.int32)
    toward = bits & -65536  # 0xFFFF0000: drop the 16 low significand bits
    away = torch.where((bits & 0xFFFF) != 0, toward + 65536, toward)
    return toward.view(torch.float32), away.view(torch.float32)


def outside_bracket(g, r):
    """Number of elements of ``g`` (bf16 values) that are neither of the two bf16 neighbours of ``r`` (f32)."""
    lo, hi = bracket(r)
    g = g.float()
    return int((~((g == lo) | (g == hi))).sum())


def flip_share(g, r):
    """Share of the elements of ``g`` (bf16 values) that are not the round-to-nearest-even bf16 of ``r`` (f32)."""
    if g.numel() == 0:
        return 0.0
    return float((g.float() != r.to(BF).float()).double().mean())


def check_round_once(g, r, what, cap=CAP):
    """``g``: bf16 tensor of the bf16 instantiation, ``r``: f32 tensor of the f32 instantiation on the same representable inputs.
    1. every element of g is one of the two bf16 values that bracket r (never two steps away), everything finite;
    2. at most ``cap`` of the elements are the bracket value that is NOT r.to(bf16) (cap = 0: exact);
    3. returns that share."""
    assert g.dtype == BF, f"{what}: the bf16 run returned {g.dtype}"
    assert r.dtype == torch.float32, f"{what}: the f32 run returned {r.dtype}"
    assert g.shape == r.shape, f"{what}: shapes {tuple(g.shape)} / {tuple(r.shape)}"
    g, r = g.detach().cpu().float().contiguous(), r.detach().cpu().contiguous()
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(r).all()), f"{what}: non-finite values"
    lo, hi = bracket(r)
    outside = ~((g == lo) | (g == hi))
    if bool(outside.any()):
        i = int(outside.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(outside.sum())} of {g.numel()} elements are not a bf16 neighbour of the f32 twin; first at "
                             f"flat index {i}: bf16 run {g.flatten()[i].item()!r}, f32 run {r.flatten()[i].item()!r}")
    share = flip_share(g, r)
    assert share <= cap, f"{what}: {share:.4%} of the roundings differ from the rounded f32 twin (cap {cap:.2%})"
    return share


# Tolerances of the f32 side outputs: the ones tests/test_gpu_kernels.py uses for the same op against fp64 (rtol, atol).
F32_TOL = {
    "rowln.y": (1e-4, 1e-5), "rowln.dx": (1e-3, 1e-4), "rowln.dw": (1e-3, 1e-3), "rowln.db": (1e-3, 1e-3),  # test_rowln_fwd_bwd
    "rowln.mean": (1e-4, 1e-5), "rowln.rstd": (1e-4, 1e-5),                                                   # "all non-GEMM kernels"
    "graphln.y": (1e-4, 1e-5), "graphln.dx": (1e-3, 1e-4), "graphln.dw": (1e-3, 2e-3), "graphln.db": (1e-3, 2e-3),  # test_graphln_lrelu_fwd_bwd
    "graphln.stats": (1e-4, 1e-5),
    "csr": (1e-5, 1e-5),     # test_csr_gather_rows_with_hundreds_of_edges (f32)
    "pe": (1e-5, 2e-5),      # test_pe_add
    "norm": (1e-4, 1e-5),    # "all non-GEMM kernels"
    "colsum": (1e-4, 1e-5),
    "dropout": (1e-5, 1e-6),
    "gemm": (1e-3, 1e-3),    # test_gemm_bf16_memory_operands, f32 output
    "head.logits": (1e-4, 1e-4), "head.loss": (1e-4, 1e-4),  # test_one_logit_head... / test_two_logit_head... (f32)
}


def check_same_f32(a, b, rows, what):
    """Outputs without a storage rounding (statistics, parameter gradients, losses, logits): within the tolerance ``what`` names in
    F32_TOL; the grouped LayerNorm's partial-row reduction scales atol by sqrt(rows) as its f32 test does (``rows`` > 0 only there).
    Integer and uint8 outputs (keep masks, arg-max winners, gates): bit-equal."""
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{tuple(a.shape)} / {b.dtype}{tuple(b.shape)}"
    if not a.dtype.is_floating_point:
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} integer elements differ"
        return
    assert a.dtype in (torch.float32, torch.float64), f"{what}: {a.dtype} is a storage type, use check_round_once"
    rtol, atol = F32_TOL[what]
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol * (max(1.0, math.sqrt(rows)) if rows else 1.0), msg=lambda m: f"{what}: {m}")


def close_to_model(a, ref, what, rows=0):
    """The f32 run against the fp64 model, at the same tolerance: the pair cannot be wrong together."""
    check_same_f32(a.detach().cpu().double(), ref.detach().cpu().double(), rows, what)


# ---------------------------------------------------------------------------------------------------------------------------
# cases: shapes, inputs (CPU, bf16-representable activations; parameters stay f32) and plain-torch models in ``dt``
# ---------------------------------------------------------------------------------------------------------------------------
EPS, SLOPE = 1e-5, 0.2

ROWLN_SHAPES = [(37, 40), (5, 250), (130, 1024), (3, 1280), (66, 2048), (9, 4096)]
ROWLN_DROPOUT = (64, 1024, 0.5)
ROWLN_GROUP = (256, [64, 192, 5])
GRAPHLN_CASES = [(40, 32, [0, 40]), (64, 1024, [0, 10, 64]), (300, 256, [0, 100, 101, 300])]
CSR_GRAPHS = ["light", "heavy1", "cut"]
CSR_COLS = [32, 250, 1024]
BANDED_COLS = [1024, 250]
PE_COLS = [250, 1024]
GATHER_MAX = [(4, 256), (3, 1024), (8, 1024), (4, 320)]
SEGMAX = [((1, 0, 7, 300, 33), 260), ((32,) * 8, 1024)]
DROPOUT_N = [4096, 4099]
GEMM_SHAPES = [(130, 70, 40), (257, 129, 144), (128, 128, 64), (300, 200, 256)]
HEAD_SHAPES = [(77, 1000), (64, 1024)]


# Seeds: the first for which the reference alone (plain torch in f32 against f64) keeps every element inside its bracket and the
# share of differing roundings below INPUT_CAP (tests/test_round_once_cpu.py).  dx = rstd (g - s1 - xhat s2) cancels to 1e-5 of its
# terms on a handful of 135168 elements under seed 0 of the cases named here: there f32 evaluation noise alone is two bf16 steps.
ROWLN_SEEDS = {(66, 2048, True): 5, (9, 4096, True): 1}
CSR_SEED, BAND_SEED, PE_SEED, GEMM_SEED = 1, 1, 4, 1  # (likewise: the first seed that holds for every width / shape of the family)


def rowln_inputs(rows, cols, seed=0):
    g = gen(1000 + rows * 7 + cols + seed)
    x = r16(torch.randn(rows, cols, generator=g) * 2 + 0.3)
    dy = r16(torch.randn(rows, cols, generator=g))
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    return dict(x=x, dy=dy, w=w, b=b)


def rowln_model(inp, dt, relu, mask=None, p=0.0):
    x, w, b = (inp[k].detach().clone().to(dt).requires_grad_(True) for k in ("x", "w", "b"))
    y = F.layer_norm(x, (x.shape[1],), w, b, EPS)
    y = torch.relu(y) if relu else y
    if mask is not None:
        y = y * mask.to(dt) / (1 - p)
    y.backward(inp["dy"].to(dt))
    xd = x.detach()
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad, mean=xd.mean(1),
                rstd=1 / torch.sqrt(xd.var(1, unbiased=False) + EPS))


def rowln_group_inputs(seed=0):
    cols, rows = ROWLN_GROUP
    g = gen(2000 + seed)
    n = sum(rows)
    return dict(x=r16(torch.randn(n, cols, generator=g) * 2 + 0.3), dy=r16(torch.randn(n, cols, generator=g)),
                ws=[torch.randn(cols, generator=g) for _ in rows], bs=[torch.randn(cols, generator=g) for _ in rows])


def rowln_group_model(inp, dt):
    """One dict of ``rowln_model`` per row range."""
    out, lo = [], 0
    for k, n in enumerate(ROWLN_GROUP[1]):
        out.append(rowln_model(dict(x=inp["x"][lo:lo + n], dy=inp["dy"][lo:lo + n], w=inp["ws"][k], b=inp["bs"][k]), dt, True))
        lo += n
    return out


def graphln_inputs(rows, cols, seed=0):
    g = gen(3000 + rows + cols + seed)
    x = r16(torch.randn(rows, cols, generator=g) * 1.5 + 0.2)
    dy = r16(torch.randn(rows, cols, generator=g))
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    return dict(x=x, dy=dy, w=w, b=b)


def graphln_model(inp, dt, segs):
    """LeakyReLU(gnn.LayerNorm(mode='graph')) per row segment: statistics over all elements of the segment, eps added to the std."""
    x, w, b = (inp[k].detach().clone().to(dt).requires_grad_(True) for k in ("x", "w", "b"))
    ys, stats = [], []
    for s, e in zip(segs[:-1], segs[1:]):
        xs = x[s:e]
        mean, std = xs.mean(), xs.std(unbiased=False)
        ys.append(F.leaky_relu((xs - mean) / (std + EPS) * w + b, SLOPE))
        stats += [mean.detach(), 1 / (std.detach() + EPS)]
    y = torch.cat(ys)
    y.backward(inp["dy"].to(dt))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad, stats=torch.stack(stats))


def csr_edges(kind):
    """(edge_index, num_nodes).  light: band and LTA sequences with short rows and isolated rows; heavy1: LTA sequences of T = 32
    (the fan-out node has 31 out-edges: listed, summed inside the launch) plus a fan-in node; cut: T = 70, B = 2 (out-degree 69 >
    64: cut over several workgroups)."""
    from egopack_amd import data as D
    g = gen(17)
    if kind == "light":
        e1 = D.radius_band_edges(torch.arange(9) - 4, 2)
        y = torch.stack([torch.randint(1, 5, (12,), generator=g), torch.randint(0, 5, (12,), generator=g)], 1)
        y[:2] = -1
        e2 = D.lta_connectivity_edges(torch.arange(12), y, 1.5) + 9
        return torch.cat([e1, e2], 1), 9 + 12 + 3
    T, B = (32, 2) if kind == "heavy1" else (70, 2)
    eis, off = [], 0
    for _ in range(B):
        y = torch.ones(T, 2, dtype=torch.long)
        y[:2] = -1
        ei = D.lta_connectivity_edges(torch.arange(T), y, 1.5)
        fan_in = torch.stack([torch.arange(3, T), torch.full((T - 3,), 2)])  # every later node -> node 2
        eis.append(torch.cat([ei, fan_in], 1) + off)
        off += T
    return torch.cat(eis, 1), off


def band_edges():
    """Band sequences only (radius 1): every row of the by-target CSR is coded, plus two isolated rows."""
    from egopack_amd import data as D
    parts, n = [], 0
    for T in (9, 32, 5, 1, 12):
        parts.append(D.radius_band_edges(torch.arange(T), 1) + n)
        n += T
    return torch.cat(parts, 1), n + 2


def csr_inputs(n, cols, seed=0):
    g = gen(4000 + n + cols + seed)
    return dict(x=r16(torch.randn(n, cols, generator=g)), gate=r16(torch.randn(n, cols, generator=g)))


def csr_model(inp, dt, ei, n):
    """fwd: mean over the in-edges (0 without any), as the reference forms it: the sum, then one division by the count (sums of a
    few bf16 values are exact in f32, so exact zeros and exact rounding midpoints -- one mean of three in ten is one -- come out
    the same in f32 and f64); bwd: the transposed gather weighted by 1 / in-degree(target), gated by gate > 0 -- as the backward of
    that mean: each row divided by its count, then summed over the out-edges (a / 3 + b / 2 with a = -1.5 b is an exact zero)."""
    A = torch.zeros(n, n, dtype=dt)
    A.index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=dt), accumulate=True)
    deg = A.sum(1).clamp(min=1)[:, None]
    x = inp["x"].to(dt)
    return dict(fwd=(A @ x) / deg, bwd=(A.t() @ (x / deg)) * (inp["gate"].to(dt) > 0))


def pe_inputs(cols, seed=0):
    g = gen(5000 + cols + seed)
    rows = 50
    return dict(x=r16(torch.randn(rows, cols, generator=g)), pos=torch.randint(-64, 64, (rows,), generator=g),
                freq=torch.logspace(0, 1, cols // 2, 1e-4))


def pe_model(inp, dt):
    arg = inp["pos"].to(dt).view(-1, 1) * inp["freq"].to(dt).view(1, -1)
    return dict(y=inp["x"].to(dt) + torch.cat([torch.sin(arg), torch.cos(arg)], -1))


def dropout_inputs(n, seed=0):
    g = gen(6000 + n + seed)
    return dict(x=r16(torch.randn(n, generator=g)), dy=r16(torch.randn(n, generator=g)))


def dropout_model(inp, dt, mask, p):
    m = mask.to(dt)
    return dict(y=inp["x"].to(dt) * m / (1 - p), dx=inp["dy"].to(dt) * m / (1 - p))


def gemm_inputs(M, N, K, seed=0):
    g = gen(7000 + M * 7 + N * 3 + K + seed)
    return dict(A=r16(torch.randn(M, K, generator=g)), B=r16(torch.randn(N, K, generator=g)), bias=torch.randn(N, generator=g),
                res=r16(torch.randn(M, N, generator=g)))


def gemm_model(inp, dt):
    """relu(A B^T + bias) + residual (the epilogue order of egk_gemm)."""
    return dict(c=torch.relu(inp["A"].to(dt) @ inp["B"].to(dt).t() + inp["bias"].to(dt)) + inp["res"].to(dt))


def gather_max_inputs(k, H, seed=0):
    g = gen(8000 + k * 5 + H + seed)
    G, N, K = 3, 40, 37
    banks = [torch.randn(K, H, generator=g) for _ in range(G)]
    nns = [torch.stack([torch.randperm(K, generator=g)[:k] for _ in range(N)]) for _ in range(G)]
    f = r16(torch.randn(G * N, H, generator=g))
    f[5] = r16(banks[0][nns[0][5, 1]])  # (ties with a rounded prototype row only where the prototype row is representable)
    return dict(banks=banks, nns=nns, f=f, dm=r16(torch.randn(G * N, H, generator=g)), N=N)


def segmax_inputs(lens, cols, n_src=3, seed=0):
    g = gen(9000 + sum(lens) + cols + seed)
    ptr = torch.tensor([0, *torch.tensor(lens).cumsum(0).tolist()], dtype=torch.int32)
    rows = int(ptr[-1])
    return dict(ptr=ptr, xs=[r16(torch.randn(rows, cols, generator=g)) for _ in range(n_src)],
                douts=[r16(torch.randn(len(lens), cols, generator=g)) for _ in range(n_src)])


def head_inputs(rows, cols, n_out, seed=0):
    g = gen(10000 + rows + cols + n_out + seed)
    y = torch.randint(0, 2, (rows,), generator=g)
    if n_out == 2:
        y[::5] = -1
    return dict(f=r16(torch.randn(rows, cols, generator=g)), W=r16(torch.randn(n_out, cols, generator=g) * 0.05),
                b=torch.randn(n_out, generator=g), y=y, seed=0.7 / rows)


def head_model(inp, n_out, smoothing=0.0):
    """fp64 model of the one-logit (BCE) and two-logit (cross entropy) heads with the DESIGNED second rounding of their bf16 form:
    z = f W^T + b, the loss of z, g = seed * dloss/dz ROUNDED to bf16 (the operand type of the contraction path these launches
    replace), df = g W (rounded once more at its store), dW = g^T f, db = sum g.  Returns the f64 values before df's storage rounding,
    for both gradients: ``g`` unrounded (the f32 form) and rounded (the bf16 form)."""
    f, W, b, y, seed = inp["f"].double(), inp["W"].double(), inp["b"].double(), inp["y"], inp["seed"]
    z = f @ W.t() + b
    if n_out == 1:
        z = z.squeeze(1)
        loss = F.binary_cross_entropy_with_logits(z, y.double(), reduction="none")
        g = ((torch.sigmoid(z) - y.double()) * seed).unsqueeze(1)
    else:
        loss = F.cross_entropy(z, y, reduction="none", ignore_index=-1, label_smoothing=smoothing)
        live = (y >= 0).double().unsqueeze(1)
        tgt = F.one_hot(y.clamp(min=0), 2).double() * (1 - smoothing) + smoothing / 2
        g = seed * (torch.softmax(z, 1) - tgt) * live
    g16 = g.float().to(BF).double()
    return dict(logits=z, loss=loss, g=g, g16=g16, df=g @ W, df16=g16 @ W, dw=g.t() @ f, dw16=g16.t() @ f, db=g.sum(0), db16=g16.sum(0))
