"""Layout tests of the autograd ops: every tensor argument of every public differentiable op of ``egopack_amd.ops``, and the
gradient of every output, in the layouts PyTorch produces -- padded rows, the second block of a ``cat(dim=1)`` (odd row stride,
unaligned pointer), transposed, every other row, and the broadcast gradients of ``sum(0)`` / ``sum()``.  What autograd really
hands out is pinned on the CPU in tests/test_layouts_cpu.py.

Every case runs the op twice through ``ops`` only: once with ONE operand as such a view, once on ``.contiguous()`` copies, and
asserts
  1. outputs and all gradients equal the plain torch float64 reference of the operation on the packed values (tolerances
     restated from tests/test_gpu_kernels.py / tests/test_gpu_models.py, named at every case; bf16: the reference takes the
     bf16-rounded operands those tests use);
  2. both runs give the same bits;
  3. nothing holds a NaN;
  4. the backing buffer of the view keeps its bits.
The backing buffers hold NaN (-1 for integers) everywhere outside the view, and at least rows * cols elements counted from the
view's first element: a launch that wrongly reads the view as packed returns NaN or a wrong number without leaving the
allocation."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16

FWD_TAGS = ("ld_aligned", "ld_offset", "col_major", "row_step")
GRAD_TAGS = ("packed", "ld_aligned", "ld_offset", "col_major", "row_step", "bcast_rows", "bcast_all")
VEC_FWD_TAGS = ("column",)
VEC_GRAD_TAGS = ("packed", "column", "bcast")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------
# the layouts
# ---------------------------------------------------------------------------------------------------------
def poison(shape, dtype, device):
    """NaN (floats) / -1 (integers) everywhere."""
    if dtype.is_floating_point:
        return torch.full(shape, float("nan"), dtype=dtype, device=device)
    return torch.full(shape, -1, dtype=dtype, device=device)


def lay_values(values, tag):
    """The packed values the view of ``lay`` holds: ``values`` itself, or its first row / first element broadcast."""
    if tag in ("bcast_rows", "bcast"):
        return values[0:1].expand(values.shape).contiguous()
    if tag == "bcast_all":
        return values[0:1, 0:1].expand(values.shape).contiguous()
    return values


def lay(values, tag):
    """(view, backing buffer): a view in layout ``tag`` that holds ``lay_values(values, tag)``, inside a buffer that is NaN / -1
    everywhere else and holds >= numel elements from the view's first element on.  2-D tags: the table of the module docstring;
    1-D tags: ``packed``, ``column`` (``big[:, 3]`` of [n, 8]) and ``bcast`` (``buf[0].expand(n)``, buf [n + 1])."""
    dt, dev = values.dtype, values.device
    if tag == "packed":
        big = values.clone()
        return big, big
    if values.dim() == 1:
        n = values.shape[0]
        if tag == "column":
            big = poison((n, 8), dt, dev)
            view = big[:, 3]
        elif tag == "bcast":
            big = poison((n + 1,), dt, dev)
            big[0] = values[0]
            return big[0].expand(n), big
        else:
            raise ValueError(tag)
        view.copy_(values)
        return view, big
    rows, cols = values.shape
    if tag == "ld_aligned":
        big = poison((rows, cols + (16 if dt == BF else 8)), dt, dev)
        view = big[:, :cols]
    elif tag == "ld_offset":
        big = poison((rows, cols + 13), dt, dev)
        view = big[:, 5:5 + cols]
    elif tag == "col_major":
        big = poison((cols, rows), dt, dev)
        view = big.t()
    elif tag == "row_step":
        big = poison((2 * rows, cols), dt, dev)
        view = big[::2]
    elif tag == "bcast_rows":
        big = poison((rows + 1, cols), dt, dev)
        big[0] = values[0]
        return big[0:1].expand(rows, cols), big
    elif tag == "bcast_all":
        big = poison((rows + 1, cols), dt, dev)
        big[0, 0] = values[0, 0]
        return big.view(-1)[0].expand(rows, cols), big
    else:
        raise ValueError(tag)
    view.copy_(values)
    return view, big


def expected_layout(tag, rows, cols, dt):
    """(strides, storage offset) of ``lay`` for a [rows, cols] tensor (checked in tests/test_layouts_cpu.py)."""
    return {"packed": ((cols, 1), 0), "ld_aligned": ((cols + (16 if dt == BF else 8), 1), 0), "ld_offset": ((cols + 13, 1), 5),
            "col_major": ((1, rows), 0), "row_step": ((2 * cols, 1), 0), "bcast_rows": ((0, 1), 0), "bcast_all": ((0, 0), 0)}[tag]


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ---------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def r16(t):
    return t.to(BF).float()


def rnd(dt, *shape, g, scale=1.0, shift=0.0):
    t = torch.randn(*shape, generator=g) * scale + shift
    return r16(t) if dt == BF else t


def distinct(rows, cols, g):
    """Small integers, distinct inside every column (exact in bf16): a max over rows has one winner."""
    return (torch.argsort(torch.rand(rows, cols, generator=g), 0).float() - rows // 2)


# tolerances (rtol, atol), restated from the existing tests
GEMM_F32 = dict(out=(1e-4, 1e-3), gin=(1e-4, 2e-3), gpar=(1e-4, 2e-3))   # test_linear_autograd_two_source_residual (tol 1e-4)
GEMM_BF = dict(out=(1e-2, 3e-2), gin=(2e-2, 6e-2), gpar=(2e-2, 6e-2))    # test_linear_autograd_full_bf16
OUT16 = (8e-3, 8e-3)                                                     # test_gpu_kernels.OUT16
EXACT = dict(out=(0, 0), gin=(0, 0), gpar=(0, 0))


def gemm_tol(dt):
    return GEMM_F32 if dt == F32 else GEMM_BF


class Case:
    """One op at one shape.  ``make(dt)`` -> (ins, params, ints): CPU tensors -- ``ins`` the differentiable operands (values
    representable in the element type they are fed in), ``params`` f32 parameters, ``ints`` integer operands;
    ``call(ops, ins, params, ints)`` -> tuple of device outputs; ``ref(ins, params, ints, hint)`` -> the same in float64 (``hint``:
    the outputs of the packed run, for what only the device knows: a dropout mask; ``ints["_dt"]``: the element type of the run); ``tol(dt)`` -> dict(out, gin, gpar).
    ``in_dtype(dt)``: the element type the differentiable operands are fed in (default: the mode's activation type).
    ``grad_values(dt, outs)``: gradient values per output (default: random); ``laid``: names of the operands that take layouts
    (default: every one of ins and ints); ``grads``: indices of the outputs whose gradient takes layouts."""

    def __init__(self, name, make, call, ref, tol, fwd_only=False, in_dtype=None, grad_values=None, laid=None, grads=None,
                 check_out=None, no_grad_outs=()):
        self.name, self.make, self.call, self.ref, self.tol = name, make, call, ref, tol
        self.fwd_only, self.in_dtype, self.grad_values, self.laid, self.grads = fwd_only, in_dtype, grad_values, laid, grads
        self.check_out, self.no_grad_outs = check_out, no_grad_outs


CASES = {}


def add(case):
    assert case.name not in CASES
    CASES[case.name] = case


M_, N_, K_, K2_ = 33, 24, 40, 16
ROWS = [(37, 40), (9, 1024)]
LN_ROWS = ROWS + [(5, 2048)]
SEQ = (9, 4)  # graph ops: two sequences
NODES = sum(SEQ)


# ---- contractions ---------------------------------------------------------------------------------------
def _linear_full(dt):
    g = gen(21)
    ins = dict(x=rnd(dt, M_, K_, g=g), x2=rnd(dt, M_, K2_, g=g), residual=rnd(dt, M_, N_, g=g))
    par = dict(W=rnd(dt, N_, K_, g=g), W2=rnd(dt, N_, K2_, g=g), b=torch.randn(N_, generator=g))
    return ins, par, {}


add(Case("linear", _linear_full,
         lambda ops, i, p, n: (ops.linear(i["x"], p["W"], p["b"], x2=i["x2"], W2=p["W2"], residual=i["residual"]),),
         lambda i, p, n, h: (F.linear(i["x"], p["W"], p["b"]) + F.linear(i["x2"], p["W2"]) + i["residual"],), gemm_tol))


def _linear_one(N):
    def make(dt):
        g = gen(22 + N)
        return dict(x=rnd(dt, M_, K_, g=g)), dict(W=rnd(dt, N, K_, g=g), b=torch.randn(N, generator=g)), {}
    return make


add(Case("linear_relu", _linear_one(N_), lambda ops, i, p, n: (ops.linear(i["x"], p["W"], p["b"], relu=True),),
         lambda i, p, n, h: (torch.relu(F.linear(i["x"], p["W"], p["b"])),), gemm_tol))
# N = 115: the logits' row stride is padded, and a gradient that is no operand takes ``_operand_rows``' padded copy
add(Case("linear_logits", _linear_one(115), lambda ops, i, p, n: (ops.linear(i["x"], p["W"], p["b"], out_f32=True),),
         lambda i, p, n, h: (F.linear(i["x"], p["W"], p["b"]),), gemm_tol))


def _multi_linear(dt):
    g = gen(23)
    return (dict(x0=rnd(dt, 20, K_, g=g), x1=rnd(dt, 13, K_, g=g)), dict(W=rnd(dt, N_, K_, g=g), b=torch.randn(N_, generator=g)), {})


add(Case("multi_linear", _multi_linear, lambda ops, i, p, n: (ops.multi_linear([i["x0"], i["x1"]], p["W"], p["b"]),),
         lambda i, p, n, h: (F.linear(torch.cat([i["x0"], i["x1"]]), p["W"], p["b"]),), gemm_tol))


# ---- layernorms -----------------------------------------------------------------------------------------
def ln_tol(rows, graph=False):
    # f32: test_rowln_fwd_bwd / test_graphln_lrelu_fwd_bwd; bf16: test_rowln_bf16_activations (the graph LayerNorm has no bf16
    # gradient test of its own: the same kernels' structure -- row passes, f32 partial sums per column -- so the same bounds)
    def tol(dt):
        if dt == F32:
            return dict(out=(1e-4, 1e-5), gin=(1e-3, 1e-4), gpar=(1e-3, 2e-3 if graph else 1e-3))
        return dict(out=OUT16, gin=(2e-2, 2e-2), gpar=(2e-2, 3e-2 * rows ** 0.5))
    return tol


def _ln_make(rows, cols):
    def make(dt):
        g = gen(rows * cols)
        return (dict(x=rnd(dt, rows, cols, g=g, scale=2.0, shift=0.3)),
                dict(w=torch.randn(cols, generator=g), b=torch.randn(cols, generator=g)), {})
    return make


def _graph_ln_ref(segs):
    def ref(i, p, n, h):
        parts = []
        for s, e in zip(segs[:-1], segs[1:]):
            x = i["x"][s:e]
            x = x - x.mean()
            parts.append(F.leaky_relu(x / (x.std(unbiased=False) + 1e-5) * p["w"] + p["b"], 0.2))
        return (torch.cat(parts),)
    return ref


for rows_, cols_ in LN_ROWS:
    for relu_ in (False, True):
        add(Case(f"row_layernorm[{rows_}x{cols_},relu={int(relu_)}]", _ln_make(rows_, cols_),
                 lambda ops, i, p, n, relu_=relu_: (ops.row_layernorm(i["x"], p["w"], p["b"], 1e-5, relu=relu_, p=0.0),),
                 lambda i, p, n, h, relu_=relu_, cols_=cols_: (
                     (torch.relu if relu_ else (lambda t: t))(F.layer_norm(i["x"], (cols_,), p["w"], p["b"], 1e-5)),),
                 ln_tol(rows_)))
    segs_ = [0, max(rows_ // 3, 2), rows_]
    add(Case(f"graph_layernorm_lrelu[{rows_}x{cols_}]", _ln_make(rows_, cols_),
             lambda ops, i, p, n, segs_=segs_: (ops.graph_layernorm_lrelu(
                 i["x"], p["w"], p["b"], torch.tensor(segs_, dtype=torch.int32, device=DEV), 1e-5, 0.2),),
             _graph_ln_ref(segs_), ln_tol(rows_, graph=True)))


# ---- graph ops ------------------------------------------------------------------------------------------
def _edges():
    from egopack_amd.data import radius_band_edges
    return torch.cat([radius_band_edges(torch.arange(SEQ[0]), 2), radius_band_edges(torch.arange(SEQ[1]), 1) + SEQ[0]], 1)


@functools.lru_cache(None)
def _graph():
    from egopack_amd.data import build_csr
    return build_csr(_edges(), NODES).to(DEV)


def _scatter_mean(src, index, n):
    out = src.new_zeros((n, src.shape[1])).index_add_(0, index, src)
    cnt = src.new_zeros(n).index_add_(0, index, src.new_ones(index.shape[0]))
    return out / cnt.clamp(min=1)[:, None]


def elem_tol(dt):
    # test_csr_mean_aggregate_fwd_bwd, test_pe_add (f32); test_graphln_csr_pe_bf16_activations (bf16: OUT16)
    return dict(out=(1e-5, 2e-5), gin=(1e-5, 2e-5), gpar=(1e-5, 2e-5)) if dt == F32 else dict(out=OUT16, gin=OUT16, gpar=OUT16)


def _freq(cols):
    return torch.logspace(0, 1, cols // 2, 1e-4)


for cols_ in (40, 1024):
    def _pe_make(dt, cols_=cols_):
        g = gen(9 + cols_)
        return dict(x=rnd(dt, NODES, cols_, g=g)), {}, dict(pos=torch.randint(-128, 128, (NODES,), generator=g))

    def _pe_ref(i, p, n, h, cols_=cols_):
        ang = n["pos"].double().view(-1, 1) * _freq(cols_).double().view(1, -1)
        return (i["x"] + torch.cat([torch.sin(ang), torch.cos(ang)], -1),)

    add(Case(f"pe_add[{cols_}]", _pe_make, lambda ops, i, p, n, cols_=cols_: (ops.pe_add(i["x"], n["pos"], _freq(cols_).to(DEV)),),
             _pe_ref, elem_tol))

    def _x_make(dt, cols_=cols_):
        return dict(x=rnd(dt, NODES, cols_, g=gen(30 + cols_))), {}, {}

    add(Case(f"csr_mean_aggregate[{cols_}]", _x_make, lambda ops, i, p, n: (ops.csr_mean_aggregate(i["x"], _graph()),),
             lambda i, p, n, h: (_scatter_mean(i["x"].index_select(0, _edges()[0]), _edges()[1], NODES),), elem_tol))

    def _live_make(dt, cols_=cols_):
        live = torch.tensor([1, 4, 9, 12])
        idx = torch.full((8,), -1, dtype=torch.int64)
        idx[:4] = live
        inv = torch.full((NODES,), -1, dtype=torch.int64)
        inv[live] = torch.arange(4)
        return dict(x=rnd(dt, NODES, cols_, g=gen(31 + cols_))), {}, dict(idx=idx, inv=inv)

    def _live_ref(i, p, n, h):
        return (torch.cat([i["x"][n["idx"][:4]], i["x"].new_zeros(4, i["x"].shape[1])]),)

    # test_live_rows_forward_gathers_and_backward_scatters_with_zero_rows: exact
    add(Case(f"live_rows[{cols_}]", _live_make, lambda ops, i, p, n: (ops.live_rows(i["x"], n["idx"], n["inv"]),), _live_ref,
             lambda dt: EXACT))

    def _gmax_make(dt, cols_=cols_):
        g = gen(32 + cols_)
        v = distinct(NODES + 7, cols_, g)
        nn = torch.stack([torch.randperm(7, generator=g)[:3] for _ in range(NODES)])
        return dict(f=v[:NODES].clone()), dict(bank=v[NODES:].clone()), dict(nn=nn)

    # test_gather_max_fwd_bwd (exact), test_gather_max_trainable_bank_gradient
    add(Case(f"gather_max[{cols_}]", _gmax_make, lambda ops, i, p, n: (ops.gather_max(i["f"], p["bank"], n["nn"]),),
             lambda i, p, n, h: (torch.cat([p["bank"][n["nn"]], i["f"][:, None]], 1).max(1).values,),
             lambda dt: dict(out=(1e-6, 1e-6) if dt == F32 else (1e-2, 1e-2), gin=(1e-6, 1e-6) if dt == F32 else (2e-2, 2e-2),
                            gpar=(1e-5, 1e-5))))

    def _smax_make(dt, cols_=cols_, k=1):
        g = gen(33 + cols_)
        return {f"x{j}": distinct(NODES, cols_, g) for j in range(k)}, {}, {}

    def _smax_ref(i, p, n, h):
        return tuple(torch.stack([x[:SEQ[0]].max(0).values, x[SEQ[0]:].max(0).values]) for x in i.values())

    _ptr = lambda: torch.tensor([0, SEQ[0], NODES], dtype=torch.int32, device=DEV)  # noqa: E731
    # test_segment_max_fwd_bwd, test_segment_max_of_several_inputs_in_one_launch: exact
    add(Case(f"segment_max[{cols_}]", _smax_make, lambda ops, i, p, n: (ops.segment_max(i["x0"], _ptr()),), _smax_ref,
             lambda dt: EXACT))
    add(Case(f"segment_max_multi[{cols_}]", functools.partial(_smax_make, k=2),
             lambda ops, i, p, n: tuple(ops.segment_max_multi([i["x0"], i["x1"]], _ptr())), _smax_ref, lambda dt: EXACT))


def _sage_make(dt):
    g = gen(40)
    par = dict(Wp=rnd(dt, K_, K_, g=g, scale=0.3), bp=torch.randn(K_, generator=g), Wl=rnd(dt, N_, K_, g=g, scale=0.3),
               bl=torch.randn(N_, generator=g), Wr=rnd(dt, N_, K_, g=g, scale=0.3))
    return dict(h=rnd(dt, NODES, K_, g=g)), par, {}


def _sage_call(ops, i, p, n):
    NS = types.SimpleNamespace
    conv = NS(lin=NS(weight=p["Wp"], bias=p["bp"]), lin_l=NS(weight=p["Wl"], bias=p["bl"]), lin_r=NS(weight=p["Wr"]))
    return (ops.sage_mean_layer(i["h"], conv, _graph()),)


def _sage_ref(i, p, n, h):
    """bf16: the layer stores its projected features, its aggregate and its output (and their gradients) as bf16 between its
    launches -- the reference rounds at those three points, as the layer's existing bf16 test does (oracle/storage.py through
    tests/test_gpu_blockwise.py::test_sage_layer_graph_layernorm_block)."""
    from oracle import storage as S
    ei = _edges()
    with S.bf16_storage(n.get("_dt") == BF):
        xp = S.act(torch.relu(F.linear(i["h"], p["Wp"], p["bp"])))
        agg = S.act(_scatter_mean(xp.index_select(0, ei[0]), ei[1], NODES))
        return (S.act(F.linear(agg, p["Wl"], p["bl"]) + F.linear(i["h"], p["Wr"])),)


BLOCK_TOL = ("rel", 5e-3)  # tests/test_gpu_blockwise.py BLOCK_TOL: |got - want| / |want| in the Frobenius norm, per tensor
add(Case("sage_mean_layer", _sage_make, _sage_call, _sage_ref,
         lambda dt: GEMM_F32 if dt == F32 else dict(out=BLOCK_TOL, gin=BLOCK_TOL, gpar=BLOCK_TOL)))


# ---- losses and fused heads -----------------------------------------------------------------------------
LOSS_TOL = dict(out=(1e-5, 1e-5), gin=(1e-4, 1e-6), gpar=(0, 0))  # test_cross_entropy_heads_ignore_index, the focal kernel test
NL = 37


def _ce_make(heads):
    def make(dt):
        g = gen(51)
        ins = {f"l{h}": torch.randn(NL, C, generator=g) * 3 for h, C in enumerate(heads)}
        y = torch.stack([torch.randint(0, C, (NL,), generator=g) for C in heads], 1)
        y[::3] = -1
        return ins, {}, dict(y=y if len(heads) > 1 else y[:, 0].clone())
    return make


def _ce_ref(i, p, n, h):
    y = n["y"] if n["y"].dim() == 2 else n["y"][:, None]
    return (sum(F.cross_entropy(l, y[:, k], ignore_index=-1, reduction="none", label_smoothing=0.1)
                for k, l in enumerate(i.values())),)


add(Case("cross_entropy", _ce_make((115,)), lambda ops, i, p, n: (ops.cross_entropy(i["l0"], n["y"], 0.1),), _ce_ref,
         lambda dt: LOSS_TOL, in_dtype=lambda dt: F32))
add(Case("cross_entropy_heads", _ce_make((115, 24)), lambda ops, i, p, n: (ops.cross_entropy((i["l0"], i["l1"]), n["y"], 0.1),),
         _ce_ref, lambda dt: LOSS_TOL, in_dtype=lambda dt: F32))


def _bce_make(dt):
    g = gen(53)
    return dict(x=torch.randn(NL, generator=g) * 4), {}, dict(y=torch.randint(0, 2, (NL,), generator=g))


# test_bce_with_logits
add(Case("bce_with_logits", _bce_make, lambda ops, i, p, n: (ops.bce_with_logits(i["x"], n["y"]),),
         lambda i, p, n, h: (F.binary_cross_entropy_with_logits(i["x"], n["y"].double(), reduction="none"),),
         lambda dt: dict(out=(1e-5, 1e-6), gin=(1e-5, 1e-6), gpar=(0, 0)), in_dtype=lambda dt: F32))


def _onehot_make(dt):
    g = gen(55)
    return dict(x=torch.randn(NL, 2, generator=g) * 3), {}, dict(y=torch.randint(0, 2, (NL,), generator=g))


def _focal_ref(i, p, n, h):
    t = F.one_hot(n["y"], 2).double()
    pr = torch.sigmoid(i["x"])
    ce = F.binary_cross_entropy_with_logits(i["x"], t, reduction="none")
    return ((0.5 * t + 0.5 * (1 - t)) * ce * (1 - (pr * t + (1 - pr) * (1 - t))) ** 2.0,)


# test_onehot_sigmoid_focal_kernel_vs_autograd
_OH_TOL = dict(out=(1e-5, 1e-6), gin=(1e-4, 1e-6), gpar=(0, 0))
add(Case("onehot_bce_with_logits", _onehot_make, lambda ops, i, p, n: (ops.onehot_bce_with_logits(i["x"], n["y"]),),
         lambda i, p, n, h: (F.binary_cross_entropy_with_logits(i["x"], F.one_hot(n["y"], 2).double(), reduction="none"),),
         lambda dt: _OH_TOL, in_dtype=lambda dt: F32))
add(Case("onehot_sigmoid_focal_loss", _onehot_make, lambda ops, i, p, n: (ops.onehot_sigmoid_focal_loss(i["x"], n["y"], 0.5, 2.0),),
         _focal_ref, lambda dt: _OH_TOL, in_dtype=lambda dt: F32))


def head_tol(scale_of):
    """test_one_logit_head_with_bce_in_one_row_pass / test_two_logit_head_with_cross_entropy_in_one_launch: gradients within a
    fraction of their largest element (``scale_of(ref)`` -> (input scale, weight scale, bias scale))."""
    def tol(dt, ref=None):
        f32 = dt == F32
        lt = (1e-4, 1e-4) if f32 else (1e-2, 2e-2)
        if ref is None:
            return dict(out=lt)
        gs, ws, bs = scale_of(ref)
        return dict(out=lt, gin=(0, (1e-5 if f32 else 1.5e-2) * gs),
                    gpar=dict(W=(0, (2e-5 if f32 else 1.5e-2) * ws), b=(0, (2e-5 if f32 else 1e-2) * max(1.0, bs * 100))))
    return tol


def _head_scales(ref):
    _, gin, gpar = ref
    return float(gin["f"].abs().max()), float(gpar["W"].abs().max()), float(gpar["b"].abs().max())


for rows_, cols_ in ROWS:
    seed_ = 0.7 / rows_

    def _head_make(n_out):
        def make(dt, rows_=rows_, cols_=cols_):
            g = gen(rows_ + cols_ + n_out)
            y = torch.randint(0, 2, (rows_,), generator=g)
            if n_out == 2:
                y[::5] = -1
            return (dict(f=rnd(dt, rows_, cols_, g=g)),
                    dict(W=rnd(dt, n_out, cols_, g=g, scale=0.05), b=torch.randn(n_out, generator=g)), dict(y=y))
        return make

    def _l1_call(ops, i, p, n, seed_=seed_):
        with ops.loss_seed(seed_):
            return tuple(ops.linear1_bce(i["f"], p["W"], p["b"], n["y"]))

    def _l2_call(ops, i, p, n, seed_=seed_):
        with ops.loss_seed(seed_):
            return tuple(ops.linear2_ce(i["f"], p["W"], p["b"], n["y"], 0.1))

    def _l1_ref(i, p, n, h):
        z = (i["f"] @ p["W"].t()).squeeze(1) + p["b"]
        return F.binary_cross_entropy_with_logits(z, n["y"].double(), reduction="none"), z

    def _l2_ref(i, p, n, h):
        z = i["f"] @ p["W"].t() + p["b"]
        return F.cross_entropy(z, n["y"], reduction="none", ignore_index=-1, label_smoothing=0.1), z

    # the gradients are computed in forward from the ANNOUNCED seed: the gradient fed to backward holds that constant
    _seed_grads = lambda dt, outs, seed_=seed_: [torch.full(outs[0].shape, seed_), None]  # noqa: E731
    add(Case(f"linear1_bce[{rows_}x{cols_}]", _head_make(1), _l1_call, _l1_ref, head_tol(_head_scales), grad_values=_seed_grads,
             grads=(0,), no_grad_outs=(1,)))
    add(Case(f"linear2_ce[{rows_}x{cols_}]", _head_make(2), _l2_call, _l2_ref, head_tol(_head_scales), grad_values=_seed_grads,
             grads=(0,), no_grad_outs=(1,)))


# ---- element-wise and casts -----------------------------------------------------------------------------
for rows_, cols_ in ROWS:
    def _ew_make(dt, rows_=rows_, cols_=cols_):
        x = rnd(dt, rows_, cols_, g=gen(60 + cols_))
        return dict(x=torch.where(x.abs() < 0.125, torch.full_like(x, 0.5), x)), {}, {}  # (no zeros: y != 0 is the keep mask)

    def _drop_call(ops, i, p, n):
        ops.manual_seed(77)
        return (ops.dropout(i["x"], 0.25, True),)

    # test_dropout_op: kept elements are x / (1 - p); the keep mask is the device's (bit-checked in test_gpu_dropout_masks.py)
    add(Case(f"dropout[{rows_}x{cols_}]", _ew_make, _drop_call, lambda i, p, n, h: (i["x"] * (h[0] != 0).double() / 0.75,),
             lambda dt: dict(out=(1e-6, 1e-6), gin=(1e-6, 1e-6)) if dt == F32 else dict(out=OUT16, gin=OUT16)))
    add(Case(f"relu[{rows_}x{cols_}]", _ew_make, lambda ops, i, p, n: (ops.relu(i["x"]),), lambda i, p, n, h: (torch.relu(i["x"]),),
             lambda dt: EXACT))

    def _cast_in(dt):
        return F32 if dt == BF else BF

    def _cast_ref(i, p, n, h):
        return (i["x"],)  # (values representable in bf16: both directions are exact)

    add(Case(f"to_act[{rows_}x{cols_}]", lambda dt, rows_=rows_, cols_=cols_: (dict(x=rnd(BF, rows_, cols_, g=gen(61))), {}, {}),
             lambda ops, i, p, n: (ops.to_act(i["x"]),), _cast_ref, lambda dt: EXACT, in_dtype=_cast_in,
             grad_values=lambda dt, outs: [r16(torch.randn(outs[0].shape, generator=gen(63)))]))
    add(Case(f"cast_raw[{rows_}x{cols_}]", lambda dt, rows_=rows_, cols_=cols_: (dict(x=rnd(BF, rows_, cols_, g=gen(62))), {}, {}),
             lambda ops, i, p, n: (ops.cast_raw(i["x"], ops.act_dtype()),), _cast_ref, lambda dt: EXACT, in_dtype=_cast_in,
             fwd_only=True))


def _sum_make(dt):
    g = gen(54)
    return {f"t{j}": torch.randn(NL, 40, generator=g) for j in range(3)}, {}, {}


for scale_ in (1.0, 0.25):  # test_weighted_mean_sum_and_sum_tensors
    add(Case(f"sum_tensors[{scale_}]", _sum_make, lambda ops, i, p, n, scale_=scale_: (ops.sum_tensors(list(i.values()), scale_),),
             lambda i, p, n, h, scale_=scale_: (torch.stack(list(i.values())).sum(0) * scale_,),
             lambda dt: dict(out=(1e-6, 1e-6), gin=(1e-6, 1e-6)), in_dtype=lambda dt: F32))


def _wms_make(dt):
    g = gen(56)
    return dict(a=torch.randn(NL, generator=g), b=torch.randn(13, generator=g)), {}, {}


add(Case("weighted_mean_sum", _wms_make, lambda ops, i, p, n: (ops.weighted_mean_sum([i["a"], i["b"]], [0.5, 2.0]),),
         lambda i, p, n, h: (0.5 * i["a"].mean() + 2.0 * i["b"].mean(),),
         lambda dt: dict(out=(1e-5, 1e-6), gin=(1.3e-6, 1e-5)), in_dtype=lambda dt: F32, grads=()))  # (gin: assert_close defaults)

add(Case("split_rows", lambda dt: (dict(x=rnd(dt, NODES, 40, g=gen(57))), {}, {}),
         lambda ops, i, p, n: tuple(ops.split_rows(i["x"], SEQ)), lambda i, p, n, h: (i["x"][:SEQ[0]], i["x"][SEQ[0]:]),
         lambda dt: EXACT))


# ---- forward-only helpers -------------------------------------------------------------------------------
GENERIC = dict(out=(1e-4, 1e-5))  # tests/test_gpu_bounds.py GENERIC: every non-GEMM kernel against its f64 reference
for rows_, cols_ in ROWS:
    _mk = lambda dt, rows_=rows_, cols_=cols_: (dict(x=rnd(dt, rows_, cols_, g=gen(70 + cols_), scale=2.0)), {}, {})  # noqa: E731
    add(Case(f"row_inv_norm[{rows_}x{cols_}]", _mk, lambda ops, i, p, n: (ops.row_inv_norm(i["x"]),),
             lambda i, p, n, h: (i["x"].pow(2).sum(1).rsqrt(),), lambda dt: GENERIC, fwd_only=True))
    add(Case(f"row_sq_norm[{rows_}x{cols_}]", _mk, lambda ops, i, p, n: (ops.row_sq_norm(i["x"]),),
             lambda i, p, n, h: (i["x"].pow(2).sum(1),), lambda dt: GENERIC, fwd_only=True))


def _np_make(dt):
    g = gen(71)
    return dict(f=rnd(dt, NODES, 40, g=g), bank=torch.randn(7, 40, generator=g)), {}, {}


def _np_check(outs, ins):
    """test_cosine_topk_indices: exact wherever the ranking gap exceeds f32 summation noise; the selected distances are the k
    smallest up to that noise everywhere."""
    nn, k = outs[0].cpu(), 3
    f, b = ins["f"].double(), ins["bank"].double()
    dist = 1 - (f / f.norm(dim=1, keepdim=True)) @ (b / b.norm(dim=1, keepdim=True)).t()
    srt, order = dist.sort(dim=-1)
    safe = (srt[:, 1:k + 1] - srt[:, :k]).min(dim=1).values > 1e-5
    assert safe.float().mean() > 0.9
    assert torch.equal(nn[safe], order[:, :k][safe])
    torch.testing.assert_close(torch.gather(dist, 1, nn), srt[:, :k], rtol=0, atol=2e-5)


add(Case("nearest_prototypes", _np_make, lambda ops, i, p, n: (ops.nearest_prototypes(i["f"], i["bank"], 3),), None, None,
         fwd_only=True, check_out=_np_check, in_dtype=lambda dt: {"f": dt, "bank": F32}))


def _scat_make(dt):
    g = gen(72)
    x = torch.randint(-8, 9, (NODES, 40), generator=g).float() / 4  # (sums exact in f32 in any order)
    label = torch.randint(-1, 5, (NODES,), generator=g)
    label[:3] = 2
    return dict(x=x), {}, dict(label=label)


def _scat_call(ops, i, p, n):
    bank = torch.zeros(5, 40, dtype=torch.float64, device=DEV)
    count = torch.zeros(5, dtype=torch.int64, device=DEV)
    ops.scatter_add_rows_f64(i["x"], n["label"], bank, count)
    return bank, count


def _scat_ref(i, p, n, h):
    keep = n["label"] >= 0
    return (torch.zeros(5, 40, dtype=torch.float64).index_add_(0, n["label"][keep], i["x"][keep]),
            torch.bincount(n["label"][keep], minlength=5))


# test_scatter_add_rows_f64: bit-exact
add(Case("scatter_add_rows_f64", _scat_make, _scat_call, _scat_ref, lambda dt: dict(out=(0, 0)), fwd_only=True))


def _expand_make(dt):
    inv = torch.full((NODES,), -1, dtype=torch.int64)
    inv[torch.tensor([1, 4, 9, 12])] = torch.arange(4)
    return dict(v=rnd(dt, 8, g=gen(73))), {}, dict(inv=inv)


def _expand_ref(i, p, n, h):
    out = i["v"].new_zeros(NODES)
    out[n["inv"] >= 0] = i["v"][n["inv"][n["inv"] >= 0]]
    return (out,)


add(Case("expand_rows", _expand_make, lambda ops, i, p, n: (ops.expand_rows(i["v"], n["inv"]),), _expand_ref,
         lambda dt: dict(out=(0, 0)), fwd_only=True))


# ---------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------
def _mode(dt):
    return "f32" if dt == F32 else "bf16"


def _in_dtype(case, dt, name):
    d = case.in_dtype(dt) if case.in_dtype is not None else dt
    return d[name] if isinstance(d, dict) else d


@functools.lru_cache(None)
def _made(name, dt):
    return CASES[name].make(dt)


_grad_base, _ref_cache = {}, {}


def run(ops, case, dt, operand, tag, use_view):
    """One evaluation of ``case``; ``operand`` (an input / integer operand name, or ``grad<i>``) is a view in layout ``tag`` when
    ``use_view``, and its ``.contiguous()`` copy otherwise.  Returns (outputs, input gradients, parameter gradients, the packed
    gradient values fed in, [(backing buffer, its bits before)])."""
    ins_v, par_v, int_v = _made(case.name, dt)
    watched = []

    def place(t, name):
        if name != operand:
            return t
        t = lay_values(t, tag)
        if not use_view:
            return t.contiguous()
        view, big = lay(t, tag)
        watched.append((big, bits(big).clone()))
        return view

    ins = {k: place(v.to(DEV).to(_in_dtype(case, dt, k)), k).detach().requires_grad_(not case.fwd_only) for k, v in ins_v.items()}
    ints = {k: place(v.to(DEV), k) for k, v in int_v.items()}
    par = {k: v.to(DEV).clone().requires_grad_(not case.fwd_only) for k, v in par_v.items()}
    fed = None
    with ops.compute_mode(_mode(dt)):
        if case.fwd_only:
            with torch.no_grad():
                outs = case.call(ops, ins, par, ints)
        else:
            outs = case.call(ops, ins, par, ints)
            key = (case.name, dt)
            if key not in _grad_base:
                g = gen(1000 + len(_grad_base))
                if case.grad_values is not None:
                    _grad_base[key] = case.grad_values(dt, outs)
                else:
                    _grad_base[key] = [(r16 if o.dtype == BF else (lambda t: t))(torch.randn(o.shape, generator=g)) for o in outs]
            fed, gs, live = [], [], []
            for j, (o, gv) in enumerate(zip(outs, _grad_base[key])):
                if j in case.no_grad_outs:
                    fed.append(None)
                    continue
                gv = lay_values(gv, tag) if operand == f"grad{j}" else gv
                fed.append(gv)
                gs.append(place(gv.to(DEV).to(o.dtype), f"grad{j}"))
                live.append(o)
            torch.autograd.backward(live, gs)
            ops.join_wgrad()
    torch.cuda.synchronize()
    gin = {k: v.grad for k, v in ins.items()} if not case.fwd_only else {}
    gpar = {k: v.grad for k, v in par.items()} if not case.fwd_only else {}
    return outs, gin, gpar, fed, watched


def reference(case, dt, operand, tag, fed, hint):
    """float64 reference on the packed values (cached per gradient: the broadcast layouts feed other values)."""
    gkey = tag if (operand.startswith("grad") and tag.startswith("bcast")) else ""
    key = (case.name, dt, operand if gkey else "", gkey)
    if key in _ref_cache:
        return _ref_cache[key]
    ins_v, par_v, int_v = _made(case.name, dt)
    ins = {k: v.double().requires_grad_(not case.fwd_only) for k, v in ins_v.items()}
    par = {k: v.double().requires_grad_(not case.fwd_only) for k, v in par_v.items()}
    outs = case.ref(ins, par, {**int_v, "_dt": dt}, hint)
    if not case.fwd_only:
        live = [(o, g.double()) for o, g in zip(outs, fed) if g is not None]
        torch.autograd.backward([o for o, _ in live], [g for _, g in live])
    res = ([o.detach() for o in outs], {k: v.grad for k, v in ins.items()}, {k: v.grad for k, v in par.items()})
    _ref_cache[key] = res
    return res


def close(got, want, tol, what):
    assert got is not None, f"{what}: no gradient"
    if not got.dtype.is_floating_point:
        assert torch.equal(got.cpu(), want), what
        return
    assert not bool(torch.isnan(got).any()), f"{what}: NaN"
    if tol[0] == "rel":
        rel = float((got.detach().double().cpu() - want.double()).norm() / want.double().norm().clamp(min=1e-30))
        assert rel < tol[1], f"{what}: relative distance {rel:.3e} (up to {tol[1]:.0e} allowed)"
        return
    torch.testing.assert_close(got.detach().double().cpu(), want.double(), rtol=tol[0], atol=tol[1], msg=lambda s: f"{what}: {s}")


def same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b)), f"{what}: not the bits of the packed run"


def _operands():
    """(case, operand, tag) of the whole suite."""
    out = []
    for name, case in CASES.items():
        ins_v, _, int_v = case.make(F32)
        named = list(ins_v.items()) + list(int_v.items())
        for k, v in named:
            if case.laid is not None and k not in case.laid:
                continue
            out += [(name, k, t) for t in (FWD_TAGS if v.dim() == 2 else VEC_FWD_TAGS)]
        if case.fwd_only:
            continue
        n_out, dims = _OUTS[name]
        for j in (range(n_out) if case.grads is None else case.grads):
            out += [(name, f"grad{j}", t) for t in (GRAD_TAGS if dims[j] == 2 else VEC_GRAD_TAGS)]
        if case.grads == ():
            out.append((name, "grad0", "packed"))
    return out


def _out_dims():
    """Number and rank of every case's outputs, from the float64 reference (the dropout mask: all kept)."""
    res = {}
    for name, case in CASES.items():
        if case.fwd_only:
            continue
        ins_v, par_v, int_v = case.make(F32)
        with torch.no_grad():
            outs = case.ref({k: v.double() for k, v in ins_v.items()}, {k: v.double() for k, v in par_v.items()}, int_v,
                            [v for v in ins_v.values()])
        res[name] = (len(outs), [o.dim() for o in outs])
    return res


_OUTS = _out_dims()
_ALL = _operands()


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,operand,tag", _ALL, ids=[f"{n}-{o}-{t}" for n, o, t in _ALL])
def test_layout(ops, name, operand, tag, dt):
    case = CASES[name]
    outs, gin, gpar, fed, watched = run(ops, case, dt, operand, tag, use_view=True)
    pouts, pgin, pgpar, _, _ = run(ops, case, dt, operand, tag, use_view=False)
    # 4. the backing buffer keeps its bits (NaN outside the view, the values inside)
    for big, before in watched:
        assert torch.equal(bits(big), before), f"{name}: the backing buffer of {operand} was written"
    # 1. + 3. the float64 reference on the packed values
    ins_v = _made(name, dt)[0]
    if case.check_out is not None:
        case.check_out(outs, ins_v)
    else:
        hint = [o.detach().cpu() for o in pouts]
        r_out, r_gin, r_gpar = ref = reference(case, dt, operand, tag, fed, hint)
        tol = case.tol(dt) if case.fwd_only or "gin" in case.tol(dt) else case.tol(dt, ref)
        for j, (o, r) in enumerate(zip(outs, r_out)):
            close(o, r, tol["out"], f"{name} output {j}")
        for k in gin:
            close(gin[k], r_gin[k], tol["gin"], f"{name} d{k}")
        for k in gpar:
            close(gpar[k], r_gpar[k], tol["gpar"][k] if isinstance(tol["gpar"], dict) else tol["gpar"], f"{name} d{k}")
    # 2. the bits of the same op on .contiguous() copies (no case needs the other-kernel-variant exemption: a view that is no
    # aligned operand is packed before its launch, so both runs issue the same kernels)
    for j, (a, b) in enumerate(zip(outs, pouts)):
        same(a, b, f"{name} output {j}")
    for k in gin:
        same(gin[k], pgin[k], f"{name} d{k}")
    for k in gpar:
        same(gpar[k], pgpar[k], f"{name} d{k}")


# ---------------------------------------------------------------------------------------------------------
# the same layouts from the downstream expressions that produce them (tests/test_layouts_cpu.py pins the table)
# ---------------------------------------------------------------------------------------------------------
DOWNSTREAM = {
    "cat_first": lambda y, o: torch.cat([y, o], 1),       # strides (cols + 5, 1)
    "cat_second": lambda y, o: torch.cat([o, y], 1),      # the same, storage offset 5
    "sum_rows": lambda y, o: y.sum(0),                    # strides (0, 1)
    "sum_all": lambda y, o: y.sum(),                      # strides (0, 0)
    "transposed": lambda y, o: y.t() * o[:, 0],           # strides (1, rows)
}


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("how", list(DOWNSTREAM))
@pytest.mark.parametrize("name", ["linear", "multi_linear", "row_layernorm[37x40,relu=1]", "graph_layernorm_lrelu[37x40]",
                                  "sage_mean_layer"])
def test_downstream_expression(ops, name, how, dt):
    """End to end: the op's output goes through a real torch expression; the gradients must be those of the float64 reference of
    the op followed by the same expression."""
    case = CASES[name]
    ins_v, par_v, int_v = _made(name, dt)
    ins = {k: v.to(DEV).to(_in_dtype(case, dt, k)).clone().requires_grad_(True) for k, v in ins_v.items()}
    par = {k: v.to(DEV).clone().requires_grad_(True) for k, v in par_v.items()}
    with ops.compute_mode(_mode(dt)):
        (y,) = case.call(ops, ins, par, {k: v.to(DEV) for k, v in int_v.items()})
        g = gen(99)
        other = rnd(dt, y.shape[0], 5, g=g)
        z = DOWNSTREAM[how](y, other.to(DEV).to(y.dtype))
        w = rnd(dt, *z.shape, g=g) if z.dim() else torch.tensor(1.0)
        z.backward(w.to(DEV).to(z.dtype))
        ops.join_wgrad()
    torch.cuda.synchronize()
    rin = {k: v.double().requires_grad_(True) for k, v in ins_v.items()}
    rpar = {k: v.double().requires_grad_(True) for k, v in par_v.items()}
    (ry,) = case.ref(rin, rpar, {**int_v, "_dt": dt}, None)
    DOWNSTREAM[how](ry, other.double()).backward(w.double())
    tol = case.tol(dt)
    # (sum over rows: the gradient of a parameter sums up to 37 equal terms; the bounds are those of the op's own test)
    for k in ins:
        close(ins[k].grad, rin[k].grad, tol["gin"], f"{name} via {how}: d{k}")
    for k in par:
        close(par[k].grad, rpar[k].grad, tol["gpar"], f"{name} via {how}: d{k}")
