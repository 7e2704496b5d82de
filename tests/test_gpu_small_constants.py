"""The small constants of the kernels in the regimes where they carry weight: the eps of the row LayerNorm (on the variance) and of
the graph LayerNorm (on the std; its backward rebuilds sigma = 1 / r - eps from the stored r), the eps and the betas of the Adam
family, the 1e-6 of the gradient clip.  Every other GPU test runs them at std ~ 1 with eps = 1e-5, resp. N(0, 1) gradients with
eps = 1e-8 and betas (0.9, 0.999), where a misplaced eps moves the result by less than those tests' tolerances.  Here: eps = 0.5
at std 1, eps = 1e-5 at std 1e-4 and 3e-6, segments of different scale inside one launch, one exactly constant segment; gradients
over 11 decades down to 1e-12 with exact zeros, betas (0.8, 0.95) with eps = 1e-3; gradient norms at, below and above the clip's
constant.  References, mutants, inputs, cases and tolerances: tests/small_constants_common.py; that the mutants are 100 x the
tolerance away (and hidden in the older regime): tests/test_small_constants_cpu.py.

Entry points reached (every one of include/*.h that takes the constant): egk_rowln_fwd / _bwd, egk_rowln_group_fwd / _bwd,
egk_graphln_fwd / _bwd, egk_graphln_fwd_apply / _bwd_apply (partials of a contraction's epilogue), egk_graphln_stats / _bwd_stats /
_bwd_finish (exchanged statistics), egk_adam_hyper, egk_adam_step / _bump / _gated, egk_optim_step, egk_optim_step_groups,
egk_optim_step_ema, egk_grad_norm_finalize.

Comparison: per tensor max |got - ref| <= tol * max |ref| against the fp64 reference of the rounded inputs (graph LayerNorm: y and
dx per SEGMENT, the segments of one launch differ by 5 decades); a tensor stored in bf16 gets one bf16 rounding step (2^-8 |ref|
per element) on top; exp_avg / exp_avg_sq per element, relative, exact zeros stay zero.  tol = 4 x the worst figure measured on an
MI355X over the whole family (f32 cases), rounded up to one digit, under the caps (a) the older test of the same kernel and (b)
1 / 100 of the smallest mutant gap.  Every test prints its figures ("err" = max |got - ref| / max |ref|, "ratio" = against its bound).

  family               tensor       f32 arithmetic (CPU)   measured worst (MI355X)   tol      cap (a)   cap (b)
  row LayerNorm        y            1.2e-7                 1.14e-7                   5e-7     1e-4      1.3e-3
  (+ grouped)          dx           1.6e-7                 1.45e-7                   6e-7     1e-3      1.5e-3
                       dw           1.5e-7                 2.12e-7                   9e-7     1e-3      1.6e-3
                       db           1.3e-7                 1.57e-7                   7e-7     1e-3      -
  graph LayerNorm      y            2.0e-7                 1.05e-7                   5e-7     1e-4      1.0e-3
  (all three routes)   dx           2.0e-7                 1.06e-7                   5e-7     1e-3      4.7e-5 (third term over sigma + eps)
                       dw           1.9e-7                 2.34e-7                   1e-6     1e-3      8.9e-4
                       db           1.3e-7                 1.35e-7                   6e-7     1e-3      -
  Adam / AdamW         p            2.4e-7                 2.51e-7                   1e-6     1e-5      5.3e-6 (betas), 2.6e-5 (eps)
  (launches, classes,  exp_avg      2.0e-7                 3.76e-7                   2e-6     -         every element moves by > 0.1 (betas)
   clip)               exp_avg_sq   3.6e-7                 3.64e-7 (AdamW rule)      2e-6     -         the same
                                                           1.31e-5 (Adam rule)       6e-5     -         the same
                       ema          1.1e-7                 1.12e-7                   5e-7     -         -
  clip                 coefficient  6e-8                   2.72e-8                   2e-7     -         1e-5
bf16 cases: the dw / db figures are below the f32 ones; y and dx reach 0.99 of their bound, which is the rounding step itself.
p is also held to the older test's elementwise rtol 1e-5 / atol 1e-6 (tol * max |ref| alone is looser than its atol where |p| is small).
exp_avg_sq: EGK_OPT_ADAM (egk_adam_step*, egk_optim_step rule 0) forms 1 - beta2 as the f32 difference 1.f - fl32(beta2), which for
beta2 = 0.999 is 1.3e-5 away from 0.001 (include/egopack_optim.h states it; torch rounds 1 - beta2 once from double).  Its bound
is 6e-5; EGK_OPT_ADAMW rounds once and is held to 2e-6."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests import small_constants_common as S
from tests.small_constants_common import BF, F64

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops as _ops
    return _ops


def _ids(cases):
    return [n for n, _ in cases]


def _tag(dt):
    return "bf16" if dt == BF else "f32"


def _held(what, figures):
    """Print every (tensor, err, ratio) of a test, then assert each ratio <= 1."""
    print(f"{what}: " + ", ".join(f"{k} err {e:.2e} ratio {r:.3f}" for k, e, r in figures))
    bad = [(k, e, r) for k, e, r in figures if not r <= 1.0]
    assert not bad, f"{what}: outside the bound: {bad}"


def _ln_figures(got, ref, tols, dt, segs=None, names=("y", "dx", "dw", "db")):
    steps, out = S.out_steps(dt), []
    for k in names:
        if segs is not None and k in ("y", "dx"):
            for s, e in zip(segs[:-1], segs[1:]):
                out.append((f"{k}[{s}:{e}]", S.rel_err(got[k][s:e], ref[k][s:e]), S.bound_ratio(got[k][s:e], ref[k][s:e], tols[k], steps[k])))
        else:
            out.append((k, S.rel_err(got[k], ref[k]), S.bound_ratio(got[k], ref[k], tols[k], steps[k])))
    return out


def _leaves(x, w, b, dt):
    return (x.to(dt).to(DEV).requires_grad_(True), w.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True))


# ---- 1. row LayerNorm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", S.rowln_cases(), ids=_ids(S.rowln_cases()))
def test_row_layernorm_against_fp64(ops, name, case):
    """egk_rowln_fwd / egk_rowln_bwd: y, dx, dw, db.  The dropout case applies the kernel's own keep mask to the reference."""
    x, w, b, noise, eps = S.rowln_inputs(case)
    dt, p = case["dt"], case["p"]
    xd, wd, bd = _leaves(x, w, b, dt)
    mask = None
    if p:
        ops.manual_seed(1234)
        y = ops.row_layernorm(xd, wd, bd, eps, relu=case["relu"], p=p, training=True)
        mask = ops.last_rowln_mask(y).cpu()
        assert abs(float(mask.float().mean()) - (1 - p)) < 0.02
    else:
        y = ops.row_layernorm(xd, wd, bd, eps, relu=case["relu"])
    ref = S.rowln_ref(x, w, b, eps, case["relu"], mask, p, noise=noise, cot_dtype=dt)
    y.backward(ref["cot"].to(dt).to(DEV))
    got = dict(y=y.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu())
    _held(f"row LayerNorm {name}", _ln_figures(got, ref, S.TOL_ROWLN, dt))


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=_tag)
@pytest.mark.parametrize("regime", ["eps0.5", "mixed"])
def test_grouped_row_layernorm_against_fp64(ops, regime, dt):
    """egk_rowln_group_fwd / egk_rowln_group_bwd (+ReLU): three row ranges with their own (w, b) in one launch; "mixed": eps = 1e-5
    with the ranges at std 1e-4, 3e-6 and 1."""
    from egopack_amd import _lib
    lib = _lib.load()
    cols, rows = S.ROWLN_GROUP["cols"], S.ROWLN_GROUP["rows"]
    G, n = len(rows), sum(rows)
    ptr = [0]
    for r in rows:
        ptr.append(ptr[-1] + r)
    scales, eps = (S.row_scales(ptr, (1e-4, 3e-6, 1.0)), 1e-5) if regime == "mixed" else (1.0, 0.5)
    x, _, _, noise = S.ln_data(256, n, cols, scales, dt)
    g = S.gen(257)
    ws_ = [S.rounded(torch.randn(cols, generator=g, dtype=F64), torch.float32) for _ in rows]
    bs_ = [S.rounded(torch.randn(cols, generator=g, dtype=F64), torch.float32) for _ in rows]
    refs = [S.rowln_ref(x[a:e], ws_[k], bs_[k], eps, True, noise=noise[a:e], cot_dtype=dt) for k, (a, e) in enumerate(zip(ptr[:-1], ptr[1:]))]
    xd, dy = x.to(dt).to(DEV), torch.cat([r["cot"] for r in refs]).to(dt).to(DEV)
    wdev, bdev = [t.float().to(DEV) for t in ws_], [t.float().to(DEV) for t in bs_]
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    mean, rstd = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    row_ptr = (C.c_int32 * (G + 1))(*ptr)
    s = ops._stream()
    assert lib.egk_rowln_group_fwd(s, ops._p(xd), ops._ptr_array(wdev), ops._ptr_array(bdev), row_ptr, G, ops._p(y), ops._p(mean),
                                   ops._p(rstd), cols, eps, 1, ops._dt(xd)) == 0, _lib.last_error()
    grid = lib.egk_rowln_bwd_ws_rows(max(rows))
    ws = torch.zeros(G * grid * 2 * cols, device=DEV)
    assert lib.egk_rowln_group_bwd(s, ops._p(dy), ops._p(xd), ops._ptr_array(wdev), ops._ptr_array(bdev), row_ptr, G, ops._p(mean),
                                   ops._p(rstd), ops._p(dx), ops._p(ws), cols, 1, ops._dt(xd)) == 0, _lib.last_error()
    figures = []
    for k, (a, e) in enumerate(zip(ptr[:-1], ptr[1:])):
        dw, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        part = ws[k * grid * 2 * cols:]
        assert lib.egk_ln_bwd_reduce(s, ops._p(part), ops._p(dw), ops._p(db), max(rows), cols, 0) == 0, _lib.last_error()
        got = dict(y=y[a:e].cpu(), dx=dx[a:e].cpu(), dw=dw.cpu(), db=db.cpu())
        figures += [(f"range{k} {t}", er, ra) for t, er, ra in _ln_figures(got, refs[k], S.TOL_ROWLN, dt)]
    _held(f"grouped row LayerNorm {regime} {_tag(dt)}", figures)


# ---- 2. graph LayerNorm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", S.graphln_cases(), ids=_ids(S.graphln_cases()))
def test_graph_layernorm_against_fp64(ops, name, case):
    """egk_graphln_fwd / egk_graphln_bwd through ops.graph_layernorm_lrelu."""
    x, w, b, noise, eps = S.graphln_inputs(case)
    dt, segs = case["dt"], case["segs"]
    ref = S.graphln_ref(x, w, b, segs, eps, case["slope"], noise=noise, cot_dtype=dt)
    xd, wd, bd = _leaves(x, w, b, dt)
    y = ops.graph_layernorm_lrelu(xd, wd, bd, torch.tensor(segs, dtype=torch.int32, device=DEV), eps, case["slope"])
    y.backward(ref["cot"].to(dt).to(DEV))
    got = dict(y=y.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu())
    _held(f"graph LayerNorm {name}", _ln_figures(got, ref, S.TOL_GRAPHLN, dt, segs))


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=_tag)
def test_graph_layernorm_constant_segment(ops, dt):
    """A segment of x = 0.25 between two of std 1e-4 (eps = 1e-5): sigma = 0 there.  The library's definition: y = leaky_relu(b)
    EXACTLY, dx = r * (dxhat - mean dxhat) with r = 1 / eps -- no third term (the ``sigma > 0 ? ... : 0`` guard of the backward
    kernels; autograd gives NaN there, tests/test_small_constants_cpu.py) -- and everything finite."""
    rows, cols, segs, eps, slope = 48, 256, [0, 16, 32, 48], 1e-5, 0.2
    x, w, b, noise = S.ln_data(48, rows, cols, 1e-4, dt)
    x[16:32] = 0.25
    ref = S.graphln_ref(x, w, b, segs, eps, slope, noise=noise, cot_dtype=dt, third_term="sigma")
    xd, wd, bd = _leaves(x, w, b, dt)
    y = ops.graph_layernorm_lrelu(xd, wd, bd, torch.tensor(segs, dtype=torch.int32, device=DEV), eps, slope)
    y.backward(ref["cot"].to(dt).to(DEV))
    got = dict(y=y.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu())
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    assert torch.equal(got["y"][16:32], F.leaky_relu(b.float(), slope).to(dt).expand(16, -1))
    _held(f"graph LayerNorm constant segment {_tag(dt)}", _ln_figures(got, ref, S.TOL_GRAPHLN, dt, segs))


@pytest.mark.parametrize("regime", ["eps0.5", "mixed"])
def test_graph_layernorm_from_epilogue_partials_against_fp64(ops, regime):
    """egk_graphln_fwd_apply / egk_graphln_bwd_apply: x comes out of a bf16 contraction whose epilogue takes the segment sums (the
    rows of one operand are scaled so that the segments land at std ~ 1 and 0.5 with eps = 0.5, resp. 1e-4 and 3e-6 with eps =
    1e-5), dy out of a dX-shaped contraction against an identity block (dy IS the cotangent) whose epilogue takes the backward sums."""
    M, segs, H, K, slope = 1000, [0, 300, 1000], 256, 512, 0.2
    scales, eps = (S.row_scales(segs, (1e-4, 3e-6)), 1e-5) if regime == "mixed" else (S.row_scales(segs, (1.0, 0.5)), 0.5)
    g = S.gen(1000)
    A = (torch.randn(M, K, generator=g, dtype=F64) * 0.5 * scales[:, None]).to(BF).to(DEV)
    W = (torch.randn(H, K, generator=g, dtype=F64) * 0.1).to(BF).to(DEV)
    w, b = (S.rounded(torch.randn(H, generator=g, dtype=F64), torch.float32) for _ in range(2))
    noise = torch.randn(M, H, generator=g, dtype=F64)
    seg = torch.tensor(segs, dtype=torch.int32, device=DEV)
    out = torch.empty(M, H, dtype=BF, device=DEV)
    got = ops._gemm_with_stats((M, H, A, K, W, K, K, out, H), dict(compute=ops.BF16), dict(mode=1, seg_ptr=seg, n_seg=2, min_rows=300))
    assert got is not None, "the epilogue must take the statistics at this shape"
    x = out.double().cpu()
    for (a, e), s_ in zip(zip(segs[:-1], segs[1:]), scales[[0, 300]].tolist()):
        assert 0.5 * s_ < float(x[a:e].std()) < 2.0 * s_ and abs(float(x[a:e].mean())) < float(x[a:e].std())
    ref = S.graphln_ref(x, w, b, segs, eps, slope, noise=noise, cot_dtype=BF)
    xd, wd, bd = out.clone().requires_grad_(True), w.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
    y, lnctx = ops.graph_layernorm_lrelu(xd, wd, bd, seg, eps, slope, partials=got, min_seg_rows=300, return_ctx=True)
    Gm = torch.zeros(M, K, dtype=BF, device=DEV)
    Gm[:, :H] = ref["cot"].to(BF).to(DEV)
    W2 = torch.zeros(K, H, dtype=BF, device=DEV)
    W2[:H] = torch.eye(H, dtype=BF, device=DEV)
    dy = torch.empty(M, H, dtype=BF, device=DEV)
    ops._ln_bwd_stats_launch(lnctx, (M, H, Gm, K, W2, H, K, dy, H), dict(transB=True, compute=ops.BF16), dy)
    assert lnctx["bwd"] is not None and lnctx["bwd"][2] == dy.data_ptr(), "the dX epilogue must take the backward sums at this shape"
    assert torch.equal(dy.cpu(), ref["cot"].to(BF))
    y.backward(dy)
    res = dict(y=y.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu())
    _held(f"graph LayerNorm from partials {regime}", _ln_figures(res, ref, S.TOL_GRAPHLN, BF, segs))


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=_tag)
def test_graph_layernorm_exchanged_statistics_against_fp64(ops, dt):
    """egk_graphln_stats / _fwd_apply / _bwd_stats / _bwd_finish (ops.set_graph_ln_exchange): this process is rank A (std 1) of
    two, the exchange adds what rank B (std 0.3) contributes, in f64 from the reference; eps = 0.5.  Rank A's y and dx are those of
    the reference over the union of the rows, its dw / db the sums over its own rows."""
    cols, na, nb, eps, slope = 256, [40, 60], [24, 36], 0.5, 0.2
    g = S.gen(77)
    w, b = (S.rounded(torch.randn(cols, generator=g, dtype=F64), torch.float32) for _ in range(2))
    draw = lambda n, s: S.rounded((torch.randn(n, cols, generator=g, dtype=F64) + 0.3) * s, dt)
    xa, xb = [draw(n, 1.0) for n in na], [draw(n, 0.3) for n in nb]
    union = torch.cat([torch.cat([a, bb]) for a, bb in zip(xa, xb)])
    segs_u = [0, na[0] + nb[0], na[0] + nb[0] + na[1] + nb[1]]
    ref = S.graphln_ref(union, w, b, segs_u, eps, slope, noise=torch.randn(union.shape, generator=g, dtype=F64), cot_dtype=dt)
    rows_a = torch.cat([torch.arange(segs_u[k], segs_u[k] + na[k]) for k in range(2)])
    rows_b = [torch.arange(segs_u[k] + na[k], segs_u[k + 1]) for k in range(2)]
    fwd_b = torch.tensor([[union[r].sum(), (union[r] ** 2).sum(), r.numel() * cols] for r in rows_b], dtype=F64)
    bwd_b = torch.tensor([[ref["dxhat"][r].sum(), (ref["dxhat"][r] * ref["xhat"][r]).sum(), r.numel() * cols] for r in rows_b], dtype=F64)
    calls = []

    def exchange(buf):
        assert buf.dtype == F64 and tuple(buf.shape) == (2, 3)
        buf += (fwd_b if not calls else bwd_b).to(buf.device)
        calls.append(1)
    xd, wd, bd = _leaves(union[rows_a], w, b, dt)
    prev = ops.set_graph_ln_exchange(exchange)
    try:
        y = ops.graph_layernorm_lrelu(xd, wd, bd, torch.tensor([0, na[0], na[0] + na[1]], dtype=torch.int32, device=DEV), eps, slope)
        y.backward(ref["cot"][rows_a].to(dt).to(DEV))
    finally:
        ops.set_graph_ln_exchange(prev)
    assert len(calls) == 2
    want = dict(y=ref["y"][rows_a], dx=ref["dx"][rows_a], dw=(ref["gg"] * ref["xhat"])[rows_a].sum(0), db=ref["gg"][rows_a].sum(0))
    got = dict(y=y.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu())
    _held(f"graph LayerNorm exchanged statistics {_tag(dt)}", _ln_figures(got, want, S.TOL_GRAPHLN, dt, [0, na[0], na[0] + na[1]]))


# ---- 3. the Adam and AdamW launches ----------------------------------------------------------------------------------------------------
def _adam_launches():
    """(id, entry point, case): egk_adam_step* run coupled Adam only; the descriptor launches both rules, plain and with two groups."""
    out = []
    for name, case in S.adam_cases():
        if case["grouped"]:
            entries = ["optim_step_groups", "optim_step_ema"]
        elif case["rule"] == "adam":
            entries = ["adam_step", "adam_step_bump", "adam_step_gated", "optim_step", "optim_step_ema"]
        else:
            entries = ["optim_step", "optim_step_ema"]
        out += [(f"{e}-{name}", e, case) for e in entries]
    return out


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("name,entry,case", _adam_launches(), ids=[n for n, _, _ in _adam_launches()])
def test_adam_launches_against_fp64(name, entry, case):
    """p, exp_avg, exp_avg_sq (and the moving average) after steps 1, 2 and 5.  The step constants come from egk_adam_hyper with the
    case's betas.  Elements whose gradient is 0 in every step keep exp_avg == exp_avg_sq == 0 and, without weight decay, their bits."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib
    lib = _lib.load()
    prob = S.adam_problem(case)
    n, rule, gdt, gs = S.ADAM_N, case["rule"], case["gdt"], case["gs"]
    b1, b2, eps = S.ADAM_HYPERS[case["hyper"]]
    wd = S.ADAM_WD[rule]
    p = prob["p"].float().to(DEV)
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    grads = [gr.to(gdt).to(DEV) for gr in prob["grads"]]
    hi, lo = torch.zeros(n, dtype=BF, device=DEV), torch.zeros(n, dtype=BF, device=DEV)
    src = torch.tensor([S.ADAM_LR, gs], dtype=torch.float32, device=DEV)
    hyper, t_dev = torch.zeros(4, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    word, gate = torch.tensor([100], dtype=torch.int64, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    seg_begin = torch.tensor([0, S.GROUP_CUT, (n + 3) // 4 * 4], dtype=torch.int64, device=DEV)
    seg_group = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    group_hyper = torch.zeros(2, 4, device=DEV)
    group_hyper[:, :2] = torch.tensor(S.GROUP_ROWS[rule], dtype=torch.float32)
    figures, g16 = [], 1 if gdt == BF else 0
    for t, gr in enumerate(grads, 1):
        assert lib.egk_adam_hyper(_stream(), _p(src), _p(t_dev), b1, b2, _p(hyper)) == 0, _lib.last_error()
        if entry.startswith("adam_step"):
            args = (_stream(), _p(p), _p(gr), g16, _p(m), _p(v), n, _p(hyper), b1, b2, eps, wd, _p(hi))
            if entry == "adam_step":
                rc = lib.egk_adam_step(*args)
            elif entry == "adam_step_bump":
                rc = lib.egk_adam_step_bump(*args, _p(lo), _p(word), 7)
            else:
                rc = lib.egk_adam_step_gated(*args, _p(lo), _p(word), 7, _p(gate))
        else:
            d = _lib.OptimDesc()
            d.rule, d.g_dtype, d.n = (_lib.OPT_ADAMW if rule == "adamw" else _lib.OPT_ADAM), g16, n
            d.p, d.g, d.state0, d.state1 = p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr()
            d.hyper, d.t_dev = hyper.data_ptr(), t_dev.data_ptr()
            d.beta1, d.beta2, d.eps, d.weight_decay = b1, b2, eps, wd
            d.bf16_shadow, d.bf16_lo_shadow, d.bump_word, d.bump, d.gate = hi.data_ptr(), lo.data_ptr(), word.data_ptr(), 7, gate.data_ptr()
            table = None
            if case["grouped"]:
                table = _lib.OptimGroups()
                table.base, table.n_seg, table.n_groups = 0, 2, 2
                table.seg_begin, table.seg_group, table.group_hyper = seg_begin.data_ptr(), seg_group.data_ptr(), group_hyper.data_ptr()
            if entry == "optim_step_ema":
                e = _lib.EmaDesc()
                e.ema, e.decay, e.warmup = ema.data_ptr(), S.EMA_DECAY, 0
                rc = lib.egk_optim_step_ema(_stream(), C.byref(d), C.byref(table) if table is not None else None, C.byref(e))
            elif entry == "optim_step_groups":
                rc = lib.egk_optim_step_groups(_stream(), C.byref(d), C.byref(table))
            else:
                rc = lib.egk_optim_step(_stream(), C.byref(d))
        assert rc == 0, _lib.last_error()
        if t not in S.ADAM_CHECK:
            continue
        torch.cuda.synchronize()
        want_hyper = torch.tensor([S.ADAM_LR, 1 - b1 ** t, math.sqrt(1 - b2 ** t), gs], dtype=F64)
        assert int(t_dev.item()) == t and float(((hyper.double().cpu() - want_hyper).abs() / want_hyper).max()) <= 2e-7
        ref, state = prob["ref"][t], S.TOL_ADAM_STATE[rule]
        figures.append((f"step{t} p", S.rel_err(p.cpu(), ref["p"]), S.bound_ratio(p.cpu(), ref["p"], S.TOL_ADAM_P)))
        figures.append((f"step{t} p (older bound)", S.rel_err(p.cpu(), ref["p"]), S.older_bound_ratio(p.cpu(), ref["p"])))
        for k, buf in (("m", m), ("v", v)):
            r = S.elementwise_ratio(buf.cpu(), ref[k], state[k])
            figures.append((f"step{t} {k} (per element)", r * state[k], r))
        if entry == "optim_step_ema":
            figures.append((f"step{t} ema", S.rel_err(ema.cpu(), ref["ema"]), S.bound_ratio(ema.cpu(), ref["ema"], S.TOL_EMA)))
    _held(f"Adam launches {name}", figures)
    assert bool((m[::17] == 0).all()) and bool((v[::17] == 0).all())
    if wd == 0:
        assert torch.equal(p[::17].cpu(), prob["p"].float()[::17])
    assert not torch.equal(p[1::17].cpu(), prob["p"].float()[1::17])


# ---- 4. the classes ------------------------------------------------------------------------------------------------------------------
CLASS_SHAPES = [(33, 7), (5,), (64, 64), (3,), (130, 9)]
CLASS_VARIANTS = {"adam": ("adam", torch.optim.Adam, dict(), torch.float32),
                  "adamw": ("adamw", torch.optim.AdamW, dict(weight_decay=1e-2), torch.float32),
                  "adamw-bf16-gradient": ("adamw", torch.optim.AdamW, dict(weight_decay=1e-2), BF)}


@pytest.mark.parametrize("name", list(CLASS_VARIANTS))
def test_flat_classes_with_other_betas_and_eps_against_torch_on_float64(name):
    """FlatAdam / FlatAdamW with betas = (0.8, 0.95), eps = 1e-3 against the torch class stepping float64 copies: the tiny
    gradients of the launch tests, 5 steps, compared after steps 1, 2 and 5."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd.optim import FlatAdam, FlatAdamW
    rule, torch_cls, kw, gdt = CLASS_VARIANTS[name]
    kw = dict(lr=S.ADAM_LR, betas=(0.8, 0.95), eps=1e-3, **kw)
    sizes = [math.prod(s) for s in CLASS_SHAPES]
    total = sum(sizes)
    split = lambda flat: [c.reshape(s) for c, s in zip(flat.split(sizes), CLASS_SHAPES)]
    ps, grads = split(S.adam_params(9, total)), [split(gr) for gr in S.tiny_gradients(13, total, S.ADAM_STEPS, gdt)]
    cpu = [p.clone().requires_grad_(True) for p in ps]
    ref = torch_cls(cpu, **kw)
    dev = [p.float().to(DEV).requires_grad_(True) for p in ps]
    opt = (FlatAdamW if rule == "adamw" else FlatAdam)(dev, **kw)
    figures, state = [], S.TOL_ADAM_STATE[rule]
    for it in range(S.ADAM_STEPS):
        for c, d, gr in zip(cpu, dev, grads[it]):
            c.grad = gr.clone()
            if d.grad is None:
                d.grad = gr.float().to(DEV)
            else:
                d.grad.copy_(gr)
        ref.step()
        if gdt == BF:
            if not opt.materialised:
                opt._materialise()
            opt.step(grads=opt.flat_g.to(BF))
        else:
            opt.step()
        if it + 1 not in S.ADAM_CHECK:
            continue
        sd = opt.state_dict()["state"]
        flat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])
        got_p, want_p = flat(dev), flat(cpu)
        figures.append((f"step{it + 1} p", S.rel_err(got_p, want_p), S.bound_ratio(got_p, want_p, S.TOL_ADAM_P)))
        figures.append((f"step{it + 1} p (older bound)", S.rel_err(got_p, want_p), S.older_bound_ratio(got_p, want_p)))
        for k, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            r = S.elementwise_ratio(flat([sd[i][key] for i in range(len(ps))]), flat([ref.state[c][key] for c in cpu]), state[k])
            figures.append((f"step{it + 1} {key} (per element)", r * state[k], r))
    _held(f"classes {name}", figures)


# ---- 5. the gradient clip --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("name", list(S.CLIP_NORMS))
def test_clip_constant_against_clip_grad_norm(name, gs):
    """FlatAdam(max_grad_norm = 1e-6), one step on a gradient whose norm (of the scaled gradient) is ~1e-6 (coefficient ~0.5; 1
    without the constant), ~1e-9 (~0.999; clamped to 1 without it), ~1e-3 (~1e-3) or exactly 0 (the coefficient clamps to 1: the
    grad_scale word is EXACTLY grad_scale and nothing moves): the coefficient against min(1, max_norm / (norm + 1e-6)), then p,
    exp_avg, exp_avg_sq against the reference stepped on the clipped gradient."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd.optim import FlatAdam
    n = S.ADAM_N
    p0, g = S.adam_params(7, n), S.clip_gradient(23, n, S.CLIP_NORMS[name] / gs)
    norm = gs * float(g.norm())
    coef = S.clip_ref(norm, S.CLIP_MAX_NORM)
    d = p0.float().to(DEV).requires_grad_(True)
    opt = FlatAdam([d], lr=S.ADAM_LR, max_grad_norm=S.CLIP_MAX_NORM)
    opt.grad_scale = gs
    d.grad = g.float().to(DEV)
    opt.step()
    torch.cuda.synchronize()
    word, stats = float(opt._hyper[3].item()), opt.grad_norm_stats()
    assert stats["steps"] == 1 and stats["skipped"] == 0 and stats["clipped"] == int(coef < 1.0)
    assert abs(stats["last_norm"] - norm) <= 2e-7 * norm
    sd = opt.state_dict()["state"][0]
    if name == "norm0":
        assert word == gs and torch.equal(d.detach().cpu(), p0.float())
        assert not bool(sd["exp_avg"].any()) and not bool(sd["exp_avg_sq"].any())
        return
    ref = S.adam_ref(p0, [g], S.ADAM_LR, S.DEFAULT_BETAS, 1e-8, 0.0, gs * coef, check=(1,))[1]
    state = S.TOL_ADAM_STATE["adam"]
    rm, rv = (S.elementwise_ratio(sd[key].cpu().reshape(-1), ref[k], state[k]) for k, key in (("m", "exp_avg"), ("v", "exp_avg_sq")))
    got_p = d.detach().cpu()
    _held(f"clip {name} grad_scale {gs:g}", [("coefficient", abs(word / gs - coef) / coef, abs(word / gs - coef) / (S.TOL_CLIP_COEF * coef)),
                                            ("p", S.rel_err(got_p, ref["p"]), S.bound_ratio(got_p, ref["p"], S.TOL_ADAM_P)),
                                            ("p (older bound)", S.rel_err(got_p, ref["p"]), S.older_bound_ratio(got_p, ref["p"])),
                                            ("exp_avg (per element)", rm * state["m"], rm), ("exp_avg_sq (per element)", rv * state["v"], rv)])
