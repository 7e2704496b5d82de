"""The teeth of tests/test_gpu_small_constants.py, checked without a GPU.  For every case of its tables and every mutant that applies:
  * the mutant reference (the constant in another place) is at least 100 x the case's tolerance away from the true reference
    (10 x for the eps placements seen through a bf16 tensor, whose bound carries one bf16 rounding step);
  * in the regime of the OLDER tests (std ~ 1 with eps = 1e-5; N(0, 1) gradients with eps = 1e-8) the same mutants stay below the
    older tolerances -- the reason this file exists;
  * an f32 torch evaluation of the true reference stays within the tolerance: the bound can be reached by f32 arithmetic."""
import pytest
import torch

from tests import small_constants_common as S
from tests.small_constants_common import BF, F64

LN_SENSITIVE = ("y", "dx", "dw")  # (db = sum of the masked cotangent: without an activation it does not see eps at all)


def _eff_tol(tols, dt, k):
    return tols[k] + S.out_steps(dt)[k]


def _margin(dt):
    return 10.0 if dt == BF else 100.0


def _seg_gap(a, b, segs):
    """Largest per-segment max |a - b| / max |b| (segments of very different scale are each read against their own size)."""
    return max(S.rel_err(a[s:e], b[s:e]) for s, e in zip(segs[:-1], segs[1:]))


# ---- row LayerNorm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", S.rowln_cases(), ids=[n for n, _ in S.rowln_cases()])
def test_rowln_mutants_are_separable_and_f32_reaches_the_bound(name, case):
    x, w, b, noise, eps = S.rowln_inputs(case)
    mask = (torch.rand(x.shape, generator=S.gen(3)) < 1 - case["p"]).to(torch.uint8) if case["p"] else None
    kw = dict(relu=case["relu"], mask=mask, p=case["p"])
    true = S.rowln_ref(x, w, b, eps, noise=noise, cot_dtype=case["dt"], **kw)
    for eps_on in ("std", "none"):
        mut = S.rowln_ref(x, w, b, eps, cot=true["cot"], eps_on=eps_on, **kw)
        for k in LN_SENSITIVE:
            gap, need = S.rel_err(mut[k], true[k]), _margin(case["dt"]) * _eff_tol(S.TOL_ROWLN, case["dt"], k)
            assert gap >= need, f"eps_on={eps_on}: {k} moves by {gap:.3g}, needs {need:.3g}"
    f32 = S.rowln_ref(x, w, b, eps, cot=true["cot"], dtype=torch.float32, **kw)
    for k in ("y", "dx", "dw", "db"):
        assert S.bound_ratio(f32[k], true[k], S.TOL_ROWLN[k]) <= 1.0, (k, S.rel_err(f32[k], true[k]))


@pytest.mark.parametrize("rows,cols", S.ROWLN_SHAPES)
def test_rowln_mutants_hide_below_the_older_tolerances_in_the_control_regime(rows, cols):
    case = dict(rows=rows, cols=cols, relu=False, dt=torch.float32, p=0.0)
    x, w, b, noise, eps = S.rowln_inputs(case, regime=S.LN_CONTROL)
    true = S.rowln_ref(x, w, b, eps, noise=noise)
    for eps_on in ("std", "none"):
        mut = S.rowln_ref(x, w, b, eps, cot=true["cot"], eps_on=eps_on)
        for k in ("y", "dx", "dw", "db"):
            assert S.rel_err(mut[k], true[k]) < S.OLD_TOL_LN[k], (eps_on, k)


def test_tolerances_are_not_looser_than_the_older_tests():
    for tols in (S.TOL_ROWLN, S.TOL_GRAPHLN):
        assert all(tols[k] <= S.OLD_TOL_LN[k] for k in tols)
    assert S.TOL_ADAM_P <= S.OLD_TOL_ADAM_P["atol"] + S.OLD_TOL_ADAM_P["rtol"]


# ---- graph LayerNorm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", S.graphln_cases(), ids=[n for n, _ in S.graphln_cases()])
def test_graphln_mutants_are_separable_and_f32_reaches_the_bound(name, case):
    x, w, b, noise, eps = S.graphln_inputs(case)
    segs, dt = case["segs"], case["dt"]
    true = S.graphln_ref(x, w, b, segs, eps, case["slope"], noise=noise, cot_dtype=dt)
    kw = dict(cot=true["cot"])
    for eps_on in ("var", "none"):
        mut = S.graphln_ref(x, w, b, segs, eps, case["slope"], eps_on=eps_on, **kw)
        for k in LN_SENSITIVE:
            gap = _seg_gap(mut[k], true[k], segs) if k != "dw" else S.rel_err(mut[k], true[k])
            need = _margin(dt) * _eff_tol(S.TOL_GRAPHLN, dt, k)
            assert gap >= need, f"eps_on={eps_on}: {k} moves by {gap:.3g}, needs {need:.3g}"
    closed = S.graphln_ref(x, w, b, segs, eps, case["slope"], third_term="sigma", **kw)
    for k in ("dx", "dw", "db"):
        assert _seg_gap(closed[k], true[k], segs if k == "dx" else [0, closed[k].shape[0]]) <= 1e-7, k  # (measured: 1e-15)
    if dt == torch.float32:  # (8.8e-3 is below a bf16 step: the f32 cases carry the third term)
        for third in ("sigma_plus_eps", "dropped"):
            mut = S.graphln_ref(x, w, b, segs, eps, case["slope"], third_term=third, **kw)
            gap = _seg_gap(mut["dx"], true["dx"], segs)
            assert gap >= 100.0 * S.TOL_GRAPHLN["dx"], f"third_term={third}: dx moves by {gap:.3g}"
    f32 = S.graphln_ref(x, w, b, segs, eps, case["slope"], dtype=torch.float32, **kw)
    for k in ("y", "dx"):
        for s, e in zip(segs[:-1], segs[1:]):
            assert S.bound_ratio(f32[k][s:e], true[k][s:e], S.TOL_GRAPHLN[k]) <= 1.0, (k, s, S.rel_err(f32[k][s:e], true[k][s:e]))
    for k in ("dw", "db"):
        assert S.bound_ratio(f32[k], true[k], S.TOL_GRAPHLN[k]) <= 1.0, (k, S.rel_err(f32[k], true[k]))


@pytest.mark.parametrize("rows,cols,segs", S.GRAPHLN_SHAPES)
def test_graphln_mutants_hide_below_the_older_tolerances_in_the_control_regime(rows, cols, segs):
    case = dict(rows=rows, cols=cols, segs=segs, dt=torch.float32)
    x, w, b, noise, eps = S.graphln_inputs(case, regime=S.LN_CONTROL)
    true = S.graphln_ref(x, w, b, segs, eps, 0.2, noise=noise)
    muts = [S.graphln_ref(x, w, b, segs, eps, 0.2, cot=true["cot"], eps_on=e) for e in ("var", "none")]
    muts.append(S.graphln_ref(x, w, b, segs, eps, 0.2, cot=true["cot"], third_term="sigma_plus_eps"))
    for mut in muts:
        for k in ("y", "dx", "dw", "db"):
            assert S.rel_err(mut[k], true[k]) < S.OLD_TOL_LN[k], k


def test_constant_segment_definition_is_finite_where_autograd_is_not():
    """x = 0.25 over a whole segment: sigma = 0.  The closed form with the guard (no third term) is finite and is r * (dxhat - mean
    dxhat); autograd through sqrt(var) gives NaN -- the expectation of the GPU test is the library's definition."""
    x, w, b, noise = S.ln_data(5, 24, 32, 1.0, torch.float32)
    x[8:16] = 0.25
    segs, eps = [0, 8, 16, 24], 1e-5
    ref = S.graphln_ref(x, w, b, segs, eps, 0.2, noise=noise, third_term="sigma")
    assert torch.equal(ref["y"][8:16], torch.nn.functional.leaky_relu(b, 0.2).expand(8, -1))
    assert bool(torch.isfinite(ref["dx"]).all())
    d = ref["dxhat"][8:16]
    torch.testing.assert_close(ref["dx"][8:16], (d - d.mean()) / eps, rtol=1e-10, atol=0)
    auto = S.graphln_ref(x, w, b, segs, eps, 0.2, cot=ref["cot"])
    assert bool(torch.isnan(auto["dx"][8:16]).any())
    torch.testing.assert_close(auto["dx"][:8], ref["dx"][:8], rtol=1e-9, atol=0)


# ---- Adam / AdamW --------------------------------------------------------------------------------------------------------------------
def _p_gap(a, b):
    return max(S.rel_err(a[t]["p"], b[t]["p"]) for t in b)


@pytest.mark.parametrize("name,case", S.adam_cases(), ids=[n for n, _ in S.adam_cases()])
def test_adam_mutants_are_separable_and_f32_reaches_the_bound(name, case):
    prob = S.adam_problem(case)
    p, grads, true = prob["p"], prob["grads"], prob["ref"]
    for eps_at in S.ADAM_EPS_MUTANTS:
        gap = _p_gap(S.adam_eval(case, p, grads, eps_at=eps_at), true)
        assert gap >= 100.0 * S.TOL_ADAM_P, f"eps_at={eps_at}: p moves by {gap:.3g}"
    if S.ADAM_HYPERS[case["hyper"]][:2] != S.DEFAULT_BETAS:
        mut = S.adam_eval(case, p, grads, betas_used=S.DEFAULT_BETAS)
        assert _p_gap(mut, true) >= 100.0 * S.TOL_ADAM_P
        for k in ("m", "v"):  # (every element with a gradient moves)
            live = true[5][k] != 0
            moved = ((mut[5][k] - true[5][k]).abs() / true[5][k].abs())[live]
            assert float(moved.median()) >= 100.0 * S.TOL_ADAM_STATE[case["rule"]][k], k
    f32 = S.adam_eval(case, p, grads, ema_decay=S.EMA_DECAY, dtype=torch.float32)
    for t in S.ADAM_CHECK:
        assert S.bound_ratio(f32[t]["p"], true[t]["p"], S.TOL_ADAM_P) <= 1.0, (t, S.rel_err(f32[t]["p"], true[t]["p"]))
        assert S.bound_ratio(f32[t]["ema"], true[t]["ema"], S.TOL_EMA) <= 1.0
        for k in ("m", "v"):
            assert S.elementwise_ratio(f32[t][k], true[t][k], S.TOL_ADAM_STATE["adamw"][k]) <= 1.0, (t, k)
    zero = torch.zeros(S.ADAM_N, dtype=torch.bool)
    zero[::17] = True
    assert bool((true[5]["m"][zero] == 0).all()) and bool((true[5]["v"][zero] == 0).all()) and bool((true[5]["m"][~zero] != 0).all())


@pytest.mark.parametrize("rule", ["adam", "adamw"])
def test_adam_without_eps_hides_below_the_older_tolerance_with_unit_gradients(rule):
    g = S.gen(61)
    p = S.rounded(torch.randn(S.ADAM_N, generator=g, dtype=F64), torch.float32)
    grads = [S.rounded(torch.randn(S.ADAM_N, generator=g, dtype=F64), torch.float32) for _ in range(S.ADAM_STEPS)]
    case = dict(rule=rule, hyper="b0.9-0.999-eps1e-8", gs=1.0, gdt=torch.float32, grouped=False)
    true, mut = S.adam_eval(case, p, grads), S.adam_eval(case, p, grads, eps_at="none")
    for t in true:
        diff, want = (mut[t]["p"] - true[t]["p"]).abs(), true[t]["p"].abs()
        assert bool((diff <= S.OLD_TOL_ADAM_P["atol"] + S.OLD_TOL_ADAM_P["rtol"] * want).all())


# ---- gradient clip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.CLIP_NORMS))
def test_clip_constant_is_separable(name):
    g = S.clip_gradient(23, S.ADAM_N, S.CLIP_NORMS[name])
    norm = float(g.norm())
    coef, mut = S.clip_ref(norm, S.CLIP_MAX_NORM), S.clip_ref(norm, S.CLIP_MAX_NORM, constant=0.0)
    f32 = torch.tensor(S.CLIP_MAX_NORM, dtype=torch.float32) / (torch.tensor(norm, dtype=torch.float32) + torch.tensor(1e-6, dtype=torch.float32))
    assert abs(min(1.0, float(f32)) - coef) <= S.TOL_CLIP_COEF * coef
    if name == "norm0":
        assert coef == mut == 1.0  # (clamped either way: the GPU test asserts the exact grad_scale word and untouched parameters)
        return
    assert abs(mut - coef) / coef >= 100.0 * S.TOL_CLIP_COEF
    assert {"norm1e-6": 0.45 < coef < 0.55 and mut == 1.0, "norm1e-9": 0.998 < coef < 1.0 and mut == 1.0,
            "norm1e-3": 0.9e-3 < coef < 1.1e-3}[name]
    p = S.adam_params(7, S.ADAM_N)
    a = S.adam_ref(p, [g], S.ADAM_LR, S.DEFAULT_BETAS, 1e-8, 0.0, coef, check=(1,))[1]
    b = S.adam_ref(p, [g], S.ADAM_LR, S.DEFAULT_BETAS, 1e-8, 0.0, mut, check=(1,))[1]
    moved = ((a["m"] - b["m"]).abs() / a["m"].abs()).min()
    assert float(moved) >= 100.0 * S.TOL_ADAM_STATE["adam"]["m"]
    if name == "norm1e-6":
        assert S.rel_err(b["p"], a["p"]) >= 100.0 * S.TOL_ADAM_P
