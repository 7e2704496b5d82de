"""The step matrix without a GPU (tests/step_matrix_common.py): the rows cover every pair of levels, every row's
overrides are a configuration the builders accept, the composed float64 model is reachable in f32 inside the tolerances the GPU
tests use, and every mutant of the model is at least 10 x the tolerance of the tensor it moves away from it."""
import math

import pytest
import torch

from tests import step_matrix_common as M

ROWS = M.rows()
ROW_IDS = [r["id"] for r in ROWS]


# ---- 1. the cover condition ---------------------------------------------------------------------------------------------------------
def test_rows_cover_every_pair_of_levels_in_at_most_16_rows():
    assert len(M.ROWS) <= M.MAX_ROWS and len(set(M.ROWS)) == len(M.ROWS)
    assert M.ROWS[0] == tuple(len(M.LEVELS[f]) - 1 for f in M.FACTORS), "row 0 is not 'all on'"
    assert M.ROWS[1] == tuple(0 for _ in M.FACTORS), "row 1 is not 'all defaults'"
    assert all(len(r) == len(M.FACTORS) and all(0 <= v < len(M.LEVELS[f]) for f, v in zip(M.FACTORS, r)) for r in M.ROWS)
    missing = M.uncovered()
    assert not missing, sorted(missing)
    # the checker itself: without row 0 a pair of two last levels is missing, and a refused pair must name real levels
    assert M.uncovered(M.ROWS[1:2]) and (("rule", 2), ("size", 1)) in M.uncovered(M.ROWS[1:2])
    for a, b, reason in M.REFUSED:
        assert (a, b) in M.all_pairs() or (b, a) in M.all_pairs()
        assert reason
    assert len(ROW_IDS) == len(set(ROW_IDS))


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_the_overrides_of_a_row_are_a_configuration_the_builders_accept(row):
    from egopack_amd import train as T
    cfg = T.load_config(M.overrides(row))
    assert cfg.optimizer._target_ == M.TARGETS[row["rule"]] and float(cfg.optimizer.lr) == M.LR and float(cfg.optimizer.weight_decay) == M.WD
    assert T.class_balance_config(cfg)["mode"] == row["class_balance"]
    sh = T.ce_shape_config(cfg)
    assert (sh["margin"], sh["gamma"] > 0) == (("ldam", True) if M.on(row, "ce_shape") else ("none", False))
    assert T.pnr_balance_config(cfg)["mode"] == row["pnr_balance"]
    assert T.task_weighting_config(cfg)["mode"] == row["task_weighting"]
    st = T.optimizer_state_config(cfg)
    assert (st["dtype"], st["seed"]) == (("bf16", M.STATE_SEED) if M.on(row, "optimizer_state") else ("f32", None))
    assert T.lta_sampling_config(cfg)["mode"] == "torch"
    assert (float(cfg.get("grad_clip_norm", 0) or 0) > 0) == M.on(row, "grad_clip_norm")
    assert (float(dict(cfg.get("ema") or {}).get("decay", 0) or 0) > 0) == M.on(row, "ema")
    # the optimizer the production builder makes of it, over a few host parameters with the modules' shapes of parameters
    ps = [torch.zeros(4, 3, requires_grad=True), torch.zeros(3, requires_grad=True)]
    opt = T.build_optimizer(cfg, ps)
    assert opt.bf16_state == M.on(row, "optimizer_state") and opt.ema == M.on(row, "ema") and opt.clipping == M.on(row, "grad_clip_norm")
    assert len(opt._state_keys) == (1 if row["rule"] == "sgd" else 2)
    if row["rule"] == "sgd":
        assert opt.param_groups[0]["momentum"] == M.MOMENTUM
    # the scalars the PNR criterion gets: train.pnr_scalars on one positive node per sequence
    sh = M.pnr_triple(row, row["size"][1])
    if row["pnr_balance"] == "pos_weight":
        pw = M.T_NODES - 1
        k = M.T_NODES / (pw + M.T_NODES - 1)
        assert sh == pytest.approx((pw * k, k, 0.0), rel=1e-6)
    elif row["pnr_balance"] == "focal":
        assert sh == (0.25, 0.75, 2.0)
    else:
        assert sh is None


# ---- 2. the model is reachable in f32 ---------------------------------------------------------------------------------------------------
def _loss_pair(row):
    inp = M.synthetic_loss_inputs(row)
    args = (row, inp["logits"], inp["labels"], inp["weights"], inp["n_full"], inp["log_var"], inp["batch"])
    return inp, M.loss_model(*args), args


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_an_f32_restatement_of_the_loss_half_stays_inside_the_tolerances(row):
    """The kernel's arithmetic restated in f32 on the host against the float64 model, at the tolerances the GPU test uses."""
    inp, ref, args = _loss_pair(row)
    got = M.loss_restate_f32(*args)
    for t in ("ar", "lta"):
        ltol, gtol = M.ce_tols(row, t, "f32")
        assert M.ratio(got["vectors"][t], ref["vectors"][t], **ltol) <= 1, (t, "loss")
        for h in range(2):
            r = M.ratio(got["operands"][t][h], ref["operands"][t][h], **gtol)
            assert r <= 1, (t, h, r)
    sh = M.pnr_triple(row, inp["batch"]) or (1.0, 1.0, 0.0)
    assert M.ratio(got["vectors"]["pnr"], ref["vectors"]["pnr"], **M.PB.LOSS_TOL) <= 1
    seed_scale = inp["n_full"]["pnr"] / (inp["weights"]["pnr"] * ref["scales"]["pnr"])  # (grad_tol is stated for a seed of 1)
    assert M.ratio(got["operands"]["pnr"] * seed_scale, ref["operands"]["pnr"] * seed_scale, **M.PB.grad_tol(sh[0], sh[1])) <= 1
    # the objective of the f32 vectors against the model's J of the SAME vectors (the launch's own error), and against the model's
    # J of the model's vectors at the loss vectors' tolerance
    J_same, ds_same = M.objective_model(row, got["vectors"], inp["weights"], inp["n_full"], inp["log_var"])
    assert M.ratio(got["objective"], J_same, **M.OBJECTIVE_TOL) <= 1
    assert abs(got["objective"] - ref["objective"]) <= sum(M.ce_tols(row, t, "f32")[0]["atol"] + 2e-5 * abs(float(ref["vectors"][t].mean()))
                                                           for t in ("ar", "lta")) * max(ref["scales"].values()) + 1e-5
    if row["task_weighting"] == "uncertainty":
        assert M.ratio(got["ds"], ds_same, **M.DS_TOL) <= 1


def _update_pair(row, ds=None):
    inp = M.synthetic_update_inputs(row, ds)
    kw = dict(clip=inp["clip"])
    return inp, M.update_model(row, inp["p"], inp["g"], inp["state"], inp["ema"], inp["t"], inp["groups"], **kw), kw


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_an_f32_restatement_of_the_update_half_stays_inside_the_tolerances(row):
    inp, ref, kw = _update_pair(row)
    got = M.update_model(row, inp["p"], inp["g"], inp["state"], inp["ema"], inp["t"], inp["groups"], dtype=torch.float32, **kw)
    assert got["p"].dtype == torch.float32 and not ref["skipped"]
    if M.on(row, "grad_clip_norm"):
        assert ref["coef"] < 0.6, "the clip does not bite"
    assert M.ratio(got["p"], ref["p"], **M.RULE_TOL) <= 1
    for a, b, sc in zip(got["state"], ref["state"], ref["state_scale"]):
        assert M.ratio(a, b, **M.RULE_TOL) <= 1
        assert float(((a.double() - b).abs() / (M.STATE_ULPS * sc + 1e-45)).max()) <= 1  # (the format-derived slack of an f32 moment)
        # what a bf16 state would store of the f32 moment -- either neighbour -- is a value the float64 model admits
        bits = a.float().view(torch.int32)
        for stored in ((bits & -65536).view(torch.float32), ((bits & -65536) + 65536).view(torch.float32)):
            keep = (bits & 0xFFFF) != 0  # (a representable moment is stored unchanged)
            ok = M.bf16_state_ok(torch.where(keep, stored, a.float()), b, sc)
            assert bool(ok.all()), int((~ok).sum())
        # ... and a value two bf16 steps further is not, wherever a bf16 step (2^-8 |x|) is well above the slack (not where the
        # moment cancelled to almost nothing)
        far = ((bits & -65536) + 3 * 65536).view(torch.float32)
        big = b.abs() * 2.0 ** -8 > 4 * M.STATE_ULPS * sc
        assert int(big.sum()) > big.numel() // 2 and not bool(M.bf16_state_ok(far, b, sc)[big].any())
    if M.on(row, "ema"):
        assert M.ratio(got["ema"], ref["ema"], **M.RULE_TOL) <= 1  # (ema's own model is exact given p; p carries the rule's tolerance)
    else:
        assert ref["ema"] is None


def test_a_non_finite_norm_skips_the_step_in_the_model():
    row = ROWS[0]
    inp = M.synthetic_update_inputs(row)
    g = inp["g"].clone()
    g[5] = float("inf")
    out = M.update_model(row, inp["p"], g, inp["state"], inp["ema"], inp["t"], inp["groups"], clip=inp["clip"])
    assert out["skipped"] and out["t"] == inp["t"] - 1 and torch.equal(out["p"].float(), inp["p"]) and out["ema"] is inp["ema"]


# ---- 3. the tests have teeth ------------------------------------------------------------------------------------------------------------
def _moved(name, row):
    """The largest |mutant - model| / tolerance over the tensors the mutant moves, on the synthetic inputs of ``row``."""
    if name in M.LOSS_MUTANTS:
        inp, ref, args = _loss_pair(row)
        mut = M.loss_model(*args, mutant=name)
        what = M.LOSS_MUTANTS[name][1]
        if what == "objective":
            return M.ratio(mut["objective"], ref["objective"], **M.OBJECTIVE_TOL)
        worst = 0.0
        for t in ("ar", "lta"):
            ltol, gtol = M.ce_tols(row, t, row["size"][0])
            if what == "vectors":
                worst = max(worst, M.ratio(mut["vectors"][t], ref["vectors"][t], **ltol))
            else:
                worst = max(worst, *(M.ratio(a, b, **gtol) for a, b in zip(mut["operands"][t], ref["operands"][t])))
        if what == "vectors":
            worst = max(worst, M.ratio(mut["vectors"]["pnr"], ref["vectors"]["pnr"], **M.PB.LOSS_TOL))
        return worst
    inp, ref, kw = _update_pair(row)
    mut = M.update_model(row, inp["p"], inp["g"], inp["state"], inp["ema"], inp["t"], inp["groups"], mutant=name, **kw)
    what = M.UPDATE_MUTANTS[name][1]
    if what == "norm":
        return abs(mut["norm"] - ref["norm"]) / (M.norm_bound(inp["p"].numel()) * ref["norm"])
    if what == "ema":
        return M.ratio(mut["ema"], ref["ema"], **M.RULE_TOL)
    return max(M.ratio(mut["p"], ref["p"], **M.RULE_TOL), *(M.ratio(a, b, **M.RULE_TOL) for a, b in zip(mut["state"], ref["state"])))


@pytest.mark.parametrize("name", list(M.MUTANTS))
def test_every_mutant_is_ten_tolerances_away_in_a_row_that_has_its_factors_on(name):
    applicable = [r for r in ROWS if M.mutant_applies(name, r)]
    assert applicable, f"no row has the factors of {name} on"
    moved = {r["id"]: _moved(name, r) for r in applicable}
    print(name, {k: f"{v:.3g}" for k, v in moved.items()})
    assert max(moved.values()) >= 10, moved
    assert all(math.isfinite(v) or v == float("inf") for v in moved.values())


def test_a_mutant_changes_nothing_in_a_row_without_its_factors():
    """Row 1 (all defaults): the update mutants are the model itself there -- they slip only where features meet."""
    row = ROWS[1]
    inp, ref, kw = _update_pair(row)
    for name in M.UPDATE_MUTANTS:
        if name in ("ema_before_update", "ema_weight_prev"):
            continue
        mut = M.update_model(row, inp["p"], inp["g"], inp["state"], inp["ema"], inp["t"], inp["groups"], mutant=name, **kw)
        assert torch.equal(mut["p"], ref["p"]) and mut["norm"] == ref["norm"], name
