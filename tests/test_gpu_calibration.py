"""Temperature calibration on the GPU (include/egopack_calibrate.h, egopack_amd/calibration.py): the four launches against the host
models of tests/calibration_common.py, the fit, the sampler's temperature, and the meters and entry points end to end.

Everything integer -- the counts, accumulation over launches, merged shards, the beta = 1 pin against egk_class_report -- and the
Newton launch are EXACT.  The sums acc[0..2] are held to the float64 model by

    |acc[i] / 2^24 - ref_i| <= TOL_i * sum_r |ref row value| + rows * 2^-25

TOL_i = 4 x the worst error of a plain f32 torch restatement of the row arithmetic against float64, measured on the CPU over this
file's statistics inputs (tests/test_calibration_cpu.py::test_the_f32_restatement_fixes_the_tolerances asserts the measurement;
the factor 4 allows for the kernel's other summation order and its expf; 2^-25 per row is the q24 rounding):

                    nll        d1         d2
    measured        1.2e-7     3.5e-6     1.05e-4     (d2: a peaked one-row case at beta = 20, where z - m cancels)
    pinned          1.3e-7     3.6e-6     1.1e-4
    TOL = 4 x       5.2e-7     1.44e-5    4.4e-4      (d2 may stay loose: it only steers the Newton step)

A fitted beta has no tolerance of its own: the float64 F' and F'' at the returned beta must satisfy
|F'| <= 2 * (TOL_1 * sum_r |d1_ref| + stop * beta * F'') -- what the statistics tolerance admits in F', plus what the stop rule
leaves, the two taken as independent."""
import ctypes

import numpy as np
import pytest
import torch

from tests import calibration_common as CM
from tests import topk_common as TK

pytestmark = pytest.mark.gpu
f32, bf16, i64, f64 = torch.float32, torch.bfloat16, torch.int64, torch.float64
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops
    return ops


def word(v):
    return torch.tensor([v], dtype=f32, device=DEV)


def stats(ops, z, y, beta, acc=None):
    acc = torch.zeros(8, dtype=i64, device=DEV) if acc is None else acc
    ops.temp_stats(z, y, beta if torch.is_tensor(beta) else word(beta), acc)
    return acc


def padded(z, pad_to=8):
    """The same values as a view of a buffer whose leading dimension is C rounded up to ``pad_to``, NaN in the pad columns."""
    rows, C = z.shape
    ld = (C + pad_to - 1) // pad_to * pad_to
    buf = torch.full((rows, ld), float("nan"), dtype=z.dtype, device=z.device)
    buf[:, :C] = z
    return buf[:, :C]


# ---- 1. the statistics ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", CM.STATS_ROWS)
@pytest.mark.parametrize("C", CM.STATS_C)
def test_statistics_equal_the_float64_model(ops, C, rows):
    z32, y = CM.stats_problem(C, rows)
    yd = y.to(DEV)
    for beta in CM.STATS_BETAS:
        ref = CM.sums_model(z32, y, beta)
        first = None
        for dt in (f32, bf16):
            zd = z32.to(dt).to(DEV)
            for view in (zd, padded(zd)):
                got = stats(ops, view, yd, beta).tolist()
                assert got[3:] == [ref["valid"], ref["ignored"], ref["left_out"], 0, 0], (dt, beta, got, ref)
                for i, (key, mag) in enumerate((("F", "A0"), ("F1", "A1"), ("F2", "A2"))):
                    err, bound = abs(got[i] / CM.Q24 - ref[key]), CM.acc_bound(i, ref[mag], ref["counted"])
                    print(f"C={C} rows={rows} beta={beta:g} {dt} ld={view.stride(0)} {key}: err {err:.3e} bound {bound:.3e}")
                    assert err <= bound, (key, dt, beta, got[i] / CM.Q24, ref[key], err, bound)
                first = first or got
                assert got == first, "f32 and bf16 logits of the same values, padded or not, give the same integers"


@pytest.mark.parametrize("C", [115, 513])
def test_accumulation_and_merged_shards_are_exact(ops, C):
    z, y = CM.stats_problem(C, 257)
    zd, yd = z.to(DEV), y.to(DEV)
    for beta in CM.STATS_BETAS:
        one = stats(ops, zd, yd, beta)
        twice = stats(ops, zd, yd, beta, stats(ops, zd, yd, beta))
        assert torch.equal(twice, 2 * one), "two launches into one accumulator"
        cuts = [0, 90, 91, 257]
        shards = [stats(ops, zd[a:b], yd[a:b], beta) for a, b in zip(cuts, cuts[1:])]
        assert torch.equal(shards[0] + shards[1] + shards[2], one), "three row shards, added"
        again = stats(ops, zd, yd, beta)
        assert torch.equal(again, one), "two runs"


@pytest.mark.parametrize("C", [2, 115, 478, 513])
def test_at_beta_1_the_nll_sum_is_the_class_reports_loss_sum(ops, C):
    """The same row function, the same bits: acc[0] == sum of egk_class_report's loss_q24 over the same rows, as integers."""
    from egopack_amd import meters as M
    z, y = CM.stats_problem(C, 257)
    zd, yd = z.to(DEV), y.to(DEV)
    state = M._ClassReport(C, DEV)
    M.class_report([(zd, yd, state)])
    acc = stats(ops, zd, yd, 1.0).tolist()
    assert acc[0] == int(state.loss_q24.sum()) and acc[3] == int(state.counts[0]) and acc[4] == int(state.counts[1])
    assert acc[5] == int(state.counts[2]) == 0


def test_rows_and_betas_that_are_left_out(ops):
    z, _ = CM.stats_problem(115, 6)
    y = torch.tensor([3, 7, 11, -1, 200, 5])
    z[0, 9] = float("nan")
    z[1, 4] = float("inf")
    z[2, 50] = float("-inf")  # a -inf logit in a finite row: a valid row
    zd, yd = z.to(DEV), y.to(DEV)
    got = stats(ops, zd, yd, 1.0).tolist()
    ref = CM.sums_model(z, y, 1.0)
    assert got[3:] == [4, 2, 2, 0, 0] == [ref["valid"], ref["ignored"], ref["left_out"], 0, 0]
    for i, (key, mag) in enumerate((("F", "A0"), ("F1", "A1"), ("F2", "A2"))):
        assert abs(got[i] / CM.Q24 - ref[key]) <= CM.acc_bound(i, ref[mag], 2), (key, got[i] / CM.Q24, ref[key])
    for bad in (0.0, float("nan"), -1.0, float("inf")):
        assert stats(ops, zd, yd, bad).tolist() == [0, 0, 0, 4, 2, 4, 0, 0], bad


# ---- 2. the Newton launch ---------------------------------------------------------------------------------------------------------------
def test_one_newton_launch_equals_the_numpy_model_bit_for_bit(ops):
    g = CM.gen(5)
    heads = []
    for h in range(8):
        F1, F2 = float(torch.randn((), generator=g)) * 10, float(torch.rand((), generator=g)) * 20
        b = float(np.float32(0.1 + 3 * float(torch.rand((), generator=g))))
        st = [b, float(np.float32(b / 2)), float(np.float32(b * 2)), float(h & 1), float((h >> 1) & 1), 1.0 if h == 5 else 0.0, float(h), 0.125]
        heads.append(([123, int(round(F1 * CM.Q24)), int(round(F2 * CM.Q24)), 50, 3, 1, 0, 0], st))
    acc = torch.tensor([a for a, _ in heads], dtype=i64, device=DEV)
    state = torch.tensor([s for _, s in heads], dtype=f64, device=DEV)
    beta = torch.tensor([s[0] for _, s in heads], dtype=f32, device=DEV)
    before = (state.clone(), beta.clone())
    ops.temp_newton(acc, state, beta, CM.BETA_MIN, CM.BETA_MAX, CM.STOP)
    want = [CM.newton_step(a, s) for a, s in heads]
    ws = torch.tensor([w[0] for w in want], dtype=f64)
    wb = torch.tensor([s[0] if w[1] is None else w[1] for w, (_, s) in zip(want, heads)], dtype=f32)
    assert torch.equal(state.cpu().view(i64), ws.view(i64)), (state.cpu(), ws)
    assert torch.equal(beta.cpu().view(torch.int32), wb.view(torch.int32))
    assert torch.equal(state[5], before[0][5]) and torch.equal(beta[5], before[1][5]), "a frozen head does not move"
    assert not torch.equal(state[0], before[0][0])


def device_fit(ops, shards, iterations=CM.ITERATIONS):
    """The iteration on the device for ONE head whose rows are given as shards, each with an accumulator of its own that are added
    before the Newton launch (what an all-reduce over ranks does): the final (state, beta) as host lists."""
    beta = torch.ones(1, dtype=f32, device=DEV)
    state = torch.tensor([CM.newton_init()], dtype=f64, device=DEV)
    for _ in range(iterations):
        accs = [stats(ops, z, y, beta) for z, y in shards]
        acc = torch.stack(accs).sum(0).reshape(1, 8)
        ops.temp_newton(acc, state, beta, CM.BETA_MIN, CM.BETA_MAX, CM.STOP)
    return state.cpu()[0].tolist(), beta.cpu().tolist()


@pytest.mark.parametrize("beta_true", CM.FIT_BETAS)
@pytest.mark.parametrize("C", CM.FIT_C)
def test_a_full_fit_converges_to_the_root_of_the_float64_derivative(ops, C, beta_true):
    from egopack_amd import calibration as CAL
    z, y = CM.fit_problem(C, beta_true)
    store = CAL.LogitStore({"h_": C}, device=DEV)
    for o, (a, b) in enumerate(((0, 100), (100, 257))):
        store.append("h_", z[a:b].to(DEV), y[a:b].to(DEV), ordinal=o)
    res = CAL.fit(store, dict(t_range=list(CM.T_RANGE), iterations=CM.ITERATIONS, stop=1e-6))["h_"]
    assert res["status"] == "converged" and res["rows"] == 257 and res["left_out"] == 0 and res["iterations"] <= 12, res
    assert res["folds"]["A"]["rows"] == 100 and res["folds"]["B"]["rows"] == 157 and res["folds"]["A"]["status"] == "converged"
    m = CM.sums_model(z, y, res["beta"])
    bound = 2 * (CM.TOL[1] * m["A1"] + CM.STOP * res["beta"] * m["F2"])
    print(f"C={C} beta_true={beta_true}: beta {res['beta']:.6f}, |F'| {abs(m['F1']):.3e}, bound {bound:.3e}, iterations {res['iterations']}")
    assert abs(m["F1"]) <= bound, (res, m["F1"], bound)
    assert abs(res["temperature"] - 1.0 / res["beta"]) <= 1e-12
    raw = CM.sums_model(z, y, 1.0)
    assert abs(res["nll"] - raw["F"] / 257) <= CM.acc_bound(0, raw["A0"], 257) / 257
    assert abs(res["nll_calibrated"] - m["F"] / 257) <= CM.acc_bound(0, m["A0"], 257) / 257
    assert res["nll_calibrated"] <= res["nll"] + CM.acc_bound(0, raw["A0"], 257) / 257
    # the same head through the bare launches, its rows in three shards: the single pass's bits
    zd, yd = z.to(DEV), y.to(DEV)
    single = device_fit(ops, [(zd, yd)])
    merged = device_fit(ops, [(zd[:90], yd[:90]), (zd[90:91], yd[90:91]), (zd[91:], yd[91:])])
    assert single == merged and single[1][0] == res["beta"] and single[0][5] == 1.0


def test_the_separable_and_the_inverted_problem_end_at_the_bounds(ops):
    z, _ = CM.fit_problem(115, 1.0)
    zd = z.to(DEV)
    hi, hb = device_fit(ops, [(zd, zd.argmax(1))])
    lo, lb = device_fit(ops, [(zd, zd.argmin(1))])
    assert hi[5] == 3.0 and hb == [CM.BETA_MAX] and hi[6] <= 12, hi
    assert lo[5] == 2.0 and lb == [CM.BETA_MIN] and lo[6] <= 12, lo
    none, nb = device_fit(ops, [(zd, torch.full((257,), -1, dtype=i64, device=DEV))], iterations=2)
    assert none[5] == 4.0 and none[6] == 1.0 and nb == [1.0]


# ---- 3. the probabilities of a given order ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [f32, bf16])
@pytest.mark.parametrize("C", [2, 115, 478, 513])
def test_topk_prob_equals_the_model_and_at_beta_1_the_topk_launch(ops, C, dt):
    from tests.test_gpu_bounds_calibration import topk_prob_model
    z, _ = CM.stats_problem(C, 257, dt)
    zd, k = z.to(DEV), min(5, C)
    (idx, prob1, lse1), = ops.topk_softmax([zd], k, want_prob=True, want_lse=True)
    keep = idx.clone()
    for beta in (0.05, 0.5, 1.0, 2.0, 20.0):
        prob, lse = ops.temp_topk_prob(zd, idx, word(beta), want_lse=True)
        p64, l64 = topk_prob_model(z, idx.cpu(), beta)
        # tests/test_gpu_topk.py's tolerance is the f32 cross entropy's at logits of magnitude <= 16 or so.  p = expf(fl(x - lse)):
        # the f32 difference alone is off by up to 2^-24 |x - lse|, the f32 lse by as much again, and that error is RELATIVE in p.
        # So the relative bound is max(that tolerance, 4 * 2^-24 * max |beta z|) -- the factor 4: the two roundings, logf and expf.
        # It is the former up to beta = 2 (max |x| < 40) and 8e-5 at beta = 20 (max |x| about 350), which f32 cannot do better at.
        tol = dict(TK.PROB_TOL, rtol=max(TK.PROB_TOL["rtol"], 4 * 2.0 ** -24 * CM.beta32(beta) * float(z.float().abs().max())))
        assert tol["rtol"] == TK.PROB_TOL["rtol"] or beta == 20.0
        np.testing.assert_allclose(prob.cpu().numpy(), p64.numpy(), err_msg=f"prob at {beta}", **tol)
        np.testing.assert_allclose(lse.cpu().numpy(), l64.numpy(), err_msg=f"lse at {beta}", **TK.PROB_TOL)
        if beta == 1.0:
            assert torch.equal(prob.view(torch.int32), prob1.view(torch.int32)) and torch.equal(lse.view(torch.int32), lse1.view(torch.int32))
    assert torch.equal(idx, keep), "idx is an input"
    holes = idx.clone()
    holes[::3, -1] = -1
    prob, _ = ops.temp_topk_prob(zd, holes, word(0.5))
    assert bool((prob[::3, -1] == 0).all()) and bool((prob[1::3] > 0).all()) and torch.equal(holes[::3, -1], torch.full_like(holes[::3, -1], -1))


@pytest.mark.parametrize("dt", [f32, bf16])
def test_scale_rows_is_one_f32_product_per_element(ops, dt):
    for C, rows in ((1, 1), (115, 257), (513, 5), (2, 8200)):
        z, _ = CM.stats_problem(C, rows, dt)
        zd = z.to(DEV)
        for beta in (0.3, 1.0, 7.0):
            want = word(beta) * zd.float()
            assert torch.equal(ops.temp_scale_rows(zd, word(beta)).view(torch.int32), want.view(torch.int32))
            out = torch.full((rows, C + 3), float("nan"), device=DEV)
            got = ops.temp_scale_rows(padded(zd), word(beta), out=out)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool(out[:, C:].isnan().all())


# ---- 4. the sampler -----------------------------------------------------------------------------------------------------------------------
def test_the_sampler_at_temperature_1_is_todays_and_at_2_draws_from_the_scaled_copy(ops):
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    lib = _lib.load()
    heads = [CM.logits(44, 115, 1).to(DEV), CM.logits(44, 478, 2).to(DEV)]
    with _counted(lib) as base:
        want = ops.categorical_sample_multi(heads, 5, 9, 3)
    with _counted(lib) as one:
        got = ops.FutureSampler(9, temperature=1.0)(heads, 5, 3)
    assert one.names == base.names == {"categorical_sample": 1}
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with _counted(lib) as two:
        got = ops.FutureSampler(9, temperature=2.0)(heads, 5, 3)
    assert two.names == {"categorical_sample": 1, "temp_scale_rows": 2}
    scaled = [ops.temp_scale_rows(h, word(0.5)) for h in heads]
    assert all(torch.equal(s, 0.5 * h) for s, h in zip(scaled, heads))
    want2 = ops.categorical_sample_multi(scaled, 5, 9, 3)
    assert all(torch.equal(a, b) for a, b in zip(got, want2)) and not all(torch.equal(a, b) for a, b in zip(got, want))


# ---- 5. the meters and the entry points -------------------------------------------------------------------------------------------------
HEADS = {"ar": ("verbs_", "nouns_"), "lta": ("verbs_", "nouns_"), "oscc": ("",)}
NEW = ("temperature", "nll", "nll_calibrated", "calibration_erorr_calibrated", "brier_score_calibrated")


@pytest.fixture(scope="module")
def run(tmp_path_factory, ops):
    import calibrate
    import main_temporal
    import predict
    tmp = tmp_path_factory.mktemp("calibration")
    common = ["k=1", "batch_size=4", "num_epochs=1", "synthetic_samples=16", "synthetic_val_samples=10", "model.hidden_size=64",
              "model.temporal_pooling.hidden_size=64", "oscc_feat_size=64", f"checkpoint_dir={tmp}", "save_model=True", "compute=f32",
              "optimizer.lr=1e-3", "enabled_tasks=[ar,lta,oscc,pnr]", "lta_sampling.mode=philox"]
    off = main_temporal.main(common)
    ckpt = tmp / "MTL_ar-lta-oscc-pnr" / "checkpoint.pth"
    assert ckpt.exists() and not list(ckpt.parent.glob("calibration_*.pt")), "mode none writes no calibration file"
    cal = calibrate.main(common + [f"resume_from={ckpt}"])
    raw = predict.main(common + [f"resume_from={ckpt}", f"predict.out={tmp / 'raw'}", "calibration.predict=false"])
    auto = predict.main(common + [f"resume_from={ckpt}", f"predict.out={tmp / 'auto'}"])
    on = main_temporal.validate_metrics(0, auto["model"], auto["tasks"], ["ar", "lta", "oscc", "pnr"], auto["datasets"], auto["loaders"], "cuda",
                                        sampler=ops.FutureSampler(0), report=lambda t: {} if t == "pnr" else dict(
                                            calibration=dict(t_range=[0.05, 20.0], iterations=16, stop=1e-6, max_rows=1 << 20)))
    plain = main_temporal.validate_metrics(0, auto["model"], auto["tasks"], ["ar", "lta", "oscc", "pnr"], auto["datasets"], auto["loaders"],
                                           "cuda", sampler=ops.FutureSampler(0))
    return dict(tmp=tmp, ckpt=ckpt, off=off, cal=cal, raw=raw["predictions"], auto=auto["predictions"], on=on, plain=plain)


@pytest.mark.timeout(600)
def test_calibrate_writes_the_files_and_predict_keeps_every_order(run):
    for t, prefixes in HEADS.items():
        blob = torch.load(run["ckpt"].parent / f"calibration_{t}.pt", weights_only=False)
        assert set(blob["heads"]) == set(prefixes) and blob["t_range"] == [0.05, 20.0] and blob["split"] == "validation" and blob["task"] == t
        for p in prefixes:
            h = blob["heads"][p]
            assert 0.05 <= h["temperature"] <= 20.0 and h["status"] in ("converged", "at_beta_min", "at_beta_max") and h["rows"] > 0, (t, p, h)
            assert set(h["folds"]) == {"A", "B"}
        raw, auto = run["raw"][t], run["auto"][t]
        assert "temperature" not in raw and auto["temperature"] == {(p.rstrip("_") or "oscc"): blob["heads"][p]["temperature"] for p in prefixes}
        changed = {"verb_prob", "noun_prob", "verb_lse", "noun_lse", "prob_change", "lse", "temperature"}
        assert set(auto) - set(raw) == {"temperature"}
        for k, v in raw.items():
            if k not in changed:
                same = torch.equal(v, auto[k]) if torch.is_tensor(v) else v == auto[k]
                assert same, f"{t}: {k} differs between the calibrated and the raw export"
        if t == "oscc":
            assert torch.equal(raw["pred"], auto["pred"])
            T = blob["heads"][""]["temperature"]
            if abs(T - 1.0) > 1e-3:
                assert not torch.equal(raw["prob_change"], auto["prob_change"])
            assert torch.equal(raw["prob_change"] > 0.5, auto["prob_change"] > 0.5) or bool(((raw["prob_change"] - 0.5).abs() < 1e-6).any())
        else:
            assert torch.equal(raw["verb_topk"], auto["verb_topk"]) and torch.equal(raw["noun_topk"], auto["noun_topk"])
            for name, p in (("verb", "verbs_"), ("noun", "nouns_")):
                lse_b = auto[f"{name}_lse"]
                assert bool(torch.isfinite(lse_b).all()) and bool((auto[f"{name}_prob"] > 0).all()) and bool((auto[f"{name}_prob"].sum(1) <= 1 + 1e-5).all())
    assert not (run["ckpt"].parent / "calibration_pnr.pt").exists() and "temperature" not in run["auto"]["pnr"]
    assert all(torch.equal(v, run["auto"]["pnr"][k]) if torch.is_tensor(v) else v == run["auto"]["pnr"][k] for k, v in run["raw"]["pnr"].items())


@pytest.mark.timeout(600)
def test_the_meters_log_the_new_keys_with_calibration_on_and_the_old_ones_without(run):
    for t, prefixes in HEADS.items():
        on, plain = run["on"][t], run["plain"][t]
        new = {f"{p}{k}" for p in prefixes for k in NEW}
        assert new <= set(on), sorted(new - set(on))
        assert set(on) - set(plain) <= new | {f"{p}calibration_in_sample" for p in prefixes}
        assert set(plain) == set(run["off"]["metrics"][t]), "mode none logs exactly the old keys"
        for k, v in plain.items():
            if not k.endswith("_ed"):
                assert on[k] == v, f"{t}: {k} moved with calibration on"
        for p in prefixes:
            fit = run["cal"]["calibration"][t][p]
            assert on[f"{p}temperature"] == fit["temperature"], "the validation's fit is calibrate.py's: the same rows, the same bits"
            # 1 lies in [beta_min, beta_max]: a converged or at-bound fit is no worse than T = 1 (slack: the nll tolerance per row)
            assert on[f"{p}nll_calibrated"] <= on[f"{p}nll"] + CM.TOL[0] * abs(on[f"{p}nll"]) + 2.0 ** -25, (t, p, on)
            assert 0.0 <= on[f"{p}calibration_erorr_calibrated"] <= 1.0 and 0.0 <= on[f"{p}brier_score_calibrated"] <= 1.0
    assert set(run["on"]["pnr"]) == set(run["plain"]["pnr"])
