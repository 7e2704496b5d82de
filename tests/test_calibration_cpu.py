"""Temperature calibration without a GPU: the float64 model of the objective (tests/calibration_common.py) against finite
differences, the Newton rule's model on the inputs the GPU tests fit, every host-side refusal of the four entry points, the
``calibration:`` config block, the meters' keys with ``mode: none``, and the f32-restatement measurement that fixes the tolerances
of tests/test_gpu_calibration.py."""
import ctypes

import numpy as np
import pytest
import torch

from egopack_amd import _lib
from tests import calibration_common as CM

vp = ctypes.c_void_p


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 115])
def test_the_derivatives_are_the_central_differences_of_the_objective(C):
    z, y = CM.fit_problem(C, 1.0)
    for b in (0.25, 1.0, 3.0):
        h = 2.0 ** -12  # (b, b - h and b + h are f32 values: beta32 changes none of them)
        lo, mid, hi = (CM.sums_model(z, y, v) for v in (b - h, b, b + h))
        d1 = (hi["F"] - lo["F"]) / (2 * h)
        d2 = (hi["F1"] - lo["F1"]) / (2 * h)
        assert abs(d1 - mid["F1"]) <= 1e-5 * max(mid["A1"], 1.0), (b, d1, mid["F1"])
        assert abs(d2 - mid["F2"]) <= 1e-5 * max(mid["A2"], 1.0), (b, d2, mid["F2"])


def test_the_objective_is_convex_and_the_fit_is_no_worse_than_t_1():
    for C in CM.FIT_C:
        for bt in CM.FIT_BETAS:
            z, y = CM.fit_problem(C, bt)
            betas = [CM.beta32(v) for v in np.geomspace(CM.BETA_MIN, CM.BETA_MAX, 25)]
            F1 = [CM.sums_model(z, y, b)["F1"] for b in betas]
            assert all(CM.sums_model(z, y, b)["F2"] >= 0 for b in betas)
            assert all(a <= b + 1e-9 * (abs(a) + abs(b)) for a, b in zip(F1, F1[1:])), "F' must not decrease"
            st = CM.fit_model(z, y)
            assert CM.sums_model(z, y, st[0])["F"] <= CM.sums_model(z, y, 1.0)["F"]


# ---- 2. the Newton rule on the GPU test's inputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CM.FIT_C)
@pytest.mark.parametrize("beta_true", CM.FIT_BETAS)
def test_the_newton_model_converges_on_the_fit_inputs_within_12_iterations(C, beta_true):
    """A condition on the INPUTS of tests/test_gpu_calibration.py's fits: status 1 in at most 12 of the 16 iterations."""
    z, y = CM.fit_problem(C, beta_true)
    st = CM.fit_model(z, y)
    assert st[5] == 1.0 and st[6] <= 12, st
    assert CM.BETA_MIN < st[0] < CM.BETA_MAX and st[0] == float(np.float32(st[0]))  # (the iterate is an f32 value)
    assert abs(np.log(st[0] / beta_true)) < np.log(1.6), (st[0], beta_true)  # (257 rows: the estimate is near the truth)


def test_the_two_bound_cases_end_at_the_bounds():
    z, _ = CM.fit_problem(115, 1.0)
    hi = CM.fit_model(z, z.argmax(1))  # separable: the sharper the better
    lo = CM.fit_model(z, z.argmin(1))  # inverted: the flatter the better
    assert hi[5] == 3.0 and hi[0] == CM.BETA_MAX and hi[6] <= 12, hi
    assert lo[5] == 2.0 and lo[0] == CM.BETA_MIN and lo[6] <= 12, lo


def test_a_frozen_head_and_a_head_without_rows():
    st = [0.75, 0.5, 1.0, 1.0, 1.0, 1.0, 5.0, 1e-7]
    assert CM.newton_step([1, 2, 3, 4, 0, 0, 0, 0], st) == (st, None)
    new, word = CM.newton_step([0, 0, 0, 3, 5, 3, 0, 0], CM.newton_init())
    assert new[5] == 4.0 and new[6] == 1.0 and word is None and new[0] == 1.0


# ---- 3. the host-side refusals ---------------------------------------------------------------------------------------------------------
def test_every_argument_error_is_refused_on_the_host_naming_the_entry_point_and_the_argument():
    """Small fake non-null pointers are safe: every check precedes the first dereference and the first launch."""
    lib = _lib.load()
    A, U4, U2 = vp(0x1000), vp(0x1004), vp(0x1002)
    F32, BF16 = 0, 1

    def refused(rc, *needles):
        err = _lib.last_error()
        assert rc == -1 and all(n in err for n in needles), (rc, err)

    stats = lambda logits=A, ld=8, labels=A, rows=4, C=8, beta=A, acc=A, dt=F32: lib.egk_temp_stats(None, logits, ld, labels, 1, rows, C, beta, acc, dt)
    for kw, arg in ((dict(logits=None), "logits"), (dict(labels=None), "labels"), (dict(beta=None), "beta"), (dict(acc=None), "acc")):
        refused(stats(**kw), "egk_temp_stats", "null pointer", arg)
    refused(stats(rows=-1), "egk_temp_stats", "rows")
    refused(stats(C=0), "egk_temp_stats", "C >= 1")
    refused(stats(ld=7), "egk_temp_stats", "ld >= C")
    refused(stats(acc=U4), "egk_temp_stats", "misaligned acc")
    refused(stats(labels=U4), "egk_temp_stats", "misaligned labels")
    refused(stats(logits=U2), "egk_temp_stats", "misaligned logits")
    refused(stats(beta=U2), "egk_temp_stats", "misaligned beta")
    refused(stats(dt=2), "egk_temp_stats", "dtype")
    assert stats(logits=U2, dt=BF16, rows=0) == 0 and stats(rows=0) == 0  # (no rows: nothing is launched)

    newton = lambda acc=A, n=2, state=A, beta=A, bmin=0.05, bmax=20.0, stop=1e-6: lib.egk_temp_newton(None, acc, n, state, beta, bmin, bmax, stop)
    for kw, arg in ((dict(acc=None), "acc"), (dict(state=None), "state"), (dict(beta=None), "beta")):
        refused(newton(**kw), "egk_temp_newton", "null pointer", arg)
    refused(newton(n=0), "egk_temp_newton", "n_heads")
    refused(newton(n=9), "egk_temp_newton", "n_heads")
    refused(newton(acc=U4), "egk_temp_newton", "misaligned acc")
    refused(newton(state=U4), "egk_temp_newton", "misaligned state")
    refused(newton(bmin=0.0), "egk_temp_newton", "beta_min")
    refused(newton(bmin=-1.0), "egk_temp_newton", "beta_min")
    refused(newton(bmin=2.0, bmax=1.0), "egk_temp_newton", "beta_max")
    refused(newton(stop=-1e-3), "egk_temp_newton", "stop")
    refused(newton(stop=float("nan")), "egk_temp_newton", "stop")

    topk = lambda logits=A, ld=8, rows=4, C=8, beta=A, idx=A, istride=5, k=5, prob=A, pstride=5, lse=None, dt=F32: \
        lib.egk_temp_topk_prob(None, logits, ld, rows, C, beta, idx, istride, k, prob, pstride, lse, dt)
    for kw, arg in ((dict(logits=None), "logits"), (dict(beta=None), "beta"), (dict(idx=None), "idx"), (dict(prob=None), "prob")):
        refused(topk(**kw), "egk_temp_topk_prob", "null pointer", arg)
    refused(topk(rows=-1), "egk_temp_topk_prob", "rows")
    refused(topk(C=0), "egk_temp_topk_prob", "C >= 1")
    refused(topk(ld=7), "egk_temp_topk_prob", "ld >= C")
    refused(topk(k=0), "egk_temp_topk_prob", "k in 1 .. 64")
    refused(topk(k=65, istride=65, pstride=65), "egk_temp_topk_prob", "k in 1 .. 64")
    refused(topk(istride=4), "egk_temp_topk_prob", "idx row stride")
    refused(topk(pstride=4), "egk_temp_topk_prob", "prob row stride")
    refused(topk(idx=U4), "egk_temp_topk_prob", "misaligned idx")
    refused(topk(lse=U2), "egk_temp_topk_prob", "misaligned", "lse")
    refused(topk(dt=9), "egk_temp_topk_prob", "dtype")
    assert topk(rows=0) == 0

    scale = lambda logits=A, ld=8, rows=4, C=8, beta=A, out=A, ldo=8, dt=F32: lib.egk_temp_scale_rows(None, logits, ld, rows, C, beta, out, ldo, dt)
    for kw, arg in ((dict(logits=None), "logits"), (dict(beta=None), "beta"), (dict(out=None), "out")):
        refused(scale(**kw), "egk_temp_scale_rows", "null pointer", arg)
    refused(scale(rows=-1), "egk_temp_scale_rows", "rows")
    refused(scale(C=0), "egk_temp_scale_rows", "C >= 1")
    refused(scale(ld=7), "egk_temp_scale_rows", "ld >= C")
    refused(scale(ldo=7), "egk_temp_scale_rows", "ldo >= C")
    refused(scale(out=U2), "egk_temp_scale_rows", "misaligned", "out")
    refused(scale(dt=-1), "egk_temp_scale_rows", "dtype")
    assert scale(rows=0) == 0


def test_the_launches_have_their_profile_ids():
    lib = _lib.load()
    names = []
    for i in range(lib.egk_prof_count()):
        name = ctypes.create_string_buffer(64)
        n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert all(n in names for n in ("temp_stats", "temp_newton", "temp_topk_prob", "temp_scale_rows")) and len(set(names)) == len(names)


# ---- 4. the configuration ---------------------------------------------------------------------------------------------------------------
def test_calibration_config_accepts_and_rejects_as_documented():
    from egopack_amd import calibration as CAL
    from egopack_amd import train as T
    cfg = T.load_config([])
    assert dict(cfg.calibration) == {"mode": "none", "tasks": ["ar", "lta", "oscc"], "t_range": [0.05, 20.0], "iterations": 16,
                                     "stop": 1e-6, "max_rows": 1048576, "save": True, "predict": "auto"} == CAL.DEFAULTS
    cal = T.calibration_config(cfg)
    assert cal["enabled"] is False and cal["predict"] == "auto" and T.calibration_meter_args(cfg, "ar") == {}
    assert T.calibration_config({})["mode"] == "none"  # (a config without the block: the defaults)
    cfg = T.load_config(["calibration.mode=Temperature", "calibration.tasks=[ar]", "calibration.predict=false", "calibration.iterations=8"])
    cal = T.calibration_config(cfg)
    assert cal["enabled"] and cal["mode"] == "temperature" and cal["predict"] == "false" and cal["iterations"] == 8
    assert T.calibration_meter_args(cfg, "ar") == {"calibration": {"t_range": [0.05, 20.0], "iterations": 8, "stop": 1e-6, "max_rows": 1048576}}
    assert T.calibration_meter_args(cfg, "lta") == {} and T.calibration_meter_args(cfg, "pnr") == {}
    for bad, needle in ((["+calibration.bins=15"], "bins"), (["calibration.mode=platt"], "platt"), (["calibration.tasks=[ar,pnr]"], "pnr"),
                        (["calibration.t_range=[2.0,20.0]"], "t_range"), (["calibration.t_range=[0.0,20.0]"], "t_range"),
                        (["calibration.t_range=[0.05]"], "t_range"), (["calibration.iterations=0"], "iterations"),
                        (["calibration.stop=-1"], "stop"), (["calibration.max_rows=0"], "max_rows"), (["calibration.predict=maybe"], "maybe")):
        with pytest.raises(ValueError) as e:
            T.calibration_config(T.load_config(bad))
        assert needle in str(e.value), (bad, str(e.value))


def test_save_and_load_calibration_round_trip(tmp_path):
    import logging
    from egopack_amd import train as T
    fits = {"ar": {"verbs_": dict(temperature=1.5, beta=1 / 1.5, status="converged", iterations=5, rows=10, left_out=0, nll=2.0, nll_calibrated=1.9),
                   "nouns_": dict(temperature=0.8, beta=1.25, status="converged", iterations=4, rows=10, left_out=0, nll=3.0, nll_calibrated=2.9)}}
    off = T.load_config([])
    assert T.save_calibration(logging.getLogger("t"), off, tmp_path, fits) == [] and not list(tmp_path.iterdir())  # (mode none: nothing)
    assert T.load_calibration(off, tmp_path, "ar") is None  # (auto, no file)
    with pytest.raises(FileNotFoundError):
        T.load_calibration(T.load_config(["calibration.predict=true"]), tmp_path, "ar")
    on = T.load_config(["calibration.mode=temperature"])
    assert T.save_calibration(logging.getLogger("t"), on, tmp_path, fits) == [tmp_path / "calibration_ar.pt"]
    blob = T.load_calibration(off, tmp_path, "ar")
    assert blob["heads"] == fits["ar"] and blob["t_range"] == [0.05, 20.0] and blob["split"] == "validation" and blob["task"] == "ar"
    assert T.load_calibration(T.load_config(["calibration.predict=false"]), tmp_path, "ar") is None
    (tmp_path / "calibration_lta.pt").write_bytes((tmp_path / "calibration_ar.pt").read_bytes())
    with pytest.raises(ValueError, match="not a calibration file of task lta"):
        T.load_calibration(off, tmp_path, "lta")
    from egopack_amd import predict as P
    assert P.temperatures(None) == {} and P.temperatures(blob) == {"temperature": {"verbs": 1.5, "nouns": 0.8}}


def test_the_sampler_refuses_a_temperature_that_is_no_finite_positive_number():
    from egopack_amd.ops import FutureSampler
    assert FutureSampler(3).temperature == 1.0 and FutureSampler(3, 2.0).temperature == 2.0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            FutureSampler(0, bad)


# ---- 5. the meters with ``mode: none`` ----------------------------------------------------------------------------------------------------
def test_a_meter_without_calibration_holds_no_state_and_adds_no_key():
    from egopack_amd import meters as M

    class DS:
        label_names = ["verbs", "nouns"]
        class_labels = [[f"v{i}" for i in range(5)], [f"n{i}" for i in range(7)]]

    for task, cls in (("ar", M.RecognitionMeter), ("anticipation", M.AnticipationMeter), ("lta", M.LTAMeter), ("oscc", M.OSCCMeter)):
        DS.task = task
        m = M.build_meter_for_dataset(DS(), device="cpu")
        assert isinstance(m, cls) and m.temp_store is None and m.temp_cfg is None and m.temperature_fit() == {}
        keys = set(m.get_logs())
        assert not any("temperature" in k or "nll" in k or "_calibrated" in k or "in_sample" in k for k in keys), (task, sorted(keys))
        assert not any("temperature" in line for line in m.print_logs())
    DS.task = "pnr"
    assert M.build_meter_for_dataset(DS(), device="cpu", calibration={"max_rows": 8}).temp_store is None  # (PNR takes none)


# ---- 6. the measurement that fixes the tolerances -------------------------------------------------------------------------------------------
def test_the_f32_restatement_fixes_the_tolerances():
    """The worst error of a plain f32 restatement of the row arithmetic against float64, over the statistics test's inputs: the
    figures calibration_common.TOL is 4 x of.  They must hold (the tolerance would else be too tight to be the reference's own error)
    and must not be padded (more than twice the measurement)."""
    worst = CM.measure_f32_error(CM.stats_family())
    print("f32 restatement, worst relative error (nll, d1, d2):", worst)
    for got, pinned in zip(worst, CM.F32_MEASURED):
        assert pinned / 2 < got <= pinned, (worst, CM.F32_MEASURED)
    assert CM.TOL == tuple(4.0 * v for v in CM.F32_MEASURED)
