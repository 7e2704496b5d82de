"""Task weighting without a GPU: what include/egopack_task_scale.h pins beyond the one ledger (tests/test_cabi.py), the host-side
refusals of its entry points, the ``task_weighting:`` config block, the float64 host model of tests/task_weighting_common.py against
torch autograd, ``train.build_optimizer`` with the log-variances, the checkpoint entry, and the refusals of the EgoPack step and the
sharded update."""
import ctypes
import logging

import numpy as np
import pytest
import torch

from tests import task_weighting_common as TW

# ---- 1. include/egopack_task_scale.h beyond the common ledger --------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_every_seeded_sibling_has_its_s_form():
    from egopack_amd import _lib
    lib, declared = _lib.load(), _lib.declared("task_scale")
    for sib in ("egk_ce_fused_multi", "egk_ce_w_fused_multi", "egk_rowdot_bce", "egk_rowdot_bce_w", "egk_rowdot_ce2", "egk_rowdot_ce2_multi"):
        assert sib + "_s" in declared and hasattr(lib, sib)


def test_the_task_scale_coverage_check_fails_for_an_entry_point_without_a_case():
    from tests import cabi_common as CC
    assert CC.uncovered("task_scale") == set() and CC.uncovered("task_scale", {"egk_task_scale_not_there"}) == {"egk_task_scale_not_there"}


def test_task_scale_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert {"task_scale", "bce_balanced", "ce_balanced", "ce_fwd", "bce_fwd", "sum_scale"} <= set(names) and len(set(names)) == len(names)


# ---- 2. host-side refusals (small fake non-null pointers: every check precedes the first dereference and the first launch) ---------
P = 0x1000


def _refused(rc, entry, needle):
    from egopack_amd import _lib
    assert rc == -1 and needle in _lib.last_error() and entry in _lib.last_error(), (rc, _lib.last_error())


def test_scaled_row_heads_refuse_what_their_siblings_refuse_and_a_null_scale():
    from egopack_amd import _lib
    lib = _lib.load()

    def bce(f=P, w=P, y=P, lg=P, ls=P, df=None, ws=None, rows=8, cols=64, scale=P, dtype=0):
        return lib.egk_rowdot_bce_s(None, f, w, None, y, lg, ls, df, ws, rows, cols, 0.1, scale, dtype)

    def bce_w(f=P, w=P, y=P, lg=P, ls=P, df=None, ws=None, rows=8, cols=64, scale=P, pos=3.0, neg=0.5, gamma=2.0, dtype=0):
        return lib.egk_rowdot_bce_w_s(None, f, w, None, y, lg, ls, df, ws, rows, cols, 0.1, scale, pos, neg, gamma, dtype)

    for call, name in ((bce, "egk_rowdot_bce_s"), (bce_w, "egk_rowdot_bce_w_s")):
        for k in ("f", "w", "y", "lg", "ls"):
            _refused(call(**{k: None}), name, "null pointer")
        _refused(call(scale=None), name, "null pointer (scale)")
        _refused(call(scale=None, rows=0), name, "null pointer (scale)")
        _refused(call(scale=P + 2), name, "not 4-byte aligned")
        _refused(call(df=P), name, "gradients need the partial-row workspace")
        _refused(call(f=P + 2), name, "unaligned pointer")
        assert call(rows=0) == 0
    _refused(bce_w(pos=-1.0), "egk_rowdot_bce_w_s", "must be finite and >= 0")
    _refused(bce_w(rows=-1), "egk_rowdot_bce_w_s", "rows must be >= 0")

    def ce2(f=P, w=P, y=P, lg=P, ls=P, df=None, dw=None, rows=8, cols=64, scale=P):
        return lib.egk_rowdot_ce2_s(None, f, w, None, y, lg, ls, df, dw, None, None, rows, cols, 0.0, 0.1, scale, 0)
    for k in ("f", "w", "y", "lg", "ls"):
        _refused(ce2(**{k: None}), "egk_rowdot_ce2_s", "null pointer")
    _refused(ce2(df=P), "egk_rowdot_ce2_s", "gradients need dw")
    _refused(ce2(scale=None), "egk_rowdot_ce2_multi_s", "null pointer (scale)")
    _refused(ce2(rows=257), "egk_rowdot_ce2_multi_s", "at most 256 rows")
    _refused(ce2(df=P, dw=P), "egk_rowdot_ce2_multi_s", "gradients need the [rows][2] workspace")
    assert ce2(rows=0) == 0
    arr = (ctypes.c_void_p * 1)(P)
    _refused(lib.egk_rowdot_ce2_multi_s(None, 5, arr, arr, None, P, P, P, None, None, None, None, 8, 64, 0, 0.0, 0.1, P, 0),
             "egk_rowdot_ce2_multi_s", "1 .. 4 sources")


def test_scaled_fused_cross_entropy_refuses_what_its_sibling_refuses_and_null_scales():
    from egopack_amd import _lib
    lib = _lib.load()

    def task(t, rows=8):
        t.logits[0], t.ld[0], t.C[0], t.pad[0], t.dcol[0] = P, 8, 5, 8, 0
        t.n_heads, t.y, t.y_stride, t.loss, t.dlogits, t.ldd, t.rows, t.gscale = 1, P, 1, P, P, 8, rows, 0.1
    plain, bal = (_lib.CETask * 1)(), (_lib.CEWTask * 1)()
    task(plain[0], 0), task(bal[0].base, 0)
    sc = (ctypes.c_void_p * 1)(P)
    for fn, arr, name in ((lib.egk_ce_fused_multi_s, plain, "egk_ce_fused_multi_s"), (lib.egk_ce_w_fused_multi_s, bal, "egk_ce_w_fused_multi_s")):
        assert fn(None, arr, sc, 1, 0.0, 0) == 0                       # no row in any task: nothing is launched
        _refused(fn(None, None, sc, 1, 0.0, 0), name, "null pointer")
        _refused(fn(None, arr, None, 1, 0.0, 0), name, "null pointer (scales)")
        _refused(fn(None, arr, (ctypes.c_void_p * 1)(None), 1, 0.0, 0), name, "null pointer (scale of task 0)")
        _refused(fn(None, arr, (ctypes.c_void_p * 1)(P + 1), 1, 0.0, 0), name, "not 4-byte aligned")
        _refused(fn(None, arr, sc, 5, 0.0, 0), name, "1 .. 4 tasks")
        _refused(fn(None, arr, sc, 1, 0.0, 2), name, "unknown activation dtype")
    plain[0].pad[0] = 4
    _refused(lib.egk_ce_fused_multi_s(None, plain, sc, 1, 0.0, 0), "egk_ce_fused_multi_s", "pad must be >= C")
    bal[0].weight[0] = P + 2
    _refused(lib.egk_ce_w_fused_multi_s(None, bal, sc, 1, 0.0, 0), "egk_ce_w_fused_multi_s", "misaligned vector pointer")


def test_prepare_grad_and_fill_refuse_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()
    _refused(lib.egk_task_scale_prepare(None, None, P, 3), "egk_task_scale_prepare", "null pointer")
    _refused(lib.egk_task_scale_prepare(None, P, None, 3), "egk_task_scale_prepare", "null pointer")
    for n in (0, 9, -1):
        _refused(lib.egk_task_scale_prepare(None, P, P, n), "egk_task_scale_prepare", "1..8 tasks")
    _refused(lib.egk_task_scale_prepare(None, P + 2, P, 3), "egk_task_scale_prepare", "4-byte aligned")
    xs, ns, cn, w = (ctypes.c_void_p * 2)(P, None), (ctypes.c_int64 * 2)(8, 0), (ctypes.c_int64 * 2)(0, 0), (ctypes.c_float * 2)(1.0, 0.5)

    def grad(xs=xs, ns=ns, cn=cn, w=w, s=P, scale=P, ds=P, obj=P, acc=P, n=2):
        return lib.egk_task_scale_grad(None, xs, ns, cn, w, s, scale, ds, obj, acc, n)
    for k in ("xs", "ns", "cn", "w", "scale", "obj"):
        _refused(grad(**{k: None}), "egk_task_scale_grad", "null pointer")
    _refused(grad(ds=None), "egk_task_scale_grad", "null pointer (ds")
    for n in (0, 9):
        _refused(grad(n=n), "egk_task_scale_grad", "1..8 tasks")
    _refused(grad(ns=(ctypes.c_int64 * 2)(8, -1)), "egk_task_scale_grad", "negative length")
    _refused(grad(acc=P + 4), "egk_task_scale_grad", "misaligned pointer")
    _refused(grad(xs=(ctypes.c_void_p * 2)(P + 2, None)), "egk_task_scale_grad", "misaligned loss vector")
    _refused(lib.egk_fill_scaled_from(None, None, 4, 0.5, P), "egk_fill_scaled_from", "null pointer")
    _refused(lib.egk_fill_scaled_from(None, P, 4, 0.5, None), "egk_fill_scaled_from", "null pointer")
    _refused(lib.egk_fill_scaled_from(None, P, -4, 0.5, P), "egk_fill_scaled_from", "n must be >= 0")
    _refused(lib.egk_fill_scaled_from(None, P, 4, 0.5, P + 2), "egk_fill_scaled_from", "4-byte aligned")
    assert lib.egk_fill_scaled_from(None, P, 0, 0.5, P) == 0


# ---- 3. the config block -------------------------------------------------------------------------------------------------------------
def test_config_defaults_parsing_and_refusals():
    from egopack_amd import train as T
    assert T.task_weighting_config(T.load_config([])) == {"mode": "none", "lr_scale": 1.0}
    assert T.task_weighting_config({}) == {"mode": "none", "lr_scale": 1.0}
    cfg = T.load_config(["task_weighting.mode=Uncertainty", "task_weighting.lr_scale=10"])
    assert T.task_weighting_config(cfg) == {"mode": "uncertainty", "lr_scale": 10.0}
    assert T.task_weighting_config({"task_weighting": {"mode": "manual"}})["mode"] == "manual"
    with pytest.raises(ValueError, match=r"unknown key\(s\) \['decay'\] \(mode, lr_scale\)"):
        T.task_weighting_config({"task_weighting": {"mode": "manual", "decay": 0.9}})
    with pytest.raises(ValueError, match=r"unknown mode 'gradnorm' \(none \| manual \| uncertainty\)"):
        T.task_weighting_config({"task_weighting": {"mode": "gradnorm"}})
    for bad in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="lr_scale"):
            T.task_weighting_config({"task_weighting": {"mode": "uncertainty", "lr_scale": bad}})
    assert T.build_task_weighting(T.load_config([]), ["ar", "lta"]) is None
    assert T.build_task_weighting(T.load_config(["task_weighting.mode=manual"]), ["ar", "lta"]) is None
    lv = T.build_task_weighting(cfg, ["ar", "lta", "pnr"])
    assert lv.tasks == ("ar", "lta", "pnr") and lv.log_var.dtype == torch.float32 and lv.log_var.tolist() == [0.0, 0.0, 0.0]
    assert list(lv.state_dict()) == ["log_var"]


# ---- 4. the host model against autograd ------------------------------------------------------------------------------------------------
def test_host_model_matches_autograd_in_float64():
    g = torch.Generator().manual_seed(3)
    vecs = [torch.rand(1, generator=g) * 3, torch.rand(70, generator=g) * 3, torch.rand(2048, generator=g) * 3]
    counts = [None, 140, None]
    w = [1.0, 0.5, 2.0]
    for s32 in ([0.0, 0.0, 0.0], [0.3, -0.7, 1e-3], [3.0, -3.0, 0.5]):
        s32 = [TW.fl32(v) for v in s32]
        L = torch.tensor(TW.means(vecs, counts), dtype=torch.float64)
        s = torch.tensor(s32, dtype=torch.float64, requires_grad=True)
        J = TW.autograd_objective(L, torch.tensor(w, dtype=torch.float64), s)
        J.backward()
        # the model with the exact float64 scales is autograd's J and gradient ...
        Jm, ds, sums = TW.objective(vecs, w, [float(np.exp(-np.float64(v))) for v in s32], s32, counts)
        torch.testing.assert_close(torch.tensor(Jm, dtype=torch.float64), J.detach(), rtol=1e-13, atol=0)
        torch.testing.assert_close(torch.tensor(ds, dtype=torch.float64), s.grad, rtol=1e-12, atol=1e-14)
        assert sums == [float(v.double().sum()) for v in vecs]
        # ... and with the f32 scales the kernels read (exp(-s) rounded once) it moves by at most half an f32 ulp of each scale
        J32, ds32, _ = TW.objective(vecs, w, [TW.prepared_scale(v) for v in s32], s32, counts)
        assert abs(J32 - Jm) <= 6e-8 * sum(abs(wt) * float(np.exp(-np.float64(v))) * Lt for wt, v, Lt in zip(w, s32, L.tolist()))
        for t in range(3):
            assert abs(ds32[t] - ds[t]) <= 6e-8 * w[t] * float(np.exp(-np.float64(s32[t]))) * float(L[t])
    # s = 0: scale exactly 1, the fixed-weight objective and dJ/ds = w (1 - L)
    J0, ds0, _ = TW.objective(vecs, w, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], counts)
    L = TW.means(vecs, counts)
    assert J0 == sum(wt * Lt for wt, Lt in zip(w, L)) and ds0 == [wt * (1.0 - Lt) for wt, Lt in zip(w, L)]
    assert TW.prepared_scale(0.0) == 1.0 and TW.scaled_seed(0.37, 1.0) == TW.fl32(0.37)
    # absent tasks add nothing; fixed scales have no gradient
    Jm, ds, sums = TW.objective([vecs[0], None, vecs[2]], w, [1.0, 0.5, 2.0], None)
    assert ds is None and sums[1] == 0.0 and Jm == w[0] * L[0] + w[2] * 2.0 * L[2]
    # the Adam rule of the first step: -lr sign(g) up to the f32 hyperparameters (6.5e-6) and eps
    for g in (-7.23, 0.375, 1e-3):
        got = TW.adam_first_step(g, 1e-2)
        assert got * g < 0 and abs(abs(got) / 1e-2 - 1.0) < 1e-5 and abs(abs(got) / 1e-2 - 1.0) > 1e-6
        assert TW.adam_first_step(-g, 1e-2) == -got
    # the scaled seed is ONE f32 product
    for c in (2.0 / 70, 0.37 / 13):
        for sc in TW.SCALES:
            assert TW.scaled_seed(c, sc) == float(np.float32(np.float32(c) * np.float32(sc)))
    assert TW.scaled_seed(2.0 / 70, 0.5) == TW.fl32(1.0 / 70)


# ---- 5. the optimizer ---------------------------------------------------------------------------------------------------------------------
def _modules():
    torch.manual_seed(0)
    model = torch.nn.Linear(8, 8)
    heads = torch.nn.Linear(8, 3)
    return [*model.parameters(), *heads.parameters()]


def test_build_optimizer_puts_log_var_last_in_a_group_of_its_own():
    from egopack_amd import train as T
    cfg = T.load_config(["task_weighting.mode=uncertainty", "task_weighting.lr_scale=5", "optimizer.lr=1e-3", "optimizer.weight_decay=1e-4"])
    lv = T.build_task_weighting(cfg, ["ar", "lta", "pnr"])
    params = _modules()
    opt = T.build_optimizer(cfg, params, log_var=lv)
    assert [g.get("name") for g in opt.param_groups] == ["all", "task_weighting"]
    last = opt.param_groups[-1]
    assert len(last["params"]) == 1 and last["params"][0] is lv.log_var and last["weight_decay"] == 0.0
    assert last["lr"] == pytest.approx(5e-3) and opt.param_groups[0]["lr"] == pytest.approx(1e-3)
    assert opt.param_groups[0]["weight_decay"] == pytest.approx(1e-4)
    assert opt._all_params()[-1] is lv.log_var and opt.layout_order[-1] is lv.log_var
    assert [id(p) for p in opt._all_params()[:-1]] == [id(p) for p in params]
    # with the groups of ``param_groups``: appended behind them, the layout order runs on
    groups = [{"params": params[:2], "name": "a", "lr": 1e-3, "weight_decay": 1e-4}, {"params": params[2:], "name": "b", "lr": 2e-3, "weight_decay": 0.0}]
    opt2 = T.build_optimizer(cfg, groups, layout_order=params, log_var=lv)
    assert [g["name"] for g in opt2.param_groups] == ["a", "b", "task_weighting"] and opt2.layout_order[-1] is lv.log_var
    assert [id(p) for p in opt2.layout_order[:-1]] == [id(p) for p in params]
    # without log_var nothing changes: one group, no layout order
    opt3 = T.build_optimizer(T.load_config([]), _modules())
    assert len(opt3.param_groups) == 1 and opt3.layout_order is None and opt3.task_weighting == "none"
    # the slot follows every other slot once the flat buffers would be laid out
    for p in (*params, lv.log_var):
        p.grad = torch.zeros_like(p)
    segs = opt.group_segments()
    assert segs[-1][2] == 1 and segs[-1][1] - segs[-1][0] == 8 and len(segs) == 2


def test_an_optimizer_state_without_the_task_weighting_group_loads_with_fresh_moments():
    """A fixed-weight run's optimizer state (one group fewer, the last index missing) loads into the optimizer of an uncertainty
    run; any other difference in the groups is torch's error."""
    from egopack_amd import train as T
    cfg = T.load_config(["task_weighting.mode=uncertainty", "optimizer.lr=1e-3"])
    params = _modules()
    old = T.build_optimizer(T.load_config(["optimizer.lr=5e-4"]), params)
    sd = old.state_dict()
    sd["state"] = {i: {"step": torch.tensor(7.0), "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)} for i, p in enumerate(params)}
    lv = T.build_task_weighting(cfg, ["ar", "lta", "pnr"])
    new = T.build_optimizer(cfg, params, log_var=lv)
    new.load_state_dict(sd)
    assert new.step_count == 7 and new.param_groups[0]["lr"] == pytest.approx(5e-4)     # (the loaded group's hyper-parameters)
    assert new.param_groups[-1]["name"] == "task_weighting" and new.param_groups[-1]["lr"] == pytest.approx(1e-3)
    assert sorted(new._pending_state["state"]) == list(range(len(params)))              # (no entry for log_var: fresh moments)
    # saved again at once, before any step: the state carries THIS optimizer's two groups and loads back into its like
    again = new.state_dict()
    assert [g.get("name") for g in again["param_groups"]] == ["all", "task_weighting"] and again["param_groups"][-1]["params"] == [len(params)]
    assert again["param_groups"][0]["lr"] == pytest.approx(5e-4) and sorted(again["state"]) == list(range(len(params)))
    T.build_optimizer(cfg, params, log_var=lv).load_state_dict(again)
    # not the trailing task_weighting group: refused as before
    other = T.build_optimizer(cfg, [{"params": params[:2], "name": "a"}, {"params": params[2:], "name": "b"}])
    with pytest.raises(ValueError, match="different number of parameter groups"):
        other.load_state_dict(sd)
    short = {**sd, "param_groups": [{**sd["param_groups"][0], "params": sd["param_groups"][0]["params"][:-1]}]}
    with pytest.raises(ValueError, match="different number of parameter groups"):
        new.load_state_dict(short)
    with pytest.raises(ValueError, match="different number of parameter groups"):
        old.load_state_dict(T.build_optimizer(cfg, params, log_var=lv).state_dict())  # (the other way round: two groups into one)


# ---- 6. the checkpoint entry ----------------------------------------------------------------------------------------------------------
class _Step:
    def __init__(self, mode, enabled=("ar", "lta", "pnr")):
        from egopack_amd.models import TaskLogVariance
        self.task_mode, self.enabled, self.weights = mode, list(enabled), {t: 1.0 for t in enabled}
        self.task_log_var = TaskLogVariance(enabled) if mode == "uncertainty" else None
        self.scales = {t: 1.0 for t in enabled}

    def task_scales(self):
        return dict(self.scales)

    def set_task_scale(self, d):
        self.scales.update(d)


def test_checkpoint_entry_round_trip(tmp_path, caplog):
    from egopack_amd import train as T
    log = logging.getLogger("task_weighting_test")
    cfg = T.load_config(["task_weighting.mode=uncertainty"])
    a = _Step("uncertainty")
    with torch.no_grad():
        a.task_log_var.log_var.copy_(torch.tensor([0.25, -0.5, 1e-3]))
    st = T.task_weighting_state(cfg, a)
    assert st["config"] == {"mode": "uncertainty", "lr_scale": 1.0} and st["tasks"] == ["ar", "lta", "pnr"]
    assert st["log_var"].dtype == torch.float32 and st["log_var"].device.type == "cpu" and "scales" not in st
    torch.save({"task_weighting": st}, tmp_path / "c.pth")
    ck = torch.load(tmp_path / "c.pth", weights_only=False)
    b = _Step("uncertainty")
    assert T.load_task_weighting(log, ck, b) and torch.equal(b.task_log_var.log_var.detach(), a.task_log_var.log_var.detach())
    # a checkpoint without the entry (or of other tasks): s = 0 and ONE log line
    for other in ({}, {"task_weighting": {**st, "tasks": ["ar", "pnr"]}}):
        c = _Step("uncertainty")
        with caplog.at_level(logging.INFO):
            caplog.clear()
            assert not T.load_task_weighting(log, other, c)
        assert c.task_log_var.log_var.tolist() == [0.0, 0.0, 0.0]
        assert sum("starting from s = 0" in r.getMessage() for r in caplog.records) == 1
    # manual: the scales
    m = _Step("manual")
    m.set_task_scale({"lta": 0.5, "pnr": 2.0})
    sm = T.task_weighting_state(T.load_config(["task_weighting.mode=manual"]), m)
    assert sm["scales"].tolist() == [1.0, 0.5, 2.0] and "log_var" not in sm
    m2 = _Step("manual")
    assert T.load_task_weighting(log, {"task_weighting": sm}, m2) and m2.task_scales() == {"ar": 1.0, "lta": 0.5, "pnr": 2.0}
    # off: no entry, nothing loaded
    assert T.task_weighting_state(T.load_config([]), _Step("none")) is None and not T.load_task_weighting(log, ck, _Step("none"))
    # the module's state is not part of any reference key
    from egopack_amd.models import TaskLogVariance
    assert list(TaskLogVariance(["ar"]).state_dict()) == ["log_var"]
    with pytest.raises(ValueError, match="no enabled task"):
        TaskLogVariance([])


# ---- 7. refusals above the kernels ---------------------------------------------------------------------------------------------------
def test_egopack_step_refuses_task_weighting_by_name():
    from egopack_amd import engine
    for mode in ("manual", "uncertainty"):
        with pytest.raises(ValueError, match="ONE primary task"):
            engine.EgoPackStep(None, {}, None, {}, None, task_weighting=mode)


def test_mtl_step_refuses_bad_modes_and_a_foreign_log_var():
    from egopack_amd import engine
    from egopack_amd.models import TaskLogVariance
    from egopack_amd.optim import FlatAdam
    tasks = {"ar": torch.nn.Linear(4, 4), "pnr": torch.nn.Linear(4, 1)}
    weights = {"ar": 1.0, "oscc": 0.0, "lta": 0.0, "pnr": 2.0}
    params = [p for t in tasks.values() for p in t.parameters()]
    opt = FlatAdam(params)
    mk = lambda **kw: engine.MTLStep(torch.nn.Linear(4, 4), tasks, {}, weights, kw.pop("opt", opt), **kw)
    with pytest.raises(ValueError, match=r"unknown mode 'pcgrad' \(none \| manual \| uncertainty\)"):
        mk(task_weighting="pcgrad")
    with pytest.raises(ValueError, match="log_var must be a TaskLogVariance over the enabled tasks"):
        mk(task_weighting="uncertainty")
    with pytest.raises(ValueError, match="log_var must be a TaskLogVariance over the enabled tasks"):
        mk(task_weighting="uncertainty", log_var=TaskLogVariance(["ar", "lta"]))
    lv = TaskLogVariance(["ar", "pnr"])
    with pytest.raises(ValueError, match="not a parameter of the optimizer"):
        mk(task_weighting="uncertainty", log_var=lv)
    with pytest.raises(ValueError, match="log_var is for the uncertainty mode"):
        mk(task_weighting="manual", log_var=lv)
    step = mk(task_weighting="uncertainty", log_var=lv, opt=FlatAdam([{"params": params}, {"params": [lv.log_var], "weight_decay": 0.0}]))
    assert step.task_mode == "uncertainty" and step.optimizer.task_weighting == "uncertainty" and step.task_scale is None and step.captures == 0
    with pytest.raises(ValueError, match="manual sets scales from the host"):
        step.set_task_scale({"ar": 2.0})
    man = mk(task_weighting="manual")
    man.set_task_scale({"pnr": 0.25})                                  # (before the first step: kept on the host)
    assert man.task_scales() == {"ar": 1.0, "pnr": 0.25}
    with pytest.raises(ValueError, match="not among the enabled tasks"):
        man.set_task_scale({"lta": 2.0})
    off = mk()
    assert off.task_mode == "none" and off.task_scale is None and off.task_scales() == {"ar": 1.0, "pnr": 1.0}


def test_sharded_update_refuses_task_weighting_by_name():
    from egopack_amd.dist import GradSync
    from egopack_amd.optim import FlatAdam
    opt = FlatAdam([torch.randn(64).requires_grad_(True)])
    sync = GradSync(2, shard_update=True)
    for mode in ("uncertainty", "manual"):
        opt.task_weighting = mode
        for call in (lambda: sync._sharded_step(opt), lambda: sync.start(opt, 0, 8)):
            with pytest.raises(ValueError, match=rf"task weighting \(task_weighting.mode: {mode}\) does not combine with the sharded update"):
                call()
