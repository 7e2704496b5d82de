"""Parameter groups without a GPU: train.build_param_groups, the constructors' refusals, the host-side segment table, what
include/egopack_optim_groups.h pins beyond the one ledger (tests/test_cabi.py), the host-side refusals of egk_optim_step_groups, the
state dicts against the torch classes over the same groups, schedulers over two groups."""
import ctypes

import pytest
import torch

SHAPES = [(33, 7), (5,), (64, 64), (3,), (130, 9)]


def _params(seed=0, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]


def _three_groups(p, **extra):
    return [{"params": [p[0], p[2]], "lr": 1e-2, "weight_decay": 1e-2}, {"params": [p[1], p[3]], "lr": 1e-2, "weight_decay": 0.0},
            {"params": [p[4]], "lr": 1e-3, "weight_decay": 1e-2, **extra}]


# ---- 1. train.build_param_groups ---------------------------------------------------------------------------------------------------
class _Module(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.lin = torch.nn.Linear(6, 4)
        self.norm = torch.nn.LayerNorm(4)

    def configure_optimizers(self, _):
        return list(self.parameters())


def _modules():
    model = _Module(0)
    tasks = {t: _Module(i + 1) for i, t in enumerate(("ar", "oscc", "lta", "pnr"))}
    return model, tasks, _Module(9)


def _main_list(model, tasks, graphone=None):
    """The list main_temporal.py / main_egopack.py have always built."""
    out = [*model.configure_optimizers(0), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].configure_optimizers(0))]
    return out + (list(graphone.parameters()) if graphone is not None else [])


def test_default_param_groups_are_the_flat_list():
    from egopack_amd import train as T
    model, tasks, graphone = _modules()
    cfg = T.load_config([])
    assert dict(cfg.param_groups) == {"no_decay_1d": False, "lr_scale": {}} and "param_groups" not in cfg.optimizer
    for g1 in (None, graphone):
        got, want = T.build_param_groups(cfg, model, tasks, g1), _main_list(model, tasks, g1)
        assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    # factors of 1.0 change nothing either
    cfg = T.load_config(["param_groups.lr_scale.tasks=1.0"])
    got = T.build_param_groups(cfg, model, tasks)
    assert all(a is b for a, b in zip(got, _main_list(model, tasks)))
    opt = T.build_optimizer(cfg, got, layout_order=_main_list(model, tasks))
    assert len(opt.param_groups) == 1 and not opt.grouped and opt.layout_order is None


def test_no_decay_1d_takes_exactly_the_vectors():
    from egopack_amd import train as T
    model, tasks, _ = _modules()
    cfg = T.load_config(["optimizer._target_=torch.optim.AdamW", "optimizer.weight_decay=1e-2", "param_groups.no_decay_1d=true"])
    groups = T.build_param_groups(cfg, model, tasks)
    flat = _main_list(model, tasks)
    assert [g["name"] for g in groups] == ["all", "all/no_decay"] and [g["weight_decay"] for g in groups] == [1e-2, 0.0]
    assert {id(p) for p in groups[1]["params"]} == {id(p) for p in flat if p.dim() <= 1}
    assert {id(p) for p in groups[0]["params"]} == {id(p) for p in flat if p.dim() > 1}
    assert all(g["lr"] == 1e-5 for g in groups)
    opt = T.build_optimizer(cfg, groups, layout_order=flat)
    assert opt.grouped and [g["weight_decay"] for g in opt.param_groups] == [1e-2, 0.0]
    # the flat layout is the ungrouped one: weight and vector slots alternate, one segment per run of equal group
    for p in flat:
        p.grad = torch.zeros_like(p)
    segs = opt.group_segments()
    plain = T.build_optimizer(T.load_config([]), flat)
    assert [id(p) for p in opt._layout(opt._live())[0]] == [id(p) for p in plain._layout(plain._live())[0]]
    assert [s[2] for s in segs] == [0, 1] * 5 and segs[0][:2] == (0, 384) and segs[1][:2] == (384, 408)  # (4 x 6 -> 64 rows; three vectors of 4 -> 8)
    assert plain.group_segments() == [(0, segs[-1][1], 0)]


def test_lr_scale_keys_map_to_the_modules():
    from egopack_amd import train as T
    model, tasks, graphone = _modules()
    over = ["optimizer.lr=1e-3", "param_groups.lr_scale.temporal_graph=0.1", "param_groups.lr_scale.graphone=2"]
    groups = T.build_param_groups(T.load_config(over), model, tasks, graphone)
    assert [g["name"] for g in groups] == ["temporal_graph", "tasks", "graphone"]
    assert [g["lr"] for g in groups] == pytest.approx([1e-4, 1e-3, 2e-3], rel=1e-12)
    assert [id(p) for p in groups[0]["params"]] == [id(p) for p in model.parameters()]
    assert [id(p) for p in groups[1]["params"]] == [id(p) for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].parameters()]
    assert [id(p) for p in groups[2]["params"]] == [id(p) for p in graphone.parameters()]
    assert all(g["weight_decay"] == 1e-5 for g in groups)
    # with no_decay_1d: module x decays-or-not, at most six; a module without parameters gives no group
    groups = T.build_param_groups(T.load_config(over + ["param_groups.no_decay_1d=true"]), model, tasks, graphone)
    assert [g["name"] for g in groups] == ["temporal_graph", "temporal_graph/no_decay", "tasks", "tasks/no_decay", "graphone", "graphone/no_decay"]
    groups = T.build_param_groups(T.load_config(over + ["param_groups.no_decay_1d=true"]), model, tasks)
    assert len(groups) == 4 and all(g["params"] for g in groups)
    seen = [id(p) for g in groups for p in g["params"]]
    assert sorted(seen) == sorted(id(p) for p in _main_list(model, tasks))


def test_unknown_param_group_keys_raise():
    from egopack_amd import train as T
    model, tasks, _ = _modules()
    with pytest.raises(ValueError, match="backbone"):
        T.build_param_groups(T.load_config(["param_groups.lr_scale.backbone=0.1"]), model, tasks)
    with pytest.raises(ValueError, match="no_decay_2d"):
        T.build_param_groups(T.load_config(["+param_groups.no_decay_2d=true"]), model, tasks)


def test_param_groups_are_logged_one_line_each(caplog):
    import logging
    from egopack_amd import train as T
    model, tasks, _ = _modules()
    cfg = T.load_config(["param_groups.no_decay_1d=true"])
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=_main_list(model, tasks))
    with caplog.at_level(logging.INFO, logger="egopack"):
        T.log_param_groups(T.logger, opt)
    lines = [r.getMessage() for r in caplog.records if "parameter group" in r.getMessage()]
    assert len(lines) == 2 and "all/no_decay" in lines[1] and "15 tensors" in lines[1] and "weight_decay 0" in lines[1]
    assert "5 tensors, 120 elements" in lines[0]


# ---- 2. the constructors ---------------------------------------------------------------------------------------------------------------
def test_a_key_other_than_lr_and_weight_decay_that_differs_is_refused_by_name():
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    p = _params()
    for cls, key, val in ((FlatAdamW, "betas", (0.5, 0.999)), (FlatAdam, "eps", 1e-6), (FlatSGD, "momentum", 0.5),
                          (FlatSGD, "dampening", 0.5), (FlatSGD, "nesterov", True)):
        with pytest.raises(ValueError) as e:
            cls(_three_groups(p, **{key: val}))
        assert repr(key) in str(e.value) and "groups 0 and 2" in str(e.value), str(e.value)
    for cls, flag in ((FlatAdam, True), (FlatAdamW, False)):  # (a key the constructor's defaults do not even carry)
        with pytest.raises(ValueError) as e:
            cls([{"params": [p[0]]}, {"params": [p[1]], "decoupled_weight_decay": flag}])
        assert "'decoupled_weight_decay'" in str(e.value) and "groups 0 and 1" in str(e.value)
    FlatSGD(_three_groups(p), momentum=0.9)  # (lr and weight_decay may differ)


def test_a_parameter_in_two_groups_raises_what_torch_raises():
    from egopack_amd.optim import FlatAdamW
    p = _params()
    groups = lambda: [{"params": [p[0], p[1]]}, {"params": [p[1], p[2]]}]
    with pytest.raises(ValueError) as ours:
        FlatAdamW(groups())
    with pytest.raises(ValueError) as theirs:
        torch.optim.AdamW(groups())
    assert str(ours.value) == str(theirs.value)
    # inside one list (and inside one group) a parameter named twice is kept once
    assert len(FlatAdamW([p[0], p[1], p[0]]).param_groups[0]["params"]) == 2
    assert len(FlatAdamW([{"params": [p[0], p[1], p[0]]}, {"params": [p[2]]}]).param_groups[0]["params"]) == 2
    with pytest.raises(ValueError, match="at most 64 parameter groups"):
        FlatAdamW([{"params": [torch.zeros(1, requires_grad=True)]} for _ in range(65)])


def test_group_segments_follow_the_slots():
    from egopack_amd.optim import FlatAdamW
    p = _params() + [torch.zeros(4, requires_grad=True)]  # (the last one never gets a gradient: no slot)
    opt = FlatAdamW([*_three_groups(p)[:2], {"params": [p[4], p[5]], "lr": 1e-3}])
    with pytest.raises(RuntimeError, match="no parameter has a gradient"):
        opt.group_segments()
    for q in p[:5]:
        q.grad = torch.zeros_like(q)
    # constructor order: [33x7 -> 64 rows x 7 = 448][64x64 = 4096] | [5 -> 8][3 -> 8] | [130x9 -> 192 rows x 9 = 1728]
    assert opt.group_segments() == [(0, 4544, 0), (4544, 4560, 1), (4560, 6288, 2)]
    # ... and in the order of the list the groups were cut from: slot by slot, adjacent slots of one group merged
    opt = FlatAdamW([*_three_groups(p)[:2], {"params": [p[4], p[5]], "lr": 1e-3}], layout_order=p)
    assert opt.group_segments() == [(0, 448, 0), (448, 456, 1), (456, 4552, 0), (4552, 4560, 1), (4560, 6288, 2)]
    segs = opt.group_segments()
    assert all(b % 4 == 0 and e % 4 == 0 for b, e, _ in segs) and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
    with pytest.raises(RuntimeError, match="segment table"):
        opt._check_segments([(0, 8, 0), (12, 16, 1)], 16)
    with pytest.raises(RuntimeError, match="segment table"):
        opt._check_segments([(0, 6, 0), (6, 16, 1)], 16)
    with pytest.raises(RuntimeError, match="covers"):
        opt._check_segments([(0, 8, 0)], 16)


# ---- 3. include/egopack_optim_groups.h beyond the common ledger ------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_optim_groups_header_includes_the_optim_header():
    from egopack_amd import _lib
    assert '#include "egopack_optim.h"' in _lib.HEADERS["optim_groups"].read_text()


def test_optim_groups_struct_size_and_limits():
    from egopack_amd import _lib
    assert ctypes.sizeof(_lib.OptimGroups) == 40 and _lib.OptimGroups.seg_begin.offset == 16
    from egopack_amd import optim
    assert (optim.MAX_SEGMENTS, optim.MAX_GROUPS) == (4096, 64) and "1..4096, 1..64" in _lib.HEADERS["optim_groups"].read_text()


def test_optim_groups_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert "optim_groups" in names and "optim" in names and len(set(names)) == len(names)


# ---- 4. host-side refusals of egk_optim_step_groups -------------------------------------------------------------------------------------
def _desc(**kw):
    """A descriptor of small fake non-null pointers: every check precedes the first dereference and the first launch."""
    from egopack_amd import _lib
    d = _lib.OptimDesc()
    d.rule, d.g_dtype, d.n = 1, 0, 64
    d.p = d.g = d.state0 = d.state1 = d.hyper = d.t_dev = 0x1000
    d.beta1, d.beta2, d.eps = 0.9, 0.999, 1e-8
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _table(**kw):
    from egopack_amd import _lib
    t = _lib.OptimGroups()
    t.base, t.n_seg, t.n_groups = 0, 2, 2
    t.seg_begin = t.seg_group = t.group_hyper = 0x2000
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_optim_step_groups_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()

    def refused(d, t, needle):
        rc = lib.egk_optim_step_groups(None, ctypes.byref(d) if d is not None else None, ctypes.byref(t) if t is not None else None)
        assert rc == -1 and needle in _lib.last_error() and "egk_optim_step_groups" in _lib.last_error(), (rc, _lib.last_error())

    refused(_desc(), None, "null group table")
    refused(None, _table(), "null descriptor")
    for base in (2, 5, -4):
        refused(_desc(), _table(base=base), "multiple of 4")
    for n_seg in (0, -1, 4097):
        refused(_desc(), _table(n_seg=n_seg), "n_seg in 1..4096")
    for n_groups in (0, 65):
        refused(_desc(), _table(n_groups=n_groups), "n_groups in 1..64")
    for name in ("seg_begin", "seg_group", "group_hyper"):
        refused(_desc(), _table(**{name: None}), "null table pointer")
    refused(_desc(), _table(seg_begin=0x2004), "misaligned table pointer")
    refused(_desc(), _table(seg_group=0x2002), "misaligned table pointer")
    refused(_desc(), _table(group_hyper=0x2008), "misaligned table pointer")
    # everything egk_optim_step refuses
    refused(_desc(rule=3), _table(), "unknown rule")
    refused(_desc(g_dtype=2), _table(), "unknown gradient dtype")
    refused(_desc(p=None), _table(), "null pointer")
    refused(_desc(p=0x1004), _table(), "16-byte aligned")
    refused(_desc(n=-1), _table(), "n >= 0")
    refused(_desc(state1=None), _table(), "missing state pointer")
    refused(_desc(rule=2, momentum=0.9, t_dev=None), _table(), "missing state pointer")
    refused(_desc(rule=2, momentum=0.0, nesterov=1), _table(), "nesterov")
    refused(_desc(bf16_shadow=0x1004), _table(), "shadow must be 8-byte aligned")
    # the limits themselves are accepted; n == 0 launches nothing
    assert lib.egk_optim_step_groups(None, ctypes.byref(_desc(n=0)), ctypes.byref(_table(n_seg=4096, n_groups=64, base=8))) == 0
    assert lib.egk_optim_step_groups(None, ctypes.byref(_desc(n=0)), ctypes.byref(_table(n_seg=1, n_groups=1))) == 0


# ---- 5. state dicts to and from the torch classes over the same groups ----------------------------------------------------------------
def _stepped(ref, params, steps=3):
    g = torch.Generator().manual_seed(9)
    for _ in range(steps):
        for q in params[:-1]:  # (the last parameter never gets a gradient: torch keeps no state for it)
            q.grad = torch.randn(q.shape, generator=g)
        ref.step()
    return ref.state_dict()


def _two_groups(p):
    return [{"params": [p[0], p[2]], "lr": 1e-2, "weight_decay": 1e-2}, {"params": [p[1], p[3], p[4]], "lr": 3e-3, "weight_decay": 0.0}]


@pytest.mark.parametrize("rule", ["adamw", "sgd_momentum"])
def test_two_group_state_round_trip_with_the_torch_class(rule):
    from egopack_amd.optim import FlatAdamW, FlatSGD
    torch_cls, flat_cls, keys = {"adamw": (torch.optim.AdamW, FlatAdamW, ("exp_avg", "exp_avg_sq")),
                                 "sgd_momentum": (lambda g: torch.optim.SGD(g, momentum=0.9), lambda g: FlatSGD(g, momentum=0.9),
                                                  ("momentum_buffer",))}[rule]
    params = _params()
    sd = _stepped(torch_cls(_two_groups(params)), params)
    assert sorted(sd["state"]) == [0, 1, 2, 3] and [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3, 4]]
    flat = flat_cls([{"params": g["params"]} for g in _two_groups(_params())])  # (CPU parameters: the state stays pending)
    flat.load_state_dict(sd)
    assert not flat.materialised
    assert [(g["lr"], g["weight_decay"]) for g in flat.param_groups] == [(1e-2, 1e-2), (3e-3, 0.0)]  # (the loaded groups win)
    back = flat.state_dict()
    assert sorted(back["state"]) == sorted(sd["state"])
    for i, st in sd["state"].items():
        for k in keys:
            assert torch.equal(st[k], back["state"][i][k]), (i, k)
    # the flat class's own layout before any state exists: torch's, indices running on across the groups
    own = flat_cls(_two_groups(_params())).state_dict()
    want = torch_cls(_two_groups(_params())).state_dict()
    assert [g["params"] for g in own["param_groups"]] == [g["params"] for g in want["param_groups"]] == [[0, 1], [2, 3, 4]]
    for a, b in zip(own["param_groups"], want["param_groups"]):
        assert all(a[k] == b[k] for k in a if k in b) and {"lr", "weight_decay", "params"} <= set(a)
    # ... and into a fresh torch optimizer, which steps on from it exactly as the one that wrote it
    fresh_params, cont_params = _params(), [q.detach().clone().requires_grad_(True) for q in params]
    fresh, cont = torch_cls(_two_groups(fresh_params)), torch_cls(_two_groups(cont_params))
    fresh.load_state_dict(back)
    cont.load_state_dict(sd)
    with torch.no_grad():
        for a, b in zip(fresh_params, params):
            a.copy_(b)
    g = torch.Generator().manual_seed(5)
    for a, b in zip(fresh_params[:-1], cont_params[:-1]):
        a.grad = torch.randn(a.shape, generator=g)
        b.grad = a.grad.clone()
    fresh.step()
    cont.step()
    for a, b in zip(fresh_params, cont_params):
        assert torch.equal(a, b)


def test_a_state_with_another_number_of_groups_raises_what_torch_raises():
    from egopack_amd.optim import FlatAdamW
    params = _params()
    sd2 = _stepped(torch.optim.AdamW(_two_groups(params)), params)
    params = _params()
    sd1 = _stepped(torch.optim.AdamW(params), params)
    for flat, ref, sd in ((FlatAdamW(_params()), torch.optim.AdamW(_params()), sd2),
                          (FlatAdamW(_two_groups(_params())), torch.optim.AdamW(_two_groups(_params())), sd1)):
        with pytest.raises(ValueError) as ours:
            flat.load_state_dict(sd)
        with pytest.raises(ValueError) as theirs:
            ref.load_state_dict(sd)
        assert str(ours.value) == str(theirs.value) and "different number of parameter groups" in str(ours.value)
    # a loaded group may not bring a key the groups must share
    bad = {"state": {}, "param_groups": [dict(g) for g in sd2["param_groups"]]}
    bad["param_groups"][1]["betas"] = (0.5, 0.9)
    with pytest.raises(ValueError, match="'betas'"):
        FlatAdamW(_two_groups(_params())).load_state_dict(bad)
    # the kernel-selecting keys stay the constructor's, group by group
    flat = FlatAdamW(_two_groups(_params()))
    plain_adam = _stepped(torch.optim.Adam(_two_groups(params)), params)
    flat.load_state_dict(plain_adam)
    assert all(g["decoupled_weight_decay"] is True for g in flat.param_groups)


# ---- 6. schedulers step every group -----------------------------------------------------------------------------------------------------
def test_build_scheduler_steps_both_groups():
    from egopack_amd import train as T
    from egopack_amd.optim import FlatAdamW
    cfg = T.load_config(["use_warmup=True", "num_epochs=10"])
    mk = lambda cls: cls(_two_groups(_params()))
    ours, ref = mk(FlatAdamW), mk(torch.optim.AdamW)
    s_ours, s_ref = T.build_scheduler(cfg, ours), T.build_scheduler(cfg, ref)
    assert isinstance(s_ours, torch.optim.lr_scheduler.ChainedScheduler)
    seen = []
    for _ in range(7):
        s_ours.step()
        s_ref.step()
        assert [g["lr"] for g in ours.param_groups] == [g["lr"] for g in ref.param_groups]
        seen.append(tuple(g["lr"] for g in ours.param_groups))
    assert len(set(seen)) == 7 and all(abs(a / b - 1e-2 / 3e-3) < 1e-9 for a, b in seen)
