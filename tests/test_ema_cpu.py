"""The weight average of the flat optimizers without a GPU: what include/egopack_ema.h pins beyond the one ledger (tests/test_cabi.py),
the host-side refusals of its two entry points, the constructors' refusals, the configuration keys, the state dict of an optimizer
whose flat buffers do not exist yet, the torch classes loading a state dict that carries an average, and the refusal under the
sharded update."""
import ctypes
import logging

import pytest
import torch

SHAPES = [(5, 3), (4,), (2, 2)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]


# ---- 1. include/egopack_ema.h beyond the common ledger ---------------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_ema_header_includes_the_groups_header():
    from egopack_amd import _lib
    assert '#include "egopack_optim_groups.h"' in _lib.HEADERS["ema"].read_text()


def test_ema_struct_layout_matches_header():
    from egopack_amd import _lib
    from tests import cabi_common as CC
    assert [n for n, _ in CC.struct_fields("ema", "egk_ema_desc")] == [f[0] for f in _lib.EmaDesc._fields_] == ["ema", "decay", "warmup"]
    assert ctypes.sizeof(_lib.EmaDesc) == 24 and _lib.EmaDesc.decay.offset == 8 and _lib.EmaDesc.warmup.offset == 16


def test_optim_ema_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert {"optim_ema", "optim_groups", "optim", "adam"} <= set(names) and len(set(names)) == len(names)


# ---- 2. host-side refusals --------------------------------------------------------------------------------------------------------------
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


def _ema(**kw):
    from egopack_amd import _lib
    e = _lib.EmaDesc()
    e.ema, e.decay, e.warmup = 0x3000, 0.999, 0
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_optim_step_ema_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()
    ref = lambda x: ctypes.byref(x) if x is not None else None

    def refused(d, t, e, needle):
        rc = lib.egk_optim_step_ema(None, ref(d), ref(t), ref(e))
        assert rc == -1 and needle in _lib.last_error() and "egk_optim_step_ema" in _lib.last_error(), (rc, _lib.last_error())

    for t in (None, _table()):  # (plain and grouped)
        refused(None, t, _ema(), "null descriptor")
        refused(_desc(), t, None, "null ema descriptor")
        refused(_desc(), t, _ema(ema=None), "null ema pointer")
        for off in (4, 8, 12):
            refused(_desc(), t, _ema(ema=0x3000 + off), "ema must be 16-byte aligned")
        for decay in (1.0, 1.5, -1e-9, float("nan"), float("inf")):
            refused(_desc(), t, _ema(decay=decay), "decay in [0, 1)")
        refused(_desc(rule=2, momentum=0.0, state0=None, state1=None, t_dev=None), t, _ema(warmup=1), "warmup needs t_dev")
        refused(_desc(t_dev=None), t, _ema(warmup=1), "warmup needs t_dev")
        # everything egk_optim_step refuses
        refused(_desc(rule=3), t, _ema(), "unknown rule")
        refused(_desc(g_dtype=2), t, _ema(), "unknown gradient dtype")
        refused(_desc(p=None), t, _ema(), "null pointer")
        refused(_desc(p=0x1004), t, _ema(), "16-byte aligned")
        refused(_desc(n=-1), t, _ema(), "n >= 0")
        refused(_desc(state1=None), t, _ema(), "missing state pointer")
        refused(_desc(rule=2, momentum=0.9, t_dev=None), t, _ema(), "missing state pointer")
        refused(_desc(rule=2, momentum=0.0, nesterov=1), t, _ema(), "nesterov")
        refused(_desc(bf16_shadow=0x1004), t, _ema(), "shadow must be 8-byte aligned")
        refused(_desc(bf16_lo_shadow=0x1004), t, _ema(), "low-half shadow must be 8-byte aligned")
    # ... and everything egk_optim_step_groups refuses in its table
    for base in (2, 5, -4):
        refused(_desc(), _table(base=base), _ema(), "multiple of 4")
    for n_seg in (0, -1, 4097):
        refused(_desc(), _table(n_seg=n_seg), _ema(), "n_seg in 1..4096")
    for n_groups in (0, 65):
        refused(_desc(), _table(n_groups=n_groups), _ema(), "n_groups in 1..64")
    for name in ("seg_begin", "seg_group", "group_hyper"):
        refused(_desc(), _table(**{name: None}), _ema(), "null table pointer")
    refused(_desc(), _table(seg_begin=0x2004), _ema(), "misaligned table pointer")
    # the limits themselves are accepted; n == 0 launches nothing
    assert lib.egk_optim_step_ema(None, ref(_desc(n=0)), None, ref(_ema(decay=0.0))) == 0
    assert lib.egk_optim_step_ema(None, ref(_desc(n=0)), ref(_table(n_seg=4096, n_groups=64, base=8)), ref(_ema(warmup=1))) == 0
    assert lib.egk_optim_step_ema(None, ref(_desc(n=0, rule=2, state0=None, state1=None, t_dev=None)), None, ref(_ema())) == 0


def test_ema_swap_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()

    def refused(p, e, n, needle):
        rc = lib.egk_ema_swap(None, p, e, n)
        assert rc == -1 and needle in _lib.last_error() and "egk_ema_swap" in _lib.last_error(), (rc, _lib.last_error())

    refused(None, 0x3000, 8, "null pointer")
    refused(0x1000, None, 8, "null pointer")
    refused(0x1004, 0x3000, 8, "16-byte aligned")
    refused(0x1000, 0x3008, 8, "16-byte aligned")
    refused(0x1000, 0x3000, -1, "n >= 0")
    assert lib.egk_ema_swap(None, 0x1000, 0x3000, 0) == 0


# ---- 3. the constructors ----------------------------------------------------------------------------------------------------------------
def test_constructors_take_and_check_the_ema_arguments():
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    for cls in (FlatAdam, FlatAdamW, FlatSGD):
        for off in (dict(), dict(ema_decay=None), dict(ema_decay=0), dict(ema_decay=0.0, ema_warmup=True)):
            opt = cls(_params(), **off)
            assert not opt.ema and opt.ema_decay == 0.0 and opt.flat_ema is None and "ema" not in opt.state_dict()
        opt = cls(_params(), ema_decay=0.999)
        assert opt.ema and opt.ema_decay == 0.999 and opt.ema_warmup is False and opt.flat_ema is None
        opt = cls(_params(), ema_decay=0.9, ema_warmup=True)
        assert opt.ema and opt.ema_warmup is True
        for bad in (1.0, 1.5, -0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError) as e:
                cls(_params(), ema_decay=bad)
            assert "ema_decay" in str(e.value) and cls.__name__ in str(e.value)
    # the average does not enter the parameter groups (torch's loader, the schedulers and _check_groups never see it)
    assert "ema_decay" not in FlatAdamW(_params(), ema_decay=0.5).param_groups[0]
    # without an average there is no context; with one, and no flat buffers yet, the average is the parameters
    with pytest.raises(RuntimeError, match="ema_decay"):
        with FlatAdamW(_params()).ema_weights():
            pass
    opt = FlatAdamW(_params(), ema_decay=0.5)
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="nesting"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.state_dict()
    assert not opt._ema_swapped
    with opt.ema_weights():  # (the failed nested entry left the outer context, and its exit, intact)
        pass


# ---- 4. the configuration ---------------------------------------------------------------------------------------------------------------
TARGETS = {"torch.optim.Adam": "FlatAdam", "torch.optim.AdamW": "FlatAdamW", "torch.optim.SGD": "FlatSGD"}


def test_build_optimizer_maps_the_ema_keys_for_the_three_targets():
    from egopack_amd import train as T
    cfg = T.load_config([])
    assert dict(cfg.ema) == {"decay": 0, "warmup": False, "validate": True, "save": True} and "ema" not in cfg.optimizer
    assert "decay" not in cfg.optimizer and T.ema_saved(cfg)
    for target, name in TARGETS.items():
        opt = T.build_optimizer(T.load_config([f"optimizer._target_={target}"]), _params())
        assert type(opt).__name__ == name and not opt.ema and opt.flat_ema is None
        opt = T.build_optimizer(T.load_config([f"optimizer._target_={target}", "ema.decay=0.999", "ema.warmup=true"]), _params())
        assert type(opt).__name__ == name and opt.ema and opt.ema_decay == 0.999 and opt.ema_warmup is True
        opt = T.build_optimizer(T.load_config([f"optimizer._target_={target}", "ema.decay=0.9", "grad_clip_norm=1.0"]), _params())
        assert opt.ema_decay == 0.9 and opt.ema_warmup is False and opt.max_grad_norm == 1.0
        with pytest.raises(ValueError, match="ema_decay"):
            T.build_optimizer(T.load_config([f"optimizer._target_={target}", "ema.decay=1.0"]), _params())
    with pytest.raises(ValueError, match="momentum"):
        T.build_optimizer(T.load_config(["+ema.momentum=0.9"]), _params())
    # groups and the average combine
    p = _params()
    groups = [{"params": [p[0], p[2]], "weight_decay": 1e-2}, {"params": [p[1]], "weight_decay": 0.0}]
    opt = T.build_optimizer(T.load_config(["optimizer._target_=torch.optim.AdamW", "ema.decay=0.99"]), groups, layout_order=p)
    assert opt.grouped and opt.ema
    assert not T.ema_saved(T.load_config(["ema.save=false"]))


def test_ema_scope_and_the_validation_log_line(caplog):
    import contextlib
    from egopack_amd import train as T
    on, off = T.load_config(["ema.decay=0.99", "ema.warmup=true"]), T.load_config([])
    no_val = T.load_config(["ema.decay=0.99", "ema.validate=false"])
    opt_on, opt_off = T.build_optimizer(on, _params()), T.build_optimizer(off, _params())
    assert isinstance(T.ema_scope(off, opt_off), contextlib.nullcontext)
    assert isinstance(T.ema_scope(no_val, T.build_optimizer(no_val, _params())), contextlib.nullcontext)
    with T.ema_scope(on, opt_on):
        assert opt_on._ema_swapped
    assert not opt_on._ema_swapped
    with caplog.at_level(logging.INFO, logger="egopack"):
        T.log_validation_weights(T.logger, on, opt_on, 3)
        T.log_validation_weights(T.logger, off, opt_off, 3)
        T.log_validation_weights(T.logger, no_val, T.build_optimizer(no_val, _params()), 3)
    lines = [r.getMessage() for r in caplog.records if "validating" in r.getMessage()]
    assert len(lines) == 3 and "averaged weights" in lines[0] and "0.99" in lines[0] and "warm-up" in lines[0]
    assert "raw weights" in lines[1] and "raw weights" in lines[2] and "ema.validate" in lines[2]


# ---- 5. state dicts ------------------------------------------------------------------------------------------------------------------
def _stepped(ref, params, steps=3):
    g = torch.Generator().manual_seed(9)
    for _ in range(steps):
        for q in params[:-1]:  # (the last parameter never gets a gradient: torch keeps no state for it)
            q.grad = torch.randn(q.shape, generator=g)
        ref.step()
    return ref.state_dict()


def _with_ema(sd, decay=0.99, warmup=True):
    g = torch.Generator().manual_seed(3)
    return {**sd, "ema": {"decay": decay, "warmup": warmup, "values": {i: torch.randn(SHAPES[i], generator=g) for i in sd["state"]}}}


MAKE = {"adam": (lambda p: torch.optim.Adam(p, lr=1e-2), "FlatAdam", dict(lr=1e-2)),
        "adamw": (lambda p: torch.optim.AdamW(p, lr=1e-2), "FlatAdamW", dict(lr=1e-2)),
        "sgd_momentum": (lambda p: torch.optim.SGD(p, lr=1e-2, momentum=0.9), "FlatSGD", dict(lr=1e-2, momentum=0.9))}


@pytest.mark.parametrize("rule", list(MAKE))
def test_an_unmaterialised_optimizer_carries_the_average_through_its_pending_state(rule, caplog):
    from egopack_amd import optim
    torch_cls, flat_name, kw = MAKE[rule]
    flat_cls = getattr(optim, flat_name)
    params = _params()
    sd = _with_ema(_stepped(torch_cls(params), params))
    assert sorted(sd["ema"]["values"]) == [0, 1]
    flat = flat_cls(_params(), ema_decay=0.99, ema_warmup=True, **kw)  # (CPU parameters: the state stays pending, no flat buffers)
    assert flat.state_dict()["ema"] == {"decay": 0.99, "warmup": True, "values": {}}
    flat.load_state_dict(sd)
    assert not flat.materialised and flat._pending_state is not None and flat.flat_ema is None
    back = flat.state_dict()
    assert sorted(back) == ["ema", "param_groups", "state"] and sorted(back["ema"]) == ["decay", "values", "warmup"]
    assert back["ema"]["decay"] == 0.99 and back["ema"]["warmup"] is True and sorted(back["ema"]["values"]) == [0, 1]
    for i, v in sd["ema"]["values"].items():
        assert torch.equal(back["ema"]["values"][i], v) and back["ema"]["values"][i] is not v  # (a snapshot, not the caller's tensors)
    for i, st in sd["state"].items():
        for k, v in st.items():
            if torch.is_tensor(v) and k != "step":
                assert torch.equal(back["state"][i][k], v)
    # an average of the wrong shape is refused by index, before anything changes
    bad = _with_ema(sd)
    bad["ema"]["values"][1] = torch.zeros(5)
    fresh = flat_cls(_params(), ema_decay=0.99, **kw)
    with pytest.raises(ValueError) as e:
        fresh.load_state_dict(bad)
    assert "parameter 1" in str(e.value) and "(5,)" in str(e.value) and "(4,)" in str(e.value) and fresh._pending_state is None
    # "ema" absent with the average on, "ema" present with the average off: one log line each, nothing raised
    plain = {k: v for k, v in sd.items() if k != "ema"}
    with caplog.at_level(logging.INFO, logger="egopack"):
        on = flat_cls(_params(), ema_decay=0.99, **kw)
        on.load_state_dict(plain)
        starts = [r.getMessage() for r in caplog.records]
        caplog.clear()
        off = flat_cls(_params(), **kw)
        off.load_state_dict(sd)
        ignored = [r.getMessage() for r in caplog.records]
    assert len(starts) == 1 and "starts from the loaded parameters" in starts[0]
    assert len(ignored) == 1 and "ignored" in ignored[0]
    assert "ema" not in on._pending_state and "ema" not in off._pending_state and "ema" not in off.state_dict()


@pytest.mark.parametrize("rule", list(MAKE))
def test_the_torch_class_loads_a_state_dict_that_carries_an_average(rule):
    """torch's loader reads "state" and "param_groups" and ignores other top-level keys: the round trip is untouched."""
    from egopack_amd import optim
    torch_cls, flat_name, kw = MAKE[rule]
    params = _params()
    sd = _with_ema(_stepped(torch_cls(params), params))
    flat = getattr(optim, flat_name)(_params(), ema_decay=0.99, ema_warmup=True, **kw)
    flat.load_state_dict(sd)
    back = flat.state_dict()
    assert "ema" in back
    fresh_params, cont_params = _params(), [q.detach().clone().requires_grad_(True) for q in params]
    fresh, cont = torch_cls(fresh_params), torch_cls(cont_params)
    fresh.load_state_dict(back)  # (with the "ema" key in it)
    cont.load_state_dict({k: v for k, v in sd.items() if k != "ema"})
    assert "ema" not in fresh.state_dict()
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


# ---- 6. the sharded update --------------------------------------------------------------------------------------------------------------
def test_the_sharded_update_refuses_an_optimizer_with_an_average():
    from egopack_amd import dist as edist
    from egopack_amd.optim import FlatAdamW
    sync = edist.GradSync(2, shard_update=True)
    opt = FlatAdamW(_params(), ema_decay=0.99)
    for call in (lambda: sync._sharded_step(opt), lambda: sync.start(opt, 0, 8)):
        with pytest.raises(ValueError) as e:
            call()
        assert "sharded_update" in str(e.value) and "ema" in str(e.value)


# ---- 7. the host model the GPU tests compare with ---------------------------------------------------------------------------------------
def test_the_host_model_rounds_three_times_and_the_weight_once():
    import numpy
    from tests import ema_common as E
    assert E.ema_weight(0.999, False, 7) == numpy.float32(1.0 - 0.999) and E.ema_weight(0.0, False, 1) == numpy.float32(1.0)
    # warm-up: t = 1, 2, 3 give three different d_t below the decay, a late step the decay itself
    ws = [E.ema_weight(0.99, True, t) for t in (1, 2, 3)]
    assert ws == [numpy.float32(1.0 - 2.0 / 11.0), numpy.float32(1.0 - 3.0 / 12.0), numpy.float32(1.0 - 4.0 / 13.0)] and len(set(ws)) == 3
    assert E.ema_weight(0.99, True, 10 ** 6) == numpy.float32(1.0 - 0.99) and E.ema_weight(0.1, True, 1) == numpy.float32(0.9)
    g = torch.Generator().manual_seed(1)
    e, p = torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    w = E.ema_weight(0.9, False, 1)
    got = E.ema_model(e, p, w)
    want = (e.double() + (float(w) * (p.double() - e.double()).float().double()).float().double()).float()
    assert torch.equal(got, want)
    assert [E.segments(n) for n in (8, 1016, 1024, 3080)] == [([0, 4, 8], [0, 1]), ([0, 336, 676, 1016], [0, 1, 2]),
                                                                ([0, 340, 680, 1024], [0, 1, 2]), ([0, 1024, 2052, 3080], [0, 1, 2])]
