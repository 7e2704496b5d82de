"""The update rules behind one launch interface, without a GPU: the configuration targets, the state dicts against torch.optim.AdamW /
torch.optim.SGD, what include/egopack_optim.h pins beyond the one ledger (tests/test_cabi.py), the host-side refusals of
egk_optim_step, and GradSync.gather_moments over an optimizer with one state buffer and with none."""
import ctypes
import os
import re
import socket

import pytest
import torch

SHAPES = [(5, 3), (4,), (2, 2)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]


# ---- 1. the configuration targets -----------------------------------------------------------------------------------------------
def test_build_optimizer_serves_the_three_targets():
    from egopack_amd import train as T
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    p = _params()
    opt = T.build_optimizer(T.load_config([]), p)
    assert type(opt) is FlatAdam and not opt.decoupled_weight_decay
    assert opt.param_groups[0]["weight_decay"] == 1e-5 and "decoupled_weight_decay" not in opt.param_groups[0]
    opt = T.build_optimizer(T.load_config(["optimizer._target_=torch.optim.AdamW", "grad_clip_norm=2.0"]), p)
    assert type(opt) is FlatAdamW and opt.decoupled_weight_decay and opt.max_grad_norm == 2.0
    assert opt.param_groups[0]["weight_decay"] == 1e-5 and opt.param_groups[0]["lr"] == 1e-5
    opt = T.build_optimizer(T.load_config(["+optimizer.decoupled_weight_decay=true"]), p)
    assert type(opt) is FlatAdamW and opt.param_groups[0]["weight_decay"] == 1e-5
    assert FlatAdamW(p).param_groups[0]["weight_decay"] == 0.01  # (torch.optim.AdamW's default)
    assert type(FlatAdam(p, decoupled_weight_decay=True)) is FlatAdam and FlatAdam(p, decoupled_weight_decay=True).decoupled_weight_decay
    opt = T.build_optimizer(T.load_config(["optimizer._target_=torch.optim.SGD", "+optimizer.momentum=0.9", "+optimizer.nesterov=true",
                                           "grad_clip_norm=1.5"]), p)
    g = opt.param_groups[0]
    assert type(opt) is FlatSGD and (g["momentum"], g["nesterov"], g["dampening"], g["weight_decay"]) == (0.9, True, 0, 1e-5)
    assert opt.max_grad_norm == 1.5
    opt = T.build_optimizer(T.load_config(["optimizer._target_=torch.optim.SGD", "+optimizer.momentum=0.9", "+optimizer.dampening=0.1"]), p)
    assert type(opt) is FlatSGD and opt.param_groups[0]["dampening"] == 0.1 and not opt.param_groups[0]["nesterov"]
    with pytest.raises(ValueError) as e:
        T.build_optimizer(T.load_config(["optimizer._target_=torch.optim.RMSprop"]), p)
    assert all(name in str(e.value) for name in ("torch.optim.Adam", "torch.optim.AdamW", "torch.optim.SGD", "RMSprop"))
    # what is not built is refused by name; execution hints are accepted
    for target in ("torch.optim.Adam", "torch.optim.AdamW"):
        with pytest.raises(ValueError, match="amsgrad"):
            T.build_optimizer(T.load_config([f"optimizer._target_={target}", "+optimizer.amsgrad=true"]), p)
    for target in ("torch.optim.Adam", "torch.optim.AdamW", "torch.optim.SGD"):
        with pytest.raises(ValueError, match="maximize"):
            T.build_optimizer(T.load_config([f"optimizer._target_={target}", "+optimizer.maximize=true"]), p)
        T.build_optimizer(T.load_config([f"optimizer._target_={target}", "+optimizer.foreach=false", "+optimizer.fused=false",
                                         "+optimizer.capturable=true", "+optimizer.differentiable=false"]), p)


def test_constructors_raise_what_torch_raises():
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    p = _params()
    for kw in (dict(momentum=0.0, nesterov=True), dict(momentum=0.9, dampening=0.1, nesterov=True), dict(lr=-1.0), dict(momentum=-0.1),
               dict(weight_decay=-1e-3)):
        with pytest.raises(ValueError) as ours:
            FlatSGD(p, **kw)
        with pytest.raises(ValueError) as theirs:
            torch.optim.SGD(p, **kw)
        assert str(ours.value) == str(theirs.value), kw
    for cls, ref in ((FlatAdam, torch.optim.Adam), (FlatAdamW, torch.optim.AdamW)):
        for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
            with pytest.raises(ValueError) as ours:
                cls(p, **kw)
            with pytest.raises(ValueError) as theirs:
                ref(p, **kw)
            assert str(ours.value) == str(theirs.value), (cls, kw)
    assert FlatSGD(p).state_buffers() == [] and FlatAdamW(p).state_buffers() == [] and FlatAdam(p).flat_m is None


# ---- 2. state dicts to and from the torch classes ------------------------------------------------------------------------------------
def _stepped(ref, params, steps=3):
    g = torch.Generator().manual_seed(9)
    for _ in range(steps):
        for q in params[:-1]:  # (the last parameter never gets a gradient: torch keeps no state for it)
            q.grad = torch.randn(q.shape, generator=g)
        ref.step()
    return ref.state_dict()


def _same_state(a, b, keys):
    assert sorted(a["state"]) == sorted(b["state"])
    for i, st in a["state"].items():
        for k in keys:
            assert torch.equal(st[k], b["state"][i][k]), (i, k)


@pytest.mark.parametrize("rule", ["adamw", "sgd_momentum", "sgd_nesterov", "sgd_plain"])
def test_torch_state_loads_into_the_flat_class_and_back(rule):
    from egopack_amd.optim import FlatAdamW, FlatSGD
    make = {"adamw": (lambda p: torch.optim.AdamW(p, lr=1e-2, weight_decay=1e-2), lambda p: FlatAdamW(p, lr=1e-2, weight_decay=1e-2),
                      ("exp_avg", "exp_avg_sq")),
            "sgd_momentum": (lambda p: torch.optim.SGD(p, lr=1e-2, momentum=0.9, dampening=0.1),
                             lambda p: FlatSGD(p, lr=1e-2, momentum=0.9, dampening=0.1), ("momentum_buffer",)),
            "sgd_nesterov": (lambda p: torch.optim.SGD(p, lr=1e-2, momentum=0.9, nesterov=True),
                             lambda p: FlatSGD(p, lr=1e-2, momentum=0.9, nesterov=True), ("momentum_buffer",)),
            "sgd_plain": (lambda p: torch.optim.SGD(p, lr=1e-2, weight_decay=1e-3), lambda p: FlatSGD(p, lr=1e-2, weight_decay=1e-3), ())}
    torch_cls, flat_cls, keys = make[rule]
    params = _params()
    sd = _stepped(torch_cls(params), params)
    assert sorted(sd["state"]) == ([0, 1] if keys else [])
    flat = flat_cls(_params())   # (CPU parameters: the state stays pending, no flat buffers)
    flat.load_state_dict(sd)
    assert not flat.materialised
    back = flat.state_dict()
    _same_state(sd, back, keys)
    if keys:
        assert flat.step_count == 3 if rule == "adamw" else flat.step_count == 1  # (a torch SGD state has no ``step``: one step taken)
    # ... and into a fresh torch optimizer, which steps on from it exactly as the one that wrote it
    fresh_params, cont_params = _params(), [q.detach().clone().requires_grad_(True) for q in params]
    fresh = torch_cls(fresh_params)
    fresh.load_state_dict(back)
    with torch.no_grad():
        for a, b in zip(fresh_params, params):
            a.copy_(b)
    cont = torch_cls(cont_params)
    cont.load_state_dict(sd)
    g = torch.Generator().manual_seed(5)
    for a, b in zip(fresh_params[:-1], cont_params[:-1]):
        a.grad = torch.randn(a.shape, generator=g)
        b.grad = a.grad.clone()
    fresh.step()
    cont.step()
    for a, b in zip(fresh_params, cont_params):
        assert torch.equal(a, b)


def test_flat_sgd_state_carries_a_step_entry_torch_accepts():
    """The flat classes' own layout (a ``step`` entry beside ``momentum_buffer``) loads into torch.optim.SGD."""
    from egopack_amd.optim import FlatSGD
    params = _params()
    sd = {"state": {0: {"step": torch.tensor(4.0), "momentum_buffer": torch.ones(5, 3)}, 1: {"step": torch.tensor(4.0), "momentum_buffer": torch.ones(4)}},
          "param_groups": [dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, params=[0, 1, 2])]}
    flat = FlatSGD(_params(), lr=1e-2, momentum=0.9)
    flat.load_state_dict(sd)
    assert flat.step_count == 4
    ref = torch.optim.SGD(params, lr=1e-2, momentum=0.9)
    ref.load_state_dict(flat.state_dict())
    for q in params[:-1]:
        q.grad = torch.ones_like(q)
    before = params[0].detach().clone()
    ref.step()
    assert torch.allclose(params[0], before - 1e-2 * (0.9 * 1.0 + 1.0))  # (the loaded buffer was used: no first-step branch)


def test_a_state_of_another_rule_is_refused_by_name():
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    params = _params()
    adam_sd = _stepped(torch.optim.AdamW(params), params)
    params = _params()
    sgd_sd = _stepped(torch.optim.SGD(params, lr=1e-2, momentum=0.9), params)
    with pytest.raises(RuntimeError) as e:
        FlatSGD(_params(), lr=1e-2, momentum=0.9).load_state_dict(adam_sd)
    assert "exp_avg" in str(e.value) and "FlatSGD" in str(e.value) and "momentum_buffer" in str(e.value)
    with pytest.raises(RuntimeError, match="exp_avg"):
        FlatSGD(_params(), lr=1e-2).load_state_dict(adam_sd)
    for cls in (FlatAdam, FlatAdamW):
        with pytest.raises(RuntimeError) as e:
            cls(_params()).load_state_dict(sgd_sd)
        assert "momentum_buffer" in str(e.value) and cls.__name__ in str(e.value) and "exp_avg" in str(e.value)
    with pytest.raises(RuntimeError, match="momentum_buffer"):
        FlatSGD(_params(), lr=1e-2).load_state_dict(sgd_sd)  # (configured without momentum: no buffer to load it into)
    opt = FlatAdamW(_params())
    opt.load_state_dict(adam_sd)  # (Adam's and AdamW's states are the same state)
    assert opt.decoupled_weight_decay and opt.param_groups[0]["decoupled_weight_decay"] is True


# ---- 3. include/egopack_optim.h beyond the common ledger -------------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_optim_rule_codes_match_header():
    from egopack_amd import _lib
    text = _lib.HEADERS["optim"].read_text()
    codes = dict(re.findall(r"(EGK_OPT_[A-Z]+) = (\d)", text))
    assert codes == {"EGK_OPT_ADAM": "0", "EGK_OPT_ADAMW": "1", "EGK_OPT_SGD": "2"}
    assert (_lib.OPT_ADAM, _lib.OPT_ADAMW, _lib.OPT_SGD) == (0, 1, 2)


# ---- 4. host-side refusals of egk_optim_step ---------------------------------------------------------------------------------------------
def _desc(**kw):
    """A descriptor of small fake non-null pointers: every check precedes the first dereference and the first launch."""
    from egopack_amd import _lib
    d = _lib.OptimDesc()
    d.rule, d.g_dtype, d.n = 0, 0, 64
    d.p = d.g = d.state0 = d.state1 = d.hyper = d.t_dev = 0x1000
    d.beta1, d.beta2, d.eps = 0.9, 0.999, 1e-8
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_optim_step_refuses_bad_descriptors_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()
    A, U4, U2 = 0x1000, 0x1004, 0x1002

    def refused(d, needle):
        rc = lib.egk_optim_step(None, ctypes.byref(d)) if d is not None else lib.egk_optim_step(None, None)
        assert rc == -1 and needle in _lib.last_error(), (rc, _lib.last_error())

    refused(None, "null descriptor")
    for rule in (3, -1):
        refused(_desc(rule=rule), "unknown rule")
    refused(_desc(g_dtype=2), "unknown gradient dtype")
    for rule in (0, 1, 2):
        for name in ("p", "g", "hyper"):
            refused(_desc(rule=rule, **{name: None}), "null pointer")
        for name in ("p", "g"):
            refused(_desc(rule=rule, **{name: U4}), "16-byte aligned")
        refused(_desc(rule=rule, momentum=0.9, bf16_shadow=U4), "shadow must be 8-byte aligned")
        refused(_desc(rule=rule, momentum=0.9, bf16_shadow=A, bf16_lo_shadow=U2), "low-half shadow must be 8-byte aligned")
        refused(_desc(rule=rule, n=-1), "n >= 0")
    for rule in (0, 1):
        refused(_desc(rule=rule, state0=None), "missing state pointer")
        refused(_desc(rule=rule, state1=None), "missing state pointer")
        refused(_desc(rule=rule, state0=U4), "16-byte aligned")
        refused(_desc(rule=rule, state1=U4), "16-byte aligned")
    refused(_desc(rule=2, momentum=0.9, state0=None), "missing state pointer")
    refused(_desc(rule=2, momentum=0.9, t_dev=None), "missing state pointer")
    refused(_desc(rule=2, momentum=0.9, state0=U4), "16-byte aligned")
    refused(_desc(rule=2, momentum=-0.5), "momentum >= 0")
    refused(_desc(rule=2, momentum=0.0, nesterov=1), "nesterov")
    refused(_desc(rule=2, momentum=0.9, dampening=0.1, nesterov=1), "nesterov")
    # n == 0 launches nothing; SGD without momentum names no state and no counter
    assert lib.egk_optim_step(None, ctypes.byref(_desc(n=0))) == 0
    assert lib.egk_optim_step(None, ctypes.byref(_desc(rule=2, n=0, state0=None, state1=None, t_dev=None))) == 0
    assert lib.egk_optim_step(None, ctypes.byref(_desc(rule=2, n=0, momentum=0.9, nesterov=1, state1=None))) == 0


def test_optim_step_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert "optim" in names and "adam" in names and len(set(names)) == len(names)


# ---- 5. gather_moments over one state buffer and over none (gloo, world 2) ---------------------------------------------------------------
class _CpuSGD:
    """The slice-wise interface dist.GradSync drives (tests/test_dist_gloo.py::_CpuAdam) for SGD in plain torch on the CPU, with the
    state accessor of optim.FlatOptimizer: one momentum buffer, or none."""

    def __init__(self, n, momentum):
        g = torch.Generator().manual_seed(3)
        self.flat_p = torch.randn(n, generator=g)
        self.flat_g = torch.zeros(n)
        self.momentum = momentum
        self._bufs = [torch.zeros(n)] if momentum else []
        self.step_count, self.grad_scale, self.refreshed = 0, 1.0, 0

    def state_buffers(self):
        return list(self._bufs)

    def prepare_hyper(self):
        self._first = self.step_count == 0

    def launch(self, grads=None, lo=0, hi=None):
        sl = slice(lo, self.flat_p.numel() if hi is None else hi)
        g = (self.flat_g if grads is None else grads)[sl] * self.grad_scale
        if self.momentum:
            buf = self._bufs[0]
            buf[sl] = g if self._first else self.momentum * buf[sl] + g
            g = buf[sl]
        self.flat_p[sl] -= 1e-2 * g

    def refresh_shadows(self):
        self.refreshed += 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_worker(rank, world, port, q):
    import torch.distributed as dist
    from egopack_amd.dist import GradSync, init_from_env
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    init_from_env(backend="gloo")
    n, ok = 1000, True
    for momentum in (0.9, 0.0):
        ref, shd = _CpuSGD(n, momentum), _CpuSGD(n, momentum)
        sync = GradSync(world, shard_update=True)
        per, lo, hi, body = sync.shard_bounds(n)
        for step in range(3):
            g = torch.randn(n, generator=torch.Generator().manual_seed(100 * step + rank))
            ref.flat_g.copy_(g)
            dist.all_reduce(ref.flat_g)
            ref.grad_scale = 1.0 / world
            ref.prepare_hyper()
            ref.launch()
            ref.step_count += 1
            shd.flat_g.copy_(g)
            sync.reduce_and_step(shd)
        ok = ok and torch.equal(ref.flat_p, shd.flat_p) and shd.step_count == 3
        ok = ok and getattr(shd, "_moments_sharded", False) is True
        if momentum:
            other = torch.ones(n, dtype=torch.bool)
            other[lo:hi] = False
            other[body:] = False
            buf = shd.state_buffers()[0]
            ok = ok and not buf[other].any() and torch.equal(buf[lo:hi], ref.state_buffers()[0][lo:hi])
        sync.gather_moments(shd)  # (a collective with one buffer; with none there is nothing to gather and the flag clears)
        ok = ok and shd._moments_sharded is False
        if momentum:
            ok = ok and torch.equal(shd.state_buffers()[0], ref.state_buffers()[0])
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_gloo_world2_gather_moments_with_one_state_buffer_and_with_none():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=100) for _ in procs)
    for p in procs:
        p.join(30)
    assert res == [(0, True), (1, True)]
