"""The optimizer state in bf16 with seeded stochastic rounding, without a GPU: the refusals of the four descriptor fields on the
three entry points, the host model of the rounding (tests/optim_state_common.py), the ``optimizer_state:`` block of the config,
what ``build_optimizer`` hands on, the state dicts of a bf16-state optimizer against the torch classes, and the refusal of the
sharded update."""
import ctypes

import numpy as np
import pytest
import torch

from tests import optim_state_common as OS

SHAPES = [(5, 3), (4,), (2, 2)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]


# ---- 1. the refusals of the descriptor's tail, on the three doors ------------------------------------------------------------------
def _desc(**kw):
    """A descriptor of small fake non-null pointers (tests/test_optim_rules_cpu.py): every check precedes the first dereference."""
    from egopack_amd import _lib
    d = _lib.OptimDesc()
    d.rule, d.g_dtype, d.n = 0, 0, 64
    d.p = d.g = d.state0 = d.state1 = d.hyper = d.t_dev = 0x1000
    d.beta1, d.beta2, d.eps = 0.9, 0.999, 1e-8
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _table():
    from egopack_amd import _lib
    t = _lib.OptimGroups()
    t.base, t.n_seg, t.n_groups = 0, 2, 2
    t.seg_begin = t.seg_group = t.group_hyper = 0x2000
    return t


def _ema():
    from egopack_amd import _lib
    e = _lib.EmaDesc()
    e.ema, e.decay, e.warmup = 0x3000, 0.999, 0
    return e


def _doors():
    from egopack_amd import _lib
    lib = _lib.load()
    ref = ctypes.byref
    return {"egk_optim_step": lambda d: lib.egk_optim_step(None, ref(d)),
            "egk_optim_step_groups": lambda d: lib.egk_optim_step_groups(None, ref(d), ref(_table())),
            "egk_optim_step_ema": lambda d: lib.egk_optim_step_ema(None, ref(d), None, ref(_ema())),
            "egk_optim_step_ema (grouped)": lambda d: lib.egk_optim_step_ema(None, ref(d), ref(_table()), ref(_ema()))}


def test_the_descriptor_has_the_four_fields_at_its_end():
    from egopack_amd import _lib
    names = [f[0] for f in _lib.OptimDesc._fields_]
    assert names[-4:] == ["state_dtype", "state_round", "state_seed", "elem0"] and names[-5] == "gate"
    d = _lib.OptimDesc()
    assert (d.state_dtype, d.state_round, d.state_seed, d.elem0) == (0, 0, 0, 0)  # (a zeroed tail: the f32 launch)


@pytest.mark.parametrize("door", ["egk_optim_step", "egk_optim_step_groups", "egk_optim_step_ema", "egk_optim_step_ema (grouped)"])
def test_every_door_refuses_a_bad_state_tail_before_any_launch(door):
    from egopack_amd import _lib
    call = _doors()[door]
    A, U8, U4, U2 = 0x1000, 0x1008, 0x1004, 0x1002

    def refused(d, needle):
        rc = call(d)
        assert rc == -1 and needle in _lib.last_error() and door.split(" ")[0] in _lib.last_error(), (rc, _lib.last_error())

    for dt in (2, -1, 7):
        refused(_desc(state_dtype=dt), "unknown state dtype")
    for rnd in (2, -1):
        refused(_desc(state_dtype=1, state_round=rnd), "state_round in {0")
    refused(_desc(state_dtype=0, state_round=1), "needs a bf16 state")
    refused(_desc(state_dtype=1, state_round=1, t_dev=None), "needs t_dev")
    for e0 in (-4, 2, 5, 1 << 42):
        refused(_desc(state_dtype=1, elem0=e0), "elem0 must be a non-negative multiple of 4")
    refused(_desc(elem0=6), "elem0 must be a non-negative multiple of 4")  # (f32 state too: the field means the same)
    for rule, mom in ((0, 0.0), (1, 0.0), (2, 0.9)):
        for off in (U4, U2):
            refused(_desc(rule=rule, momentum=mom, state_dtype=1, state0=off), "bf16 state must be 8-byte aligned")
        if rule != 2:
            refused(_desc(rule=rule, state_dtype=1, state1=U4), "bf16 state must be 8-byte aligned")
    # f32 state keeps its message, an 8-byte aligned bf16 state passes (n == 0 launches nothing)
    refused(_desc(state0=U8), "16-byte aligned")
    assert call(_desc(n=0, state_dtype=1, state_round=1, state0=U8, state1=U8, elem0=4096, state_seed=(1 << 64) - 1)) == 0
    assert call(_desc(n=0, state_dtype=1, state_round=0, t_dev=None, elem0=(1 << 42) - 4)) == 0
    assert call(_desc(rule=2, n=0, state_dtype=1, state_round=1, state0=None, state1=None)) == 0  # (SGD without momentum: no state)
    # what was refused before this tail existed is still refused first, with its own message
    refused(_desc(rule=3, state_dtype=9), "unknown rule")
    refused(_desc(g_dtype=2, state_dtype=9), "unknown gradient dtype")
    refused(_desc(p=None, state_dtype=9), "null pointer")
    refused(_desc(n=-1, state_dtype=9), "n >= 0")
    refused(_desc(state0=None, state_dtype=9), "missing state pointer")
    refused(_desc(p=U4, state_dtype=1, state0=U2), "16-byte aligned")
    refused(_desc(bf16_shadow=U4, state_dtype=9), "shadow must be 8-byte aligned")
    refused(_desc(bf16_shadow=A, bf16_lo_shadow=U2, state_dtype=9), "low-half shadow must be 8-byte aligned")
    refused(_desc(rule=2, momentum=-0.5, state_dtype=9), "momentum >= 0")


def test_the_pinned_refusals_of_the_other_doors_come_before_the_tail():
    from egopack_amd import _lib
    lib = _lib.load()
    bad = _desc(state_dtype=9)
    t = _table()
    t.base = 2
    assert lib.egk_optim_step_groups(None, ctypes.byref(bad), ctypes.byref(t)) == -1 and "multiple of 4" in _lib.last_error()
    assert "base" in _lib.last_error()
    assert lib.egk_optim_step_groups(None, ctypes.byref(bad), None) == -1 and "null group table" in _lib.last_error()
    e = _ema()
    e.decay = 1.5
    assert lib.egk_optim_step_ema(None, ctypes.byref(bad), None, ctypes.byref(e)) == -1 and "decay in [0, 1)" in _lib.last_error()
    assert lib.egk_optim_step_ema(None, ctypes.byref(bad), None, None) == -1 and "null ema descriptor" in _lib.last_error()


# ---- 2. the host model of the rounding -----------------------------------------------------------------------------------------
ALL_R = np.arange(65536, dtype=np.uint32)


@pytest.mark.parametrize("x", [1.0 + 2.0 ** -9, -1.0 - 2.0 ** -9, 0.5 + 2.0 ** -12, 3.14159274, -2.71828175, 1e-3, 6.1e-39, -1e30,
                               1.0 + 255 * 2.0 ** -16, 0.59121])
def test_stochastic_rounding_is_exactly_unbiased(x):
    """Summed over all 65536 values of r, in integers: the results are the two bf16 neighbours of x, the upper one for exactly
    b & 0xFFFF of the draws -- so sum(result bits) * 2^16 == 2^16 * b, and the mean of the VALUES is x itself."""
    b = int(OS.f32_bits(np.float32(x)).reshape(-1)[0])
    got = OS.stochastic_bits(np.full(65536, b, dtype=np.uint32), ALL_R).astype(np.int64)
    lo, hi = b >> 16, (b >> 16) + 1
    assert set(np.unique(got).tolist()) <= {lo, hi}
    ups = int((got == hi).sum())
    assert ups == (b & 0xFFFF)                                      # (the magnitude grows for exactly b & 0xFFFF of the 65536 draws)
    assert int(got.sum()) == 65536 * lo + (b & 0xFFFF) == b         # (sum of the bf16 bit patterns == the f32 bit pattern)
    # ... which is the expectation of the VALUE (the inputs here have both neighbours in one binade: equally spaced values):
    vlo, vhi = (float(OS.widen(np.uint16(v & 0xFFFF))) for v in (lo, hi))
    if np.isfinite(vhi):
        mean = (vlo * (65536 - ups) + vhi * ups) / 65536            # (exact in f64: 8-bit mantissas times 17-bit counts)
        assert mean == float(np.float32(x))


def test_a_representable_value_is_unchanged_for_every_r():
    for x in (1.0, -1.0, 0.5, 3.0, -0.0078125, 1.0 + 2.0 ** -7, 3.3895314e38, 2.0 ** -133):  # (the last two: the largest finite bf16, the smallest denormal)
        b = OS.f32_bits(np.float32(x)).reshape(-1)
        assert int(b[0]) & 0xFFFF == 0, x
        got = OS.stochastic_bits(np.full(65536, b[0], dtype=np.uint32), ALL_R)
        assert (got == np.uint16(int(b[0]) >> 16)).all(), x


def test_signed_zero_infinities_nan_and_the_carries():
    z = OS.stochastic_bits(np.array([0x00000000, 0x80000000], dtype=np.uint32).repeat(65536), np.tile(ALL_R, 2)).reshape(2, -1)
    assert (z[0] == 0x0000).all() and (z[1] == 0x8000).all()       # +0 stays +0, -0 stays -0
    inf = OS.stochastic_bits(np.array([0x7F800000, 0xFF800000], dtype=np.uint32).repeat(65536), np.tile(ALL_R, 2)).reshape(2, -1)
    assert (inf[0] == 0x7F80).all() and (inf[1] == 0xFF80).all()   # inf: f2bf's bits, whatever r is
    nan = OS.widen(OS.stochastic_bits(np.full(65536, 0x7FC00001, dtype=np.uint32), ALL_R))
    assert np.isnan(nan).all()
    # the carry into the next binade: 1.99999988 (0x3FFFFFFF) goes to 1.9921875 (0x3FFF) or 2.0 (0x4000), for either sign
    for sign in (0, 0x80000000):
        got = OS.stochastic_bits(np.full(65536, sign | 0x3FFFFFFF, dtype=np.uint32), ALL_R)
        top = sign >> 16
        assert set(np.unique(got).tolist()) == {top | 0x3FFF, top | 0x4000} and int((got == (top | 0x4000)).sum()) == 65535
    # ... and out of the largest finite value: inf, as the header states
    got = OS.stochastic_bits(np.full(65536, 0x7F7FFFFF, dtype=np.uint32), ALL_R)
    assert set(np.unique(got).tolist()) == {0x7F7F, 0x7F80}
    # a denormal rounds inside the denormals / into the smallest normal the same way
    got = OS.stochastic_bits(np.full(65536, 0x007FFFFF, dtype=np.uint32), ALL_R)
    assert set(np.unique(got).tolist()) == {0x007F, 0x0080}


def test_nearest_is_torch_s_bfloat16_conversion():
    g = torch.Generator().manual_seed(4)
    x = torch.cat([torch.randn(4096, generator=g), torch.randn(512, generator=g) * 1e-30, torch.randn(512, generator=g) * 1e30,
                   torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.4e38])])
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(OS.nearest_bits(OS.f32_bits(x.numpy())), want)
    assert np.array_equal(OS.round_state(x.numpy(), 0), want)


def test_the_draws_depend_on_seed_step_element_and_buffer_only():
    from tests import philox_ref as P
    k = OS.key(1234)
    hi, lo = OS.random_bits(k, 7, 4096, 1031)
    # written out: element e draws word e & 3 of counter (t << 40) | (e >> 2)
    for i in (0, 1, 5, 1030):
        e = 4096 + i
        w = P.philox_u64_scalar((7 << 40) | (e >> 2), k)[e & 3]
        assert (int(hi[i]), int(lo[i])) == (w >> 16, w & 0xFFFF)
    # slicing: [0, n) in one piece equals two pieces with elem0 moved
    a_hi, a_lo = OS.random_bits(k, 7, 4096, 1028)
    b_hi, b_lo = OS.random_bits(k, 7, 4096 + 1028, 3)
    assert np.array_equal(np.concatenate([a_hi, b_hi]), hi) and np.array_equal(np.concatenate([a_lo, b_lo]), lo)
    assert not np.array_equal(OS.random_bits(k, 8, 4096, 1031)[0], hi)          # another step
    assert not np.array_equal(OS.random_bits(OS.key(1235), 7, 4096, 1031)[0], hi)  # another seed
    assert np.array_equal(OS.random_bits(k, 7 + (1 << 24), 4096, 1031)[0], hi)   # (t enters modulo 2^24)
    assert hi.max() < 65536 and lo.max() < 65536 and not np.array_equal(hi, lo)


def test_the_key_is_neither_the_dropout_key_nor_the_sampler_key_and_the_package_agrees():
    from egopack_amd import ops
    assert ops.OPTIM_STATE_KEY_SALT == OS.KEY_SALT == int.from_bytes(b"OPT_STAT", "big") != ops.SAMPLER_KEY_SALT
    for seed in (0, 1, 12345, (1 << 64) - 1):
        assert ops.optim_state_key(seed) == OS.key(seed) and 0 <= OS.key(seed) < 1 << 64
        assert len({seed, ops.sampler_key(seed), ops.optim_state_key(seed)}) == 3
    prev = ops._rng["seed"]
    try:
        ops.manual_seed(77)
        assert ops.optim_state_key(None) == OS.key(77)
    finally:
        ops.manual_seed(prev)


# ---- 3. the config block -------------------------------------------------------------------------------------------------------
def test_optimizer_state_config_defaults_case_folding_and_errors():
    from egopack_amd import train as T
    cfg = T.load_config([])
    assert T.optimizer_state_config(cfg) == {"dtype": "f32", "rounding": "stochastic", "seed": None}
    assert dict(cfg.optimizer_state) == {"dtype": "f32", "rounding": "stochastic", "seed": None}
    assert "optimizer_state" not in cfg.optimizer and not any("state" in k for k in cfg.optimizer)  # (beside ``optimizer:``, not inside)
    assert T.optimizer_state_config({}) == {"dtype": "f32", "rounding": "stochastic", "seed": None}
    got = T.optimizer_state_config(T.load_config(["optimizer_state.dtype=BF16", "optimizer_state.rounding=Nearest", "optimizer_state.seed=5"]))
    assert got == {"dtype": "bf16", "rounding": "nearest", "seed": 5}
    with pytest.raises(ValueError) as e:
        T.optimizer_state_config({"optimizer_state": {"dtype": "bf16", "bits": 8}})
    assert "bits" in str(e.value) and all(k in str(e.value) for k in ("dtype", "rounding", "seed"))
    with pytest.raises(ValueError) as e:
        T.optimizer_state_config({"optimizer_state": {"dtype": "fp8"}})
    assert "fp8" in str(e.value) and "f32" in str(e.value) and "bf16" in str(e.value)
    with pytest.raises(ValueError) as e:
        T.optimizer_state_config({"optimizer_state": {"dtype": "bf16", "rounding": "floor"}})
    assert "floor" in str(e.value) and "stochastic" in str(e.value) and "nearest" in str(e.value)
    for seed in (-1, 1 << 64, 1.5, True, "7"):
        with pytest.raises(ValueError, match="optimizer_state.seed"):
            T.optimizer_state_config({"optimizer_state": {"seed": seed}})


def test_build_optimizer_default_is_what_it_was_and_the_block_is_passed_on():
    from egopack_amd import train as T
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    opt = T.build_optimizer(T.load_config([]), _params())
    assert type(opt) is FlatAdam and opt.state_dtype is torch.float32 and not opt.bf16_state
    opt = T.build_optimizer(T.load_config(["optimizer_state.dtype=bf16"]), _params())
    assert type(opt) is FlatAdam and opt.state_dtype is torch.bfloat16 and opt.bf16_state and opt.state_rounding == "stochastic"
    opt = T.build_optimizer(T.load_config(["optimizer._target_=torch.optim.AdamW", "optimizer_state.dtype=bf16",
                                           "optimizer_state.rounding=nearest", "optimizer_state.seed=9"]), _params())
    assert type(opt) is FlatAdamW and opt.bf16_state and opt.state_rounding == "nearest" and opt.state_seed == 9
    opt = T.build_optimizer(T.load_config(["optimizer._target_=torch.optim.SGD", "+optimizer.momentum=0.9", "optimizer_state.dtype=bf16"]),
                            _params())
    assert type(opt) is FlatSGD and opt.bf16_state
    for kw in (dict(state_dtype=torch.float16), dict(state_dtype=torch.bfloat16, state_rounding="floor"),
               dict(state_dtype=torch.bfloat16, state_seed=-1)):
        with pytest.raises(ValueError):
            FlatAdam(_params(), **kw)


# ---- 4. state dicts of a bf16-state optimizer on CPU parameters (pending state) ------------------------------------------------------
def _stepped(ref, params, steps=3):
    g = torch.Generator().manual_seed(9)
    for _ in range(steps):
        for q in params[:-1]:
            q.grad = torch.randn(q.shape, generator=g)
        ref.step()
    return ref.state_dict()


@pytest.mark.parametrize("rule", ["adam", "adamw", "sgd_momentum"])
def test_a_bf16_state_round_trips_with_the_torch_class(rule):
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    bf = dict(state_dtype=torch.bfloat16, state_seed=11)
    make = {"adam": (lambda p: torch.optim.Adam(p, lr=1e-2), lambda p: FlatAdam(p, lr=1e-2, **bf), ("exp_avg", "exp_avg_sq")),
            "adamw": (lambda p: torch.optim.AdamW(p, lr=1e-2), lambda p: FlatAdamW(p, lr=1e-2, **bf), ("exp_avg", "exp_avg_sq")),
            "sgd_momentum": (lambda p: torch.optim.SGD(p, lr=1e-2, momentum=0.9), lambda p: FlatSGD(p, lr=1e-2, momentum=0.9, **bf),
                             ("momentum_buffer",))}
    torch_cls, flat_cls, keys = make[rule]
    params = _params()
    sd = _stepped(torch_cls(params), params)
    flat = flat_cls(_params())
    flat.load_state_dict(sd)  # (CPU parameters: the state stays pending)
    assert not flat.materialised
    back = flat.state_dict()
    assert (back["state_dtype"], back["state_rounding"], back["state_seed"]) == ("bf16", "stochastic", 11)
    assert sorted(back["state"]) == sorted(sd["state"])
    for i, st in sd["state"].items():
        for k in keys:  # f32 tensors: the incoming moments rounded to nearest, widened
            assert back["state"][i][k].dtype == torch.float32
            assert torch.equal(back["state"][i][k], st[k].to(torch.bfloat16).float()), (i, k)
    # exact for a dict a bf16 run wrote: a second trip changes nothing
    again = flat_cls(_params())
    again.load_state_dict(back)
    for i, st in back["state"].items():
        for k in keys:
            assert torch.equal(again.state_dict()["state"][i][k], st[k])
    # ... and the dict, extra keys and all, loads into the torch class of the rule
    fresh_params = _params()
    fresh = torch_cls(fresh_params)
    fresh.load_state_dict(back)
    for i, q in enumerate(fresh_params[:-1]):
        for k in keys:
            assert torch.equal(fresh.state[q][k], back["state"][i][k]), (i, k)
    for q in fresh_params[:-1]:
        q.grad = torch.ones_like(q)
    fresh.step()
    assert all(bool(torch.isfinite(q).all()) for q in fresh_params)
    # an f32-state optimizer takes a bf16 run's dict as it is (widened: exact) and writes the dict it always wrote, without the keys
    f32 ={"adam": FlatAdam, "adamw": FlatAdamW, "sgd_momentum": lambda p, **kw: FlatSGD(p, momentum=0.9, **kw)}[rule](_params(), lr=1e-2)
    f32.load_state_dict(back)
    out = f32.state_dict()
    assert sorted(out) == ["param_groups", "state"]
    for i, st in back["state"].items():
        for k in keys:
            assert torch.equal(out["state"][i][k], st[k])


def test_bf16_state_with_the_sharded_update_is_refused_by_name(monkeypatch):
    from egopack_amd.optim import FlatAdam, FlatSGD
    monkeypatch.setenv("EGK_ENABLE", "sharded_update")
    for make in (lambda: FlatAdam(_params(), state_dtype=torch.bfloat16), lambda: FlatSGD(_params(), momentum=0.9, state_dtype=torch.bfloat16)):
        with pytest.raises(ValueError) as e:
            make()
        assert "sharded_update" in str(e.value) and "bfloat16" in str(e.value) and "optimizer_state.dtype" in str(e.value)
    FlatAdam(_params())  # (f32 state: as before)
    monkeypatch.delenv("EGK_ENABLE")
    FlatAdam(_params(), state_dtype=torch.bfloat16)
