"""Guard-band tests of the bf16 optimizer state (include/egopack_optim.h: state_dtype = EGK_BF16) on the three entry points that take
the descriptor: a launch touches only what its arguments name.

The form of tests/test_gpu_bounds_optim.py (the helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is
registered there): every device argument sits in a sentinel-filled window, the bf16 state windows at an 8-byte aligned offset that
is NOT 16-byte aligned, n has a tail, and everything outside [0, n) must keep the sentinel bits.  The values are checked where they
can be checked exactly: p and the copies against the f32-state launch on the widened state, the stored state against the host model
of the rounding (tests/optim_state_common.py).  The module imports without a GPU."""
import ctypes as C
import math

import pytest
import torch

from tests import optim_state_common as OS
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, S, bf16, f32, gen, i32, i64, ok, refused, same

ADAM, ADAMW, SGD = 0, 1, 2
KEY = OS.key(99)
CASES = [dict(door=door, rule=rule, n=n, mode=mode, gate=gate)
         for door in ("step", "groups", "ema")
         for rule, n, mode, gate in ((ADAM, 1003, 1, None), (ADAMW, 4099, 1, 1), (SGD, 1001, 1, None), (ADAM, 1003, 0, None),
                                     (ADAMW, 1003, 1, 0), (SGD, 2, 1, None))]


def _id(c):
    return f"{c['door']}-rule{c['rule']}-n{c['n']}-mode{c['mode']}" + ("" if c["gate"] is None else f"-gate{c['gate']}")


def _bits(t):
    return t.detach().view(torch.int16).cpu().numpy().view("uint16")


def _launch(lib, _lib, door, d, table, ema):
    if door == "ema":
        return lib.egk_optim_step_ema(S(), C.byref(d), C.byref(table), C.byref(ema))
    if door == "groups":
        return lib.egk_optim_step_groups(S(), C.byref(d), C.byref(table))
    return lib.egk_optim_step(S(), C.byref(d))


def _case(lib, G, door, rule, n, mode, gate, narrow, elem0=8200, t=5):
    """One launch with every argument in a guarded window; ``narrow``: the state in bf16 (windows 8 bytes off a 16-byte boundary),
    otherwise the f32-state launch on the widened state (the reference)."""
    from egopack_amd import _lib
    gn = gen(n + 13 * rule)
    p, g = torch.randn(n, generator=gn), torch.randn(n, generator=gn)
    a, b = (torch.randn(n, generator=gn) * 0.1).to(bf16).float(), (torch.rand(n, generator=gn) * 0.01).to(bf16).float()
    hyper = torch.tensor([1e-2, 1 - 0.9 ** t, math.sqrt(1 - 0.999 ** t), 0.5])
    mom = 0.9 if rule == SGD else 0.0
    sdt, off = (bf16, 4) if narrow else (f32, 0)  # (4 bf16 elements: the window starts 8 bytes behind a 16-byte boundary)
    Pp, Gg, H = G.v("p", n, f32, init=p), G.v("g", n, f32, init=g), G.v("hyper", 4, f32, init=hyper)
    S0 = G.v("state0", n, sdt, init=a, offset_elems=off)
    S1 = G.v("state1", n, sdt, init=b, offset_elems=off) if rule != SGD else None
    T = G.v("t_dev", 1, i64, init=torch.tensor([t]), poison=0)
    hi, lo16 = G.v("bf16_shadow", n, bf16), G.v("bf16_lo_shadow", n, bf16)
    bump = G.v("bump_word", 1, i64, init=torch.tensor([100]), poison=0)
    gt = G.v("gate", 1, i32, init=torch.tensor([gate]), poison=1) if gate is not None else None
    if narrow and not G.plain:
        assert S0.ptr % 8 == 0 and S0.ptr % 16 == 8 and (S1 is None or S1.ptr % 16 == 8)
    d = _lib.OptimDesc()
    d.rule, d.g_dtype, d.n = rule, 0, n
    d.p, d.g, d.hyper, d.t_dev = Pp.ptr, Gg.ptr, H.ptr, T.ptr
    d.state0, d.state1 = S0.ptr, (S1.ptr if S1 is not None else None)
    d.beta1, d.beta2, d.eps, d.weight_decay, d.momentum = 0.9, 0.999, 1e-8, 1e-2, mom
    d.bf16_shadow, d.bf16_lo_shadow, d.bump_word, d.bump = hi.ptr, lo16.ptr, bump.ptr, 7
    d.gate = gt.ptr if gt is not None else None
    if narrow:
        d.state_dtype, d.state_round, d.state_seed, d.elem0 = 1, mode, KEY, elem0
    table = ema = E = None
    if door in ("groups", "ema"):  # one group that holds the launch's lr and weight decay, two segments cut inside the launch
        cut = elem0 + (n // 8) * 4
        SB = G.v("seg_begin", 3, i64, init=torch.tensor([0, cut, elem0 + n]), poison=0)
        SG = G.v("seg_group", 2, i32, init=torch.tensor([0, 0]), poison=0)
        GH = G.v("group_hyper", 4, f32, init=torch.tensor([1e-2, 1e-2, 0.0, 0.0]))
        table = _lib.OptimGroups()
        table.base, table.n_seg, table.n_groups = elem0, 2, 1
        table.seg_begin, table.seg_group, table.group_hyper = SB.ptr, SG.ptr, GH.ptr
    if door == "ema":
        E = G.v("ema", n, f32, init=p * 0.5)
        ema = _lib.EmaDesc()
        ema.ema, ema.decay, ema.warmup = E.ptr, 0.99, 1
    ok(_launch(lib, _lib, door, d, table, ema), door)
    G.check()
    assert bump.view.tolist() == [107], "bump_word"
    assert T.view.tolist() == [t], "t_dev is read, never written"
    if narrow and n > 4:  # refused on the host, nothing launched
        d.state0 = S0.ptr + 2
        refused(_launch(lib, _lib, door, d, table, ema), "bf16 state must be 8-byte aligned")
        d.state0, d.elem0 = S0.ptr, elem0 + 2
        refused(_launch(lib, _lib, door, d, table, ema), "elem0 must be a non-negative multiple of 4")
        d.elem0 = elem0
        G.check()
        assert bump.view.tolist() == [107], "a refused call moved the offset word"
    out = dict(p=Pp, hi=hi, lo=lo16, state0=S0)
    if S1 is not None:
        out["state1"] = S1
    if E is not None:
        out["ema"] = E
    return out, dict(p=p, a=a, b=b, t=t, elem0=elem0)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_bounds_optim_state(c):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib
    lib = _lib.load()
    try:
        G = Guards()
        got, prob = _case(lib, G, narrow=True, **c)
        G.check()
        R = Guards()
        ref, _ = _case(lib, R, narrow=False, **c)  # the f32-state launch on the widened state
        R.check()
        if c["gate"] == 0:  # a skipped step: nothing but *bump_word changed
            same(got["p"].view, prob["p"], "p")
            same(got["state0"].view.float(), prob["a"], "state0")
            if "state1" in got:
                same(got["state1"].view.float(), prob["b"], "state1")
            assert bool(got["hi"].is_sentinel().all()) and bool(got["lo"].is_sentinel().all()), "a gated-off step wrote a bf16 copy"
        else:
            for k in ("p", "hi", "lo") + (("ema",) if "ema" in got else ()):
                same(B._bits(got[k]), B._bits(ref[k]), f"{k}: the bf16-state launch against the f32-state launch")
            for k, buf in (("state0", 0), ("state1", 1)):
                if k in got:
                    want = OS.round_state(ref[k].view.cpu().numpy(), c["mode"], KEY, prob["t"], prob["elem0"], buf)
                    assert (_bits(got[k].view.contiguous()) == want).all(), f"{k}: not the host model's rounding of the f32 launch's state"
        H = Guards(plain=True)  # ... and the same bits on plain contiguous buffers
        base, _ = _case(lib, H, narrow=True, **c)
        torch.cuda.synchronize()
        for k, v in base.items():
            assert torch.equal(B._bits(got[k]), B._bits(v)), f"{k}: the guarded call and the contiguous call differ in bits"
    finally:
        torch.cuda.synchronize()
