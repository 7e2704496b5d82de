"""Guard-band tests of include/egopack_optim.h: egk_optim_step touches only what its descriptor names.

The form of tests/test_gpu_bounds.py (its helpers and its ``Guards`` are imported; nothing is registered there): every device
argument sits in a sentinel-filled window, the outputs are compared with an f64 reference of the rule at the tolerance of
tests/test_gpu_kernels.py::test_flat_adam_matches_torch_adam, everything outside the windows must keep the sentinel bits, and a
second run on plain buffers must give the same bits.  The ledger of this header is in tests/test_optim_rules_cpu.py; the module
imports without a GPU."""
import ctypes as C
import math

import pytest
import torch

from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, S, bf16, close, edt, f32, gen, i32, i64, ok, r16, refused, same

TOL = dict(rtol=1e-5, atol=1e-6)  # tests/test_gpu_kernels.py::test_flat_adam_matches_torch_adam
ADAM, ADAMW, SGD = 0, 1, 2

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list


def case(*covers, variants=None, plain=True):
    def deco(fn):
        for v in variants or [dict()]:
            v = dict(v)
            second = v.pop("plain", plain)
            vid = v.pop("id", None) or "-".join(f"{k}={B._fmt(x)}" for k, x in v.items())
            CASES.append((fn.__name__ + ("-" + vid if vid else ""), fn, v, covers, second))
        fn.covers = covers
        return fn
    return deco


def covered():
    """Every entry point some case declares it covers (the ledger in tests/test_optim_rules_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


def _rule_ref(rule, p, g, s0, s1, hyper, first, b1, b2, eps, wd, mu, damp, nesterov):
    """The rule in f64 on the stored inputs (torch 2.10's single-tensor formulas)."""
    p, g = p.double(), g.double()
    lr, bc1, bc2s, gs = (float(h) for h in hyper)
    if rule == SGD:
        gg = g * gs + wd * p
        step = gg
        if mu:
            s0 = gg if first else mu * s0.double() + (1 - damp) * gg
            step = gg + mu * s0 if nesterov else s0
        return p - lr * step, s0, None
    if rule == ADAMW:
        p = p * (1 - lr * wd)
        gg = g * gs
    else:
        gg = g * gs + wd * p
    m = s0.double() + (gg - s0.double()) * (1 - b1)
    v = s1.double() * b2 + (1 - b2) * gg * gg
    return p - (lr / bc1) * (m / (v.sqrt() / bc2s + eps)), m, v


@case("egk_optim_step",
      variants=[dict(rule=ADAM, n=1003, gdt=f32), dict(rule=ADAM, n=4099, gdt=bf16, gate=1), dict(rule=ADAM, n=1003, gdt=f32, gate=0),
                dict(rule=ADAMW, n=1003, gdt=f32, gate=1), dict(rule=ADAMW, n=4099, gdt=bf16), dict(rule=ADAMW, n=1003, gdt=bf16, gate=0),
                dict(rule=ADAMW, n=4096, gdt=f32, lo=False), dict(rule=ADAMW, n=0, gdt=f32),
                dict(rule=SGD, n=1003, gdt=f32), dict(rule=SGD, n=4099, gdt=bf16, wd=1e-3, gate=1), dict(rule=SGD, n=1003, gdt=f32, gate=0),
                dict(rule=SGD, n=1003, gdt=f32, mu=0.9, t=1), dict(rule=SGD, n=4099, gdt=bf16, mu=0.9, damp=0.1, t=3, gate=1),
                dict(rule=SGD, n=1001, gdt=f32, mu=0.9, nesterov=1, wd=1e-3, t=2), dict(rule=SGD, n=1003, gdt=bf16, mu=0.9, t=2, gate=0),
                dict(rule=SGD, n=4096, gdt=f32, mu=0.9, t=1, gate=1, lo=False), dict(rule=SGD, n=0, gdt=f32, mu=0.9), dict(rule=SGD, n=0, gdt=f32)])
def optim_step(lib, ops, G, rule, n, gdt, gate=None, wd=1e-2, mu=0.0, damp=0.0, nesterov=0, t=2, lo=True):
    """The launch runs over an inner slice of larger flat buffers (the guards ARE the rest of the buffers), n % 4 != 0; a rule
    without a state buffer is handed none (NULL), and SGD without momentum no step counter either."""
    from egopack_amd import _lib
    gn = gen(n + 97 * rule + 7)
    p, g = torch.randn(n, generator=gn), r16(torch.randn(n, generator=gn))
    a, b = torch.randn(n, generator=gn) * 0.1, torch.rand(n, generator=gn) * 0.01
    hyper = torch.tensor([1e-2, 1 - 0.9 ** 3, math.sqrt(1 - 0.999 ** 3), 0.5])
    b1, b2, eps = 0.9, 0.999, 1e-8
    n_state = 2 if rule != SGD else (1 if mu else 0)
    Pp, Gg, H = G.v("p", n, f32, init=p), G.v("g", n, gdt, init=g), G.v("hyper", 4, f32, init=hyper)
    S0 = G.v("state0", n, f32, init=a) if n_state >= 1 else None
    S1 = G.v("state1", n, f32, init=b) if n_state >= 2 else None
    T = G.v("t_dev", 1, i64, init=torch.tensor([t]), poison=0) if (rule == SGD and mu) or rule != SGD else None
    hi, lo16 = G.v("bf16_shadow", n, bf16), (G.v("bf16_lo_shadow", n, bf16) if lo else None)
    bump = G.v("bump_word", 1, i64, init=torch.tensor([100]), poison=0)
    gt = G.v("gate", 1, i32, init=torch.tensor([gate]), poison=1) if gate is not None else None
    d = _lib.OptimDesc()
    d.rule, d.g_dtype, d.n = rule, edt(gdt), n
    d.p, d.g, d.hyper = Pp.ptr, Gg.ptr, H.ptr
    d.state0, d.state1, d.t_dev = (x.ptr if x is not None else None for x in (S0, S1, T))
    d.beta1, d.beta2, d.eps, d.weight_decay, d.momentum, d.dampening, d.nesterov = b1, b2, eps, wd, mu, damp, nesterov
    d.bf16_shadow, d.bf16_lo_shadow = hi.ptr, (lo16.ptr if lo16 is not None else None)
    d.bump_word, d.bump, d.gate = bump.ptr, 7, (gt.ptr if gt is not None else None)
    ok(lib.egk_optim_step(S(), C.byref(d)), "egk_optim_step")
    G.check()
    assert bump.view.tolist() == [107 if n > 0 else 100], "bump_word"
    if T is not None:
        assert T.view.tolist() == [t], "t_dev is read, never written"
    if gate == 0:  # a skipped step: nothing but *bump_word changes
        same(Pp.view, p, "p")
        if S0 is not None:
            same(S0.view, a, "state0")
        if S1 is not None:
            same(S1.view, b, "state1")
        assert bool(hi.is_sentinel().all()) and (lo16 is None or bool(lo16.is_sentinel().all())), "a gated-off step wrote a bf16 copy"
    else:
        rp, r0, r1 = _rule_ref(rule, p, g, a, b, hyper, t == 1, b1, b2, eps, wd, mu, damp, nesterov)
        close(Pp.view, rp.float(), "p", **TOL)
        if S0 is not None:
            close(S0.view, r0.float(), "state0", **TOL)
        if S1 is not None:
            close(S1.view, r1.float(), "state1", **TOL)
        pd = Pp.view.clone()
        same(hi.view.view(torch.int16), pd.to(bf16).view(torch.int16), "bf16_shadow")  # = bf16(p) of the stored p, bit for bit
        if lo16 is not None:
            same(lo16.view.view(torch.int16), (pd - pd.to(bf16).float()).to(bf16).view(torch.int16), "bf16_lo_shadow")
    # refused on the host, nothing launched: a misaligned slice, a state pointer the rule needs and does not get
    if n > 4:
        d.p = Pp.ptr + 4
        refused(lib.egk_optim_step(S(), C.byref(d)), "16-byte aligned")
        d.p = Pp.ptr
        if n_state:
            d.state0 = None
            refused(lib.egk_optim_step(S(), C.byref(d)), "missing state pointer")
        G.check()
        assert bump.view.tolist() == [107], "a refused call moved the offset word"
    out = dict(p=Pp, hi=hi)
    for k, x in (("state0", S0), ("state1", S1), ("lo", lo16)):
        if x is not None:
            out[k] = x
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_optim(name, fn, variant, covers, plain):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib, ops
    lib = _lib.load()
    try:
        G = Guards()
        out = fn(lib, ops, G, **variant)
        G.check()
        if plain and out:
            got = {k: B._bits(v) for k, v in out.items()}
            H = Guards(plain=True)
            base = fn(lib, ops, H, **variant)
            torch.cuda.synchronize()
            for k, v in base.items():
                b = B._bits(v)
                assert got[k].shape == b.shape and torch.equal(got[k], b), f"{k}: the guarded call and the contiguous call differ in bits"
    finally:
        torch.cuda.synchronize()
