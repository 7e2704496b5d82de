"""Guard-band tests of include/egopack_ema.h: egk_optim_step_ema touches only what its descriptor, its group table and its ema
descriptor name; egk_ema_swap only its two buffers.

The form of tests/test_gpu_bounds_param_groups.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is
registered there): every device argument -- ``ema`` and the three tables included -- sits in a sentinel-filled window; p, the state
and both bf16 copies are compared BIT FOR BIT with one egk_optim_step launch per segment (tests/param_groups_common.py), ``ema``
with the host model of tests/ema_common.py applied to the stored p; everything outside the windows must keep the sentinel bits,
and a second run on plain buffers must give the same bits.  The ledger of this header is in tests/test_ema_cpu.py; the module
imports without a GPU."""
import ctypes as C

import pytest
import torch

from tests import ema_common as E
from tests import param_groups_common as PG
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, S, bf16, f32, gen, i32, i64, ok, refused, same

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
DECAY = 0.9


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
    """Every entry point some case declares it covers (the ledger in tests/test_ema_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


@case("egk_optim_step_ema",
      variants=[dict(kind="adam", n=1003, gdt=f32), dict(kind="adam", n=4099, gdt=bf16, gate=1, groups=True, warmup=1),
                dict(kind="adam", n=1003, gdt=f32, gate=0, warmup=1),
                dict(kind="adamw", n=1003, gdt=f32, gate=1, warmup=1), dict(kind="adamw", n=4099, gdt=bf16, groups=True, base=1024),
                dict(kind="adamw", n=1003, gdt=bf16, gate=0, groups=True), dict(kind="adamw", n=4099, gdt=f32, lo=False),
                dict(kind="adamw", n=0, gdt=f32), dict(kind="adamw", n=0, gdt=f32, groups=True),
                dict(kind="sgd", n=1003, gdt=f32, groups=True, warmup=1), dict(kind="sgd", n=4099, gdt=bf16, gate=1),
                dict(kind="sgd", n=1003, gdt=f32, gate=0),
                dict(kind="sgd_momentum", n=1003, gdt=f32), dict(kind="sgd_momentum", n=4099, gdt=bf16, gate=1, groups=True, base=8),
                dict(kind="sgd_momentum", n=1003, gdt=bf16, gate=0, warmup=1),
                dict(kind="sgd_momentum", n=4099, gdt=f32, lo=False, gate=1, groups=True, warmup=1)])
def optim_step_ema(lib, ops, G, kind, n, gdt, gate=None, lo=True, base=0, groups=False, warmup=0):
    """``groups``: five segments over three groups (``base``: the launch is a slice [base, base + m) of the table's range, and
    ``hyper[0]`` and the descriptor's weight_decay are NaN: ignored); otherwise no table, lr in ``hyper[0]``.  ``ema`` starts from
    values of its own (not p), so a thread that read the wrong element of it, or none, is seen."""
    from egopack_amd import _lib
    key = n if n else 1003
    begins, m = PG.SEG_BEGINS[key], max(n - base, 0)
    prob = PG.problem(m, kind, gdt)
    ns = prob["n_state"]
    hyper = prob["hyper"].clone()
    if not groups:
        hyper[0] = PG.ONE_GROUP[0]
    e0 = torch.randn(m, generator=gen(m + 5))
    Pp, Gg, H = G.v("p", m, f32, init=prob["p"]), G.v("g", m, gdt, init=prob["g"]), G.v("hyper", 4, f32, init=hyper)
    S0 = G.v("state0", m, f32, init=prob["a"]) if ns >= 1 else None
    S1 = G.v("state1", m, f32, init=prob["b"]) if ns >= 2 else None
    T = G.v("t_dev", 1, i64, init=prob["t"], poison=0)
    EM = G.v("ema", m, f32, init=e0)
    hi, lo16 = G.v("bf16_shadow", m, bf16), (G.v("bf16_lo_shadow", m, bf16) if lo else None)
    bump = G.v("bump_word", 1, i64, init=torch.tensor([100]), poison=0)
    gt = G.v("gate", 1, i32, init=torch.tensor([gate]), poison=1) if gate is not None else None
    d = PG.descriptor(kind, gdt, m, Pp.ptr, Gg.ptr, S0.ptr if S0 is not None else 0, S1.ptr if S1 is not None else 0, H.ptr, T.ptr,
                      hi.ptr, lo16.ptr if lo16 is not None else 0, bump.ptr, gt.ptr if gt is not None else None,
                      weight_decay=float("nan") if groups else PG.ONE_GROUP[1])
    t = None
    if groups:
        SB = G.v("seg_begin", len(begins), i64, init=torch.tensor(begins), poison=1 << 40)
        SG = G.v("seg_group", len(PG.SEG_GROUPS), i32, init=torch.tensor(PG.SEG_GROUPS, dtype=torch.int32), poison=3)
        rows = PG.hyper_rows(PG.GROUP_HYPER + [(float("nan"), float("nan"))])
        GH = G.v("group_hyper", rows.numel(), f32, init=rows.reshape(-1))
        t = PG.group_table(base, SB.ptr, SG.ptr, GH.ptr, n_groups=4, n_seg=len(PG.SEG_GROUPS))
    e = _lib.EmaDesc()
    e.ema, e.decay, e.warmup = EM.ptr, DECAY, warmup
    tp = C.byref(t) if t is not None else None
    ok(lib.egk_optim_step_ema(S(), C.byref(d), tp, C.byref(e)), "egk_optim_step_ema")
    G.check()
    assert bump.view.tolist() == [107 if m > 0 else 100], "bump_word"
    assert T.view.tolist() == prob["t"].tolist(), "t_dev is read, never written"
    if gate == 0:  # a skipped step: nothing but *bump_word changes
        same(Pp.view, prob["p"], "p")
        same(EM.view, e0, "ema")
        if S0 is not None:
            same(S0.view, prob["a"], "state0")
        if S1 is not None:
            same(S1.view, prob["b"], "state1")
        assert bool(hi.is_sentinel().all()) and (lo16 is None or bool(lo16.is_sentinel().all())), "a gated-off step wrote a bf16 copy"
    elif m > 0:
        if groups:
            ref = PG.reference(prob, begins, PG.SEG_GROUPS, PG.GROUP_HYPER, gate=gate, lo=lo, base=base)
        else:
            ref = PG.reference(prob, [0, (m + 3) // 4 * 4], [0], [PG.ONE_GROUP], gate=gate, lo=lo)
        assert bool(torch.isfinite(ref["p"]).all()) and not torch.equal(ref["p"], prob["p"])
        same(Pp.view, ref["p"], "p")
        if S0 is not None:
            same(S0.view, ref["state0"], "state0")
        if S1 is not None:
            same(S1.view, ref["state1"], "state1")
        same(hi.view.view(torch.int16), ref["hi"], "bf16_shadow")
        if lo16 is not None:
            same(lo16.view.view(torch.int16), ref["lo"], "bf16_lo_shadow")
        w = E.ema_weight(DECAY, warmup, int(prob["t"][0]))
        want = E.ema_model(e0, Pp.view.detach().cpu().clone(), w)
        assert not torch.equal(want, e0)
        same(EM.view, want, "ema")
    # refused on the host, nothing launched
    if m > 4:
        e.ema = EM.ptr + 4
        refused(lib.egk_optim_step_ema(S(), C.byref(d), tp, C.byref(e)), "ema must be 16-byte aligned")
        e.ema = EM.ptr
        e.decay = 1.0
        refused(lib.egk_optim_step_ema(S(), C.byref(d), tp, C.byref(e)), "decay in [0, 1)")
        e.decay = DECAY
        d.p = Pp.ptr + 4
        refused(lib.egk_optim_step_ema(S(), C.byref(d), tp, C.byref(e)), "16-byte aligned")
        d.p = Pp.ptr
        if t is not None:
            t.base = base + 2
            refused(lib.egk_optim_step_ema(S(), C.byref(d), tp, C.byref(e)), "multiple of 4")
            t.base = base
        G.check()
        assert bump.view.tolist() == [107], "a refused call moved the offset word"
    out = dict(p=Pp, hi=hi, ema=EM)
    for k, x in (("state0", S0), ("state1", S1), ("lo", lo16)):
        if x is not None:
            out[k] = x
    return out


@case("egk_ema_swap", variants=[dict(n=3), dict(n=1003), dict(n=1024), dict(n=4099), dict(n=0)])
def ema_swap(lib, ops, G, n):
    """p <-> ema over [0, n): below one 16-byte access, a scalar tail, whole blocks; twice restores both."""
    gn = gen(n + 31)
    p0, e0 = torch.randn(n, generator=gn), torch.randn(n, generator=gn)
    Pp, EM = G.v("p", n, f32, init=p0), G.v("ema", n, f32, init=e0)
    ok(lib.egk_ema_swap(S(), Pp.ptr, EM.ptr, n), "egk_ema_swap")
    G.check()
    same(Pp.view, e0, "p")
    same(EM.view, p0, "ema")
    if n > 4:
        refused(lib.egk_ema_swap(S(), Pp.ptr + 4, EM.ptr, n - 4), "16-byte aligned")
        refused(lib.egk_ema_swap(S(), Pp.ptr, EM.ptr + 8, n - 4), "16-byte aligned")
        refused(lib.egk_ema_swap(S(), Pp.ptr, EM.ptr, -1), "n >= 0")
        G.check()
        same(Pp.view, e0, "p after refused calls")
    ok(lib.egk_ema_swap(S(), Pp.ptr, EM.ptr, n), "egk_ema_swap")
    G.check()
    same(Pp.view, p0, "p swapped back")
    same(EM.view, e0, "ema swapped back")
    ok(lib.egk_ema_swap(S(), Pp.ptr, EM.ptr, n), "egk_ema_swap")
    return dict(p=Pp, ema=EM)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_ema(name, fn, variant, covers, plain):
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
