"""Guard-band tests of include/egopack_lamb.h: each of the three launches touches only what its arguments name.

The form of tests/test_gpu_bounds_ema.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is registered
there): every pointer argument -- the five tables included -- sits in a sentinel-filled window, ``part``, ``trust`` and ``norms``
have exactly their stated size, the results are held to the float64 model of tests/lamb_common.py, everything outside the windows
(and, inside them, outside the launch's range) keeps its bits, and a second run on plain buffers gives the same bits.  The ledger
of this header is tests/test_cabi_lamb.py; the module imports without a GPU."""
import numpy as np
import pytest
import torch

from tests import ema_common as E
from tests import lamb_common as L
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, S, bf16, f32, f64, i32, i64, ok, refused, same

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
    """Every entry point some case declares it covers (the ledger in tests/test_cabi_lamb.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


def _start(gdt):
    """The problem one model step in (non-zero moments), and the step the launches take: (p, g, m, v as f32 numpy, hyper of t = 2)."""
    pr = L.problem()
    p, m, v, _, _ = L.lamb_model(pr["p"], pr["g"][0], pr["m"], pr["v"], pr["begin"], L.SLOT_GROUP, L.GROUPS, L.hyper(1))
    g = pr["g"][1]
    if gdt == bf16:
        g = torch.from_numpy(g).to(bf16).float().numpy()
    return pr, p.astype(np.float32), g, m.astype(np.float32), v.astype(np.float32), L.hyper(2)


def _tables(G, ptr):
    """The five tables in windows; returns the host copies (lamb_common.tables' dict without device tensors)."""
    begin, piece0, pieces = L.piece_table(L.SIZES)
    gh = torch.zeros(len(L.GROUPS), 4)
    gh[:, :2] = torch.tensor(L.GROUPS)
    SB = G.v("slot_begin", len(begin), i64, init=torch.tensor(begin), poison=1 << 40)
    SP = G.v("slot_piece0", len(piece0), i32, init=torch.tensor(piece0, dtype=torch.int32), poison=1 << 20)
    SG = G.v("slot_group", len(L.SLOT_GROUP), i32, init=torch.tensor(L.SLOT_GROUP, dtype=torch.int32), poison=1)
    GH = G.v("group_hyper", gh.numel(), f32, init=gh.reshape(-1))
    ptr.update(slot_begin=SB.ptr, slot_piece0=SP.ptr, slot_group=SG.ptr, group_hyper=GH.ptr)
    return dict(begin=begin, piece0=piece0, pieces=pieces, group_hyper=gh)


# ranges over the 21040 elements of lamb_common.SIZES: everything; whole slots; whole pieces inside a slot; a front cut of the piece
# [4128, 8224); a back cut of [12328, 16424), the whole piece [16424, 16432) and a front cut of [16432, 20528)
RANGES = {"all": (0, 21040), "slots": (32, 8232), "pieces": (8232, 16424), "front": (4128, 6000), "back": (14000, 20520)}


@case("egk_lamb_moments",
      variants=[dict(rng="all", gdt=f32), dict(rng="all", gdt=bf16, gate=1), dict(rng="all", gdt=f32, gate=0),
                dict(rng="slots", gdt=f32), dict(rng="pieces", gdt=bf16), dict(rng="front", gdt=f32, gate=1),
                dict(rng="back", gdt=bf16), dict(rng="back", gdt=f32, gate=0)])
def lamb_moments(lib, ops, G, rng, gdt, gate=None):
    pr, p0, g0, m0, v0, hy = _start(gdt)
    lo, hi = RANGES[rng]
    n, ptr = pr["total"], {}
    T = _tables(G, ptr)
    Pp, Gg = G.v("p", n, f32, init=torch.from_numpy(p0)), G.v("g", n, gdt, init=torch.from_numpy(g0))
    M, V = G.v("m", n, f32, init=torch.from_numpy(m0)), G.v("v", n, f32, init=torch.from_numpy(v0))
    H = G.v("hyper", 4, f32, init=torch.from_numpy(hy))
    part = G.v("part", T["piece0"][-1] * 4, f64)  # (exactly pieces x 2 halves x {P, U}: no slack)
    bump = G.v("bump_word", 1, i64, init=torch.tensor([100]), poison=0)
    gt = G.v("gate", 1, i32, init=torch.tensor([gate]), poison=1) if gate is not None else None
    ptr.update(p=Pp.ptr, g=Gg.ptr, m=M.ptr, v=V.ptr, hyper=H.ptr, part=part.ptr)
    ok(L.moments(lib, S(), ptr, T, lo, hi, g_dtype=1 if gdt == bf16 else 0, gate=gt.ptr if gt is not None else None, bump_word=bump.ptr,
                 bump=7), "egk_lamb_moments")
    G.check()
    assert bump.view.tolist() == [107], "bump_word"
    same(Pp.view, torch.from_numpy(p0), "p is read, never written")
    q0, nq, _ = L.piece_range(T["pieces"], lo, hi)
    written = ~part.is_sentinel().reshape(-1, 2, 2).cpu()
    if gate == 0:  # a closed gate: nothing but *bump_word changes
        same(M.view, torch.from_numpy(m0), "m")
        same(V.view, torch.from_numpy(v0), "v")
        assert not bool(written.any()), "a closed gate wrote partial sums"
    else:
        _, m1, v1, _, _ = L.lamb_model(p0, g0, m0, v0, pr["begin"], L.SLOT_GROUP, L.GROUPS, hy)
        got_m, got_v = M.view.cpu().numpy(), V.view.cpu().numpy()
        assert np.array_equal(got_m[:lo], m0[:lo]) and np.array_equal(got_m[hi:], m0[hi:]), "m outside [lo, hi) changed"
        assert np.array_equal(got_v[:lo], v0[:lo]) and np.array_equal(got_v[hi:], v0[hi:]), "v outside [lo, hi) changed"
        assert L.within(got_m[lo:hi], m1[lo:hi], **L.TOL) and L.within(got_v[lo:hi], v1[lo:hi], **L.TOL) and not np.array_equal(got_m, m0)
        # which halves were written: half 0 where the range holds the piece's first element, half 1 where it starts inside it;
        # a whole piece zeroes half 1; pieces the range does not meet keep the sentinel
        pcs = T["pieces"]
        for q in range(len(pcs) - 1):
            met = q0 <= q < q0 + nq
            front, back = met and lo <= pcs[q], met and hi >= pcs[q + 1]
            want = [bool(front), bool(met and (not front or back))]
            assert written[q].all(dim=1).tolist() == want and written[q].any(dim=1).tolist() == want, (q, written[q].tolist(), want)
        # the sums of the range's part of every piece, against f64 sums of the model's u
        vals = part.view.cpu().numpy().reshape(-1, 2, 2)
        wd = np.concatenate([np.full(s, L.f32(L.GROUPS[g][1])) for s, g in zip(L.SIZES, L.SLOT_GROUP)])
        u = (m1 / float(hy[1])) / (np.sqrt(v1) / float(hy[2]) + L.f32(L.EPS)) + wd * p0.astype(np.float64)
        for q in range(q0, q0 + nq):
            a, b = max(pcs[q], lo), min(pcs[q + 1], hi)
            half = 0 if a == pcs[q] else 1
            P, U = float(np.sum(p0[a:b].astype(np.float64) ** 2)), float(np.sum(u[a:b] ** 2))
            assert abs(vals[q, half, 0] - P) <= 1e-12 * P and abs(vals[q, half, 1] - U) <= 2e-6 * U, (q, vals[q, half], P, U)
            if a == pcs[q] and b == pcs[q + 1]:
                assert vals[q, 1].tolist() == [0.0, 0.0]
    # refused on the host, nothing launched
    ptr["m"] = M.ptr + 4
    refused(L.moments(lib, S(), ptr, T, lo, hi), "16-byte aligned")
    ptr["m"] = M.ptr
    refused(L.moments(lib, S(), ptr, T, lo + 4, hi), "multiples of 8")
    refused(lib.egk_lamb_moments(S(), L.vp(ptr["p"]), L.vp(ptr["g"]), 0, L.vp(ptr["m"]), L.vp(ptr["v"]), 4136, 4144, 1, 1, 0,
                                 L.vp(ptr["slot_begin"]), L.vp(ptr["slot_piece0"]), L.vp(ptr["slot_group"]), len(L.SIZES),
                                 L.vp(ptr["group_hyper"]), len(L.GROUPS), L.vp(ptr["hyper"]), L.B1, L.B2, L.EPS, L.vp(ptr["part"]), None,
                                 L.vp(bump.ptr), 7), "shorter than a piece")
    G.check()
    assert bump.view.tolist() == [107], "a refused call moved the offset word"
    return dict(m=M, v=V, part=part)


@case("egk_lamb_trust", variants=[dict(), dict(clip=1), dict(adapt=1), dict(gate=1, clip=1, adapt=1), dict(gate=0)])
def lamb_trust(lib, ops, G, clip=0, adapt=0, gate=None):
    """From partial sums of its own: slot 0 has P = 0, slot 1 (wd 0) U = 0, slot 4 (wd 0) both positive, slot 3 a ratio above 1."""
    ptr = {}
    T = _tables(G, ptr)
    npc, ns = T["piece0"][-1], len(L.SIZES)
    gn = torch.Generator().manual_seed(11)
    vals = torch.rand(npc, 2, 2, generator=gn, dtype=f64) + 0.5
    vals[:, :, 0] *= 40.0  # (P well above U: ratios above 1)
    vals[T["piece0"][2], :, 0] *= 1e-3  # slot 2: a ratio below 1
    vals[T["piece0"][0], :, 0] = 0.0
    vals[T["piece0"][1], :, 1] = 0.0
    part = G.v("part", npc * 4, f64, init=vals.reshape(-1))
    TR, NR = G.v("trust", ns, f32), G.v("norms", 2 * ns, f64)  # (exactly one word and one pair per slot)
    gt = G.v("gate", 1, i32, init=torch.tensor([gate]), poison=1) if gate is not None else None
    ptr.update(part=part.ptr, trust=TR.ptr, norms=NR.ptr)
    ok(L.trust(lib, S(), ptr, T, clip, adapt, gate=gt.ptr if gt is not None else None), "egk_lamb_trust")
    G.check()
    same(part.view, vals.reshape(-1), "part is read, never written")
    if gate == 0:
        assert bool(TR.is_sentinel().all()) and bool(NR.is_sentinel().all()), "a closed gate wrote trust or norms"
    else:
        got_t, got_n = TR.view.cpu().numpy(), NR.view.cpu().numpy().reshape(-1, 2)
        for s in range(ns):
            P = float(vals[T["piece0"][s]:T["piece0"][s + 1], :, 0].sum())
            U = float(vals[T["piece0"][s]:T["piece0"][s + 1], :, 1].sum())
            wd = L.GROUPS[L.SLOT_GROUP[s]][1]
            want = 1.0 if ((wd == 0.0 and not adapt) or P == 0.0 or U == 0.0) else L.f32(np.sqrt(P) / np.sqrt(U))
            want = min(want, 1.0) if clip else want
            assert abs(got_n[s, 0] - np.sqrt(P)) <= 1e-13 * np.sqrt(P) and abs(got_n[s, 1] - np.sqrt(U)) <= 1e-13 * np.sqrt(U), (s, got_n[s])
            assert abs(float(got_t[s]) - want) <= 1.2e-7 * want, (s, float(got_t[s]), want)  # (one f32 ulp: the f64 sums' order)
        assert got_t[0] == 1.0 and got_t[1] == 1.0 and (got_t[4] == 1.0) == (not adapt or bool(clip)) and (got_t[3] > 1.0) == (not clip) and got_t[2] < 1.0
    ptr["norms"] = NR.ptr + 4
    refused(L.trust(lib, S(), ptr, T), "misaligned part, norms")
    ptr["norms"] = NR.ptr
    G.check()
    return dict(trust=TR, norms=NR)


@case("egk_lamb_apply",
      variants=[dict(), dict(lo=False), dict(gate=1, ema=True), dict(ema=True, warmup=1, lo=False), dict(gate=0, ema=True)])
def lamb_apply(lib, ops, G, lo=True, gate=None, ema=False, warmup=0):
    pr, p0, g0, m0, v0, hy = _start(f32)
    n, ptr = pr["total"], {}
    T = _tables(G, ptr)
    p1, m1, v1, tr, _ = L.lamb_model(p0, g0, m0, v0, pr["begin"], L.SLOT_GROUP, L.GROUPS, hy)
    m1, v1, tr32 = m1.astype(np.float32), v1.astype(np.float32), tr.astype(np.float32)
    e0 = torch.randn(n, generator=torch.Generator().manual_seed(5))
    Pp = G.v("p", n, f32, init=torch.from_numpy(p0))
    M, V = G.v("m", n, f32, init=torch.from_numpy(m1)), G.v("v", n, f32, init=torch.from_numpy(v1))
    H, TR = G.v("hyper", 4, f32, init=torch.from_numpy(hy)), G.v("trust", len(L.SIZES), f32, init=torch.from_numpy(tr32))
    W16, LO = G.v("bf16_shadow", n, bf16), (G.v("bf16_lo_shadow", n, bf16) if lo else None)
    EM = G.v("ema", n, f32, init=e0) if ema else None
    TD = G.v("t_dev", 1, i64, init=torch.tensor([2]), poison=0)
    gt = G.v("gate", 1, i32, init=torch.tensor([gate]), poison=1) if gate is not None else None
    ptr.update(p=Pp.ptr, m=M.ptr, v=V.ptr, hyper=H.ptr, trust=TR.ptr, w16=W16.ptr, w16lo=LO.ptr if lo else None)
    call = lambda: L.apply(lib, S(), ptr, T, gate=gt.ptr if gt is not None else None, ema=EM.ptr if ema else None, ema_decay=0.9,
                           ema_warmup=warmup, t_dev=TD.ptr)
    ok(call(), "egk_lamb_apply")
    G.check()
    same(M.view, torch.from_numpy(m1), "m is read, never written")
    same(V.view, torch.from_numpy(v1), "v is read, never written")
    assert TD.view.tolist() == [2], "t_dev is read, never written"
    if gate == 0:
        same(Pp.view, torch.from_numpy(p0), "p")
        same(EM.view, e0, "ema")
        assert bool(W16.is_sentinel().all()) and (LO is None or bool(LO.is_sentinel().all())), "a closed gate wrote a bf16 copy"
    else:
        # (the model from the f32 moments the launch read: its own rounding of u and of the step only)
        got = Pp.view.cpu()
        ref, _, _, _, _ = L.lamb_model(p0, g0, m0, v0, pr["begin"], L.SLOT_GROUP, L.GROUPS, hy)
        assert L.within(got.numpy(), ref, **L.TOL) and not np.array_equal(got.numpy(), p0), L.excess(got.numpy(), ref, **L.TOL)
        assert not bool(got[torch.from_numpy(~pr["mask"])].view(torch.int32).any()), "the padding must keep its zero bits"
        hi16 = got.to(bf16)
        same(W16.view.view(torch.int16), hi16.view(torch.int16), "bf16_shadow")
        if lo:
            same(LO.view.view(torch.int16), (got - hi16.float()).to(bf16).view(torch.int16), "bf16_lo_shadow")
        if ema:
            same(EM.view, E.ema_model(e0, got, E.ema_weight(0.9, warmup, 2)), "ema")
    ptr["p"] = Pp.ptr + 8
    refused(call(), "16-byte aligned")
    ptr["p"] = Pp.ptr
    G.check()
    out = dict(p=Pp, hi=W16)
    if lo:
        out["lo"] = LO
    if ema:
        out["ema"] = EM
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_lamb(name, fn, variant, covers, plain):
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
