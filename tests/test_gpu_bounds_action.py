"""Guard-band tests of include/egopack_action.h: each of the two launches touches only what its arguments name.

The form of tests/test_gpu_bounds_calibration.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is
registered there): every device argument sits in a sentinel-filled window -- NaN in the guard rows and in the padding columns of
both logits matrices (ld = C + one 16-byte vector: a read beyond a window puts a NaN into the log-sum-exp), the labels as columns
0 and 2 of one [rows, 3] matrix with a poison between them, ``pair`` / ``logp`` / ``prob`` with row strides above the minimum and a
sentinel between the rows, the optional outputs absent in one variant.  The results are held to the host model of
tests/action_common.py bit for bit (pairs, logp, rank), everything outside the windows keeps its bits, and a second run on plain
buffers gives the same bits.  The ledger of this header is tests/test_cabi_addons.py; the module imports without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import action_common as AC
from tests import test_gpu_bounds as B
from tests import topk_common as TK
from tests.test_gpu_bounds import Guards, S, bf16, f32, i32, i64, ok, refused, same

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
POISON = -7


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
    """Every entry point some case declares it covers (the ledger in tests/test_cabi_addons.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


def vp(x):
    return None if x is None else ctypes.c_void_p(int(x))


@case("egk_action_topk",
      variants=[dict(rows=9, Cv=115, Cn=478, k=5, dt=bf16, beta=None, full=True), dict(rows=9, Cv=115, Cn=478, k=5, dt=f32, beta=(0.5, 2.0), full=True),
                dict(rows=5, Cv=3, Cn=5, k=32, dt=f32, beta=None, full=True), dict(rows=3, Cv=600, Cn=1024, k=32, dt=bf16, beta=(1.0, 1.0), full=True),
                dict(rows=6, Cv=65, Cn=130, k=4, dt=f32, beta=None, full=False), dict(rows=1, Cv=1, Cn=1, k=1, dt=f32, beta=None, full=True),
                dict(rows=0, Cv=115, Cn=478, k=5, dt=f32, beta=None, full=True, plain=False)])
def action_topk(lib, ops, G, rows, Cv, Cn, k, dt, beta, full):
    """``full``: logp, prob, lse and rank (with the labels) are given; otherwise the pairs alone."""
    g = AC.gen(1000 * Cv + Cn + k)
    zv, zn = AC.grid(rows, Cv, g).to(dt), AC.grid(rows, Cn, g).to(dt)
    y = AC.pair_labels(rows, Cv, Cn, g)
    V = G.m("verb_logits", rows, Cv, dt, pad=B.pad_cols(dt), init=zv)
    N = G.m("noun_logits", rows, Cn, dt, pad=B.pad_cols(dt), init=zn)
    Y = G.m("labels", rows, 3, i64, init=y, poison=POISON) if full else None
    PR = G.m("pair", rows, 2 * k, i64, pad=3, poison=POISON)
    LP = G.m("logp", rows, k, f32, pad=2) if full else None
    PB = G.m("prob", rows, k, f32, pad=2) if full else None
    E = G.m("lse", rows, 2, f32) if full else None
    R = G.v("rank", rows, i32, poison=POISON) if full else None
    BT = G.v("beta", 2, f32, init=torch.tensor(beta)) if beta is not None else None
    opt = lambda x, off=0: None if x is None else x.ptr + off
    call = lambda **kw: lib.egk_action_topk(
        S(), vp(kw.get("verb", V.ptr)), kw.get("ld_v", V.ld), kw.get("Cv", Cv), vp(kw.get("noun", N.ptr)), kw.get("ld_n", N.ld), kw.get("Cn", Cn),
        vp(kw.get("beta", opt(BT))), vp(kw.get("yv", opt(Y))), 3, vp(kw.get("yn", opt(Y, 16))), 3, rows, kw.get("k", k),
        vp(kw.get("pair", PR.ptr)), kw.get("pstride", PR.ld), vp(opt(LP)), vp(opt(PB)), kw.get("ostride", LP.ld if full else 0), vp(opt(E)),
        vp(kw.get("rank", opt(R))), kw.get("dtype", B.edt(dt)))
    ok(call(), "egk_action_topk")
    G.check()
    znp, nnp = TK.widen(zv), TK.widen(zn)
    if full:
        lse = E.view.cpu().numpy()
        B.close(E.view, torch.from_numpy(np.stack([TK.logsumexp64(AC.scaled(znp, beta and beta[0])), TK.logsumexp64(AC.scaled(nnp, beta and beta[1]))], 1))
                if rows else torch.zeros((0, 2), dtype=torch.float64), "lse", **TK.PROB_TOL)
    else:
        lse = AC.lse32(znp, nnp, beta)  # (the pairs of a 0.25-grid row do not depend on the last bit of lse: see below)
    pair, logp, rank, _ = AC.model(znp, nnp, lse, k, labels=(y[:, 0].numpy(), y[:, 2].numpy()) if full else None, beta=beta)
    if full:
        same(PR.view.reshape(rows, k, 2), torch.from_numpy(pair), "pair (bit for bit)")
        same(LP.view.view(torch.int32), torch.from_numpy(logp).view(torch.int32), "logp (bit for bit)")
        same(R.view, torch.from_numpy(rank), "rank (exact)")
        B.close(PB.view, torch.from_numpy(AC.prob64(znp, nnp, pair, beta)), "prob", **TK.PROB_TOL)
        same(Y.view, y, "labels are read, never written")
    else:
        # without the launch's lse the scores' last bit is not known, the pairs' SCORE CLASSES are: sort both by exact probability
        got = PR.view.reshape(rows, k, 2).cpu().numpy()
        np.testing.assert_allclose(AC.prob64(znp, nnp, got, beta), AC.prob64(znp, nnp, pair, beta), rtol=1e-12, atol=0)
    before = PR.bits()
    refused(call(verb=None), "egk_action_topk: null pointer (verb_logits)")
    refused(call(pair=None), "egk_action_topk: null pointer (pair)")
    refused(call(k=0), "egk_action_topk: k in 1 .. 32")
    refused(call(k=33), "egk_action_topk: k in 1 .. 32")
    refused(call(Cv=1025), "egk_action_topk: Cv in 1 .. 1024")
    refused(call(Cn=0), "egk_action_topk: Cn in 1 .. 1024")
    refused(call(ld_v=Cv - 1), "egk_action_topk: ld_v >= Cv")
    refused(call(ld_n=Cn - 1), "egk_action_topk: ld_n >= Cn")
    refused(call(pstride=2 * k - 1), "egk_action_topk: pair row stride")
    refused(call(pair=PR.ptr + 4), "egk_action_topk: misaligned pair")
    refused(call(dtype=4), "egk_action_topk: unknown logits dtype")
    if full:
        refused(call(ostride=k - 1), "egk_action_topk: logp / prob row stride")
        refused(call(rank=None), "egk_action_topk: the labels are given for rank")
        refused(call(yn=None), "egk_action_topk: verb_labels and noun_labels")
        refused(call(yv=Y.ptr + 4), "egk_action_topk: misaligned labels")
    else:
        refused(call(rank=PR.ptr), "egk_action_topk: rank requires the labels")
    G.check()
    assert torch.equal(before, PR.bits()), "a refused call wrote the pairs"
    out = dict(pair=PR)
    if full:
        out.update(logp=LP, prob=PB, lse=E, rank=R)
    return out


@case("egk_edit_distance_pairs",
      variants=[dict(N=5, Z=20, K=5), dict(N=3, Z=1, K=2), dict(N=2, Z=64, K=3), dict(N=70, Z=7, K=1), dict(N=0, Z=20, K=5, plain=False)])
def edit_distance_pairs(lib, ops, G, N, Z, K):
    pv, pn, lv, ln = AC.futures(N, Z, K, AC.gen(100 * N + Z + K))
    PV = G.m("pred_v", N * Z, K, i64, pad=2, init=pv.reshape(N * Z, K), poison=POISON)
    PN = G.m("pred_n", N * Z, K, i64, pad=2, init=pn.reshape(N * Z, K), poison=POISON)
    LV = G.m("label_v", N, Z, i64, pad=3, init=lv, poison=POISON)
    LN = G.m("label_n", N, Z, i64, pad=3, init=ln, poison=POISON)
    O = G.v("out", N * K * 3, i32, poison=POISON)
    call = lambda **kw: lib.egk_edit_distance_pairs(S(), vp(kw.get("pv", PV.ptr)), vp(kw.get("pn", PN.ptr)), Z * PV.ld, PV.ld, 1, vp(LV.ptr),
                                                    vp(kw.get("ln", LN.ptr)), LV.ld, 1, vp(kw.get("out", O.ptr)), kw.get("N", N), kw.get("Z", Z), K)
    ok(call(), "egk_edit_distance_pairs")
    G.check()
    got = O.view.reshape(N, K, 3)
    same(got, torch.from_numpy(AC.edit_model(pv.numpy(), pn.numpy(), lv.numpy(), ln.numpy())), "distances (exact)")
    if N:
        assert bool((got[..., 2] >= got[..., :2].max(-1).values).all()), "an action matches only where verb and noun do"
    same(PV.view, pv.reshape(N * Z, K), "pred_v is read, never written")
    before = O.bits()
    refused(call(pv=None), "egk_edit_distance_pairs: null pointer (pred_v)")
    refused(call(ln=None), "egk_edit_distance_pairs: null pointer (label_n)")
    refused(call(out=None), "egk_edit_distance_pairs: null pointer (out)")
    refused(call(Z=65), "egk_edit_distance_pairs: sequence length 65")
    refused(call(N=-1), "egk_edit_distance_pairs: N >= 0")
    refused(call(pn=PN.ptr + 4), "egk_edit_distance_pairs: misaligned pred or label")
    refused(call(out=O.ptr + 2), "egk_edit_distance_pairs: misaligned out")
    G.check()
    assert torch.equal(before, O.bits()), "a refused call wrote the distances"
    return dict(out=O)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_action(name, fn, variant, covers, plain):
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
