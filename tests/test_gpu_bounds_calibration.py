"""Guard-band tests of include/egopack_calibrate.h: each of the four launches touches only what its arguments name.

The form of tests/test_gpu_bounds_topk.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is registered
there): every device argument sits in a sentinel-filled window -- NaN in the guard rows and in the padding columns of the logits
(ld = C + one 16-byte vector: a read beyond a window puts a NaN into the sums), the labels read through ``label_stride = 2`` with
an out-of-range label in the odd words, ``acc`` with its own sentinels in [6] and [7], a poison index between the rows of ``idx``,
NaN between the rows of ``prob`` and in the padding columns of ``out``.  The results are held to the host models of
tests/calibration_common.py, everything outside the windows keeps its bits, and a second run on plain buffers gives the same bits.
The ledger of this header is tests/test_cabi_addons.py; the module imports without a GPU."""
import numpy as np
import pytest
import torch

from tests import calibration_common as CM
from tests import test_gpu_bounds as B
from tests import topk_common as TK
from tests.test_gpu_bounds import Guards, S, bf16, f32, f64, i64, ok, refused, same

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
POISON = -7  # around and between the rows of idx: "no class"
ACC0 = [100, -200, 300, 400, 500, 600, 0x5EED5EED, -0x5EED5EED]  # what acc holds before the launch; [6] and [7] are never touched


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
    import ctypes
    return None if x is None else ctypes.c_void_p(int(x))


@case("egk_temp_stats",
      variants=[dict(rows=44, C=115, dt=f32, beta=1.0), dict(rows=44, C=478, dt=bf16, beta=0.5), dict(rows=9, C=513, dt=f32, beta=2.0),
                dict(rows=5, C=1030, dt=bf16, beta=1.0), dict(rows=1, C=1, dt=f32, beta=20.0), dict(rows=8200, C=2, dt=bf16, beta=0.05),
                dict(rows=0, C=115, dt=f32, beta=1.0, plain=False)])
def temp_stats(lib, ops, G, rows, C, dt, beta):
    z, y = CM.stats_problem(C, rows, dt)
    L = G.m("logits", rows, C, dt, pad=B.pad_cols(dt), init=z)
    y2 = torch.full((2 * rows,), C + 5, dtype=i64)  # (the odd words: a label the launch would count as ignored)
    y2[0::2] = y
    Y = G.v("labels", 2 * rows, i64, init=y2, poison=POISON)
    stride = 2
    BT = G.v("beta", 1, f32, init=torch.tensor([beta]))
    A = G.v("acc", 8, i64, init=torch.tensor(ACC0), poison=0)
    call = lambda **kw: lib.egk_temp_stats(S(), vp(kw.get("logits", L.ptr)), kw.get("ld", L.ld), vp(kw.get("labels", Y.ptr)), stride,
                                           kw.get("rows", rows), kw.get("C", C), vp(kw.get("beta", BT.ptr)), vp(kw.get("acc", A.ptr)),
                                           kw.get("dtype", B.edt(dt)))
    ok(call(), "egk_temp_stats")
    G.check()
    got = [int(a) - int(b) for a, b in zip(A.view.tolist(), ACC0)]
    ref = CM.sums_model(z, y, beta)
    assert got[3:] == [ref["valid"], ref["ignored"], ref["left_out"], 0, 0], (got[3:], ref)
    for i, (key, mag) in enumerate((("F", "A0"), ("F1", "A1"), ("F2", "A2"))):
        err, bound = abs(got[i] / CM.Q24 - ref[key]), CM.acc_bound(i, ref[mag], ref["counted"])
        assert err <= bound, (key, got[i] / CM.Q24, ref[key], err, bound)
    same(BT.view, torch.tensor([beta]), "beta is read, never written")
    # refused on the host, nothing launched
    before = A.bits()
    refused(call(logits=None), "egk_temp_stats: null pointer (logits)")
    refused(call(acc=A.ptr + 4), "egk_temp_stats: misaligned acc")
    refused(call(labels=Y.ptr + 4), "egk_temp_stats: misaligned labels")
    refused(call(ld=C - 1), "egk_temp_stats: ld >= C")
    refused(call(dtype=5), "egk_temp_stats: unknown logits dtype")
    G.check()
    assert torch.equal(before, A.bits()), "a refused call wrote the accumulator"
    return dict(acc=A)


@case("egk_temp_newton", variants=[dict(n=1), dict(n=3), dict(n=8)])
def temp_newton(lib, ops, G, n):
    """Hand-made sums and states: running heads on either side of the root, a frozen head, a head without rows, heads at the bounds."""
    q = lambda v: int(round(v * CM.Q24))
    heads = [  # (acc, state)
        ([q(50.0), q(-3.0), q(7.0), 40, 2, 0, 0, 0], CM.newton_init()),
        ([q(50.0), q(3.0), q(7.0), 40, 2, 0, 0, 0], [1.5, 0.5, 3.0, 1.0, 1.0, 0.0, 2.0, 0.25]),
        ([q(9.0), q(1.0), q(1.0), 7, 0, 0, 0, 0], [0.75, 0.5, 1.0, 1.0, 1.0, 1.0, 5.0, 1e-7]),       # frozen: converged
        ([0, 0, 0, 4, 9, 4, 0, 0], CM.newton_init()),                                              # every valid row left out
        ([q(5.0), q(2.0), q(0.0), 3, 0, 0, 0, 0], [CM.BETA_MIN, CM.BETA_MIN, 1.0, 0.0, 1.0, 0.0, 1.0, 0.9]),  # at beta_min
        ([q(5.0), q(-2.0), q(0.0), 3, 0, 0, 0, 0], [CM.BETA_MAX, 1.0, CM.BETA_MAX, 1.0, 0.0, 0.0, 1.0, 0.9]),  # at beta_max
        ([q(5.0), q(-2.0), q(0.0), 3, 0, 0, 0, 0], [2.0, 1.0, CM.BETA_MAX, 1.0, 0.0, 0.0, 1.0, 0.5]),  # no curvature: to the far end
        ([q(5.0), q(4.0), q(1.0), 3, 0, 0, 0, 0], [1.25, 1.0, 2.0, 1.0, 1.0, 0.0, 3.0, 0.5]),         # beyond lo, seen: the geometric mean
    ][:n]
    acc0 = torch.tensor([a for a, _ in heads], dtype=i64)
    st0 = torch.tensor([s for _, s in heads], dtype=f64)
    b0 = torch.tensor([np.float32(s[0]) for _, s in heads], dtype=f32)
    A = G.v("acc", 8 * n, i64, init=acc0, poison=1 << 40)
    ST = G.v("state", 8 * n, f64, init=st0)
    BT = G.v("beta", n, f32, init=b0)
    call = lambda **kw: lib.egk_temp_newton(S(), vp(kw.get("acc", A.ptr)), kw.get("n", n), vp(kw.get("state", ST.ptr)), vp(BT.ptr),
                                            kw.get("bmin", CM.BETA_MIN), kw.get("bmax", CM.BETA_MAX), kw.get("stop", CM.STOP))
    ok(call(), "egk_temp_newton")
    G.check()
    same(A.view, acc0.reshape(-1), "acc is read, never written")
    want_st, want_b = [], []
    for (a, s), old in zip(heads, b0.tolist()):
        ns, nb = CM.newton_step(a, s)
        want_st.append(ns)
        want_b.append(old if nb is None else nb)
    same(ST.view.view(i64), torch.tensor(want_st, dtype=f64).reshape(-1).view(i64), "state (bit for bit)")
    same(BT.view.view(torch.int32), torch.tensor(want_b, dtype=f32).view(torch.int32), "beta (bit for bit)")
    before = ST.bits()
    refused(call(n=0), "egk_temp_newton: n_heads in 1 .. 8")
    refused(call(n=9), "egk_temp_newton: n_heads in 1 .. 8")
    refused(call(state=ST.ptr + 4), "egk_temp_newton: misaligned state")
    refused(call(acc=None), "egk_temp_newton: null pointer (acc)")
    refused(call(bmin=0.0), "egk_temp_newton: beta_min > 0")
    refused(call(bmax=CM.BETA_MIN / 2), "egk_temp_newton: beta_max >= beta_min")
    refused(call(stop=-1.0), "egk_temp_newton: stop >= 0")
    G.check()
    assert torch.equal(before, ST.bits()), "a refused call wrote the state"
    return dict(state=ST, beta=BT)


def topk_prob_model(z, idx, beta):
    """(prob float64 [N, k], lse float64 [N]) of the header's definition: x = fl32(beta z), everything after it exact."""
    x = (torch.tensor(CM.beta32(beta), dtype=f32) * z.detach().cpu().float()).double()
    lse = torch.logsumexp(x, dim=1)
    C = x.shape[1]
    live = (idx >= 0) & (idx < C)
    p = torch.exp(x.gather(1, torch.where(live, idx, torch.zeros_like(idx))) - lse[:, None])
    return torch.where(live, p, torch.zeros_like(p)), lse


@case("egk_temp_topk_prob",
      variants=[dict(rows=44, C=115, k=5, dt=f32, beta=0.5, lse=True), dict(rows=44, C=478, k=5, dt=bf16, beta=2.0, lse=False),
                dict(rows=5, C=513, k=16, dt=f32, beta=1.0, lse=True), dict(rows=3, C=7, k=64, dt=bf16, beta=20.0, lse=True),
                dict(rows=1, C=1, k=1, dt=f32, beta=0.05, lse=True), dict(rows=0, C=115, k=5, dt=f32, beta=1.0, lse=True, plain=False)])
def temp_topk_prob(lib, ops, G, rows, C, k, dt, beta, lse):
    z, _ = CM.stats_problem(C, rows, dt)
    idx = torch.from_numpy(TK.topk_order(TK.widen(z), k)) if rows else torch.zeros((0, k), dtype=i64)
    L = G.m("logits", rows, C, dt, pad=B.pad_cols(dt), init=z)
    I = G.m("idx", rows, k, i64, pad=3, init=idx, poison=POISON)
    P = G.m("prob", rows, k, f32, pad=2)
    E = G.v("lse", rows, f32) if lse else None
    BT = G.v("beta", 1, f32, init=torch.tensor([beta]))
    call = lambda **kw: lib.egk_temp_topk_prob(S(), vp(kw.get("logits", L.ptr)), kw.get("ld", L.ld), rows, kw.get("C", C), vp(BT.ptr),
                                               vp(kw.get("idx", I.ptr)), kw.get("istride", I.ld), kw.get("k", k), vp(kw.get("prob", P.ptr)),
                                               kw.get("pstride", P.ld), vp(E.ptr) if lse else None, kw.get("dtype", B.edt(dt)))
    ok(call(), "egk_temp_topk_prob")
    G.check()
    same(I.view, idx, "idx is an input: never written")
    p64, lse64 = topk_prob_model(z, idx, beta)
    B.close(P.view, p64, "prob", **TK.PROB_TOL)
    if lse:
        B.close(E.view, lse64, "lse", **TK.PROB_TOL)
    if rows and k > C:
        assert bool((P.view[:, C:] == 0).all()), "an entry without a class has probability 0"
    before = P.bits()
    refused(call(k=0), "egk_temp_topk_prob: k in 1 .. 64")
    refused(call(k=65), "egk_temp_topk_prob: k in 1 .. 64")
    refused(call(idx=I.ptr + 4), "egk_temp_topk_prob: misaligned idx")
    refused(call(idx=None), "egk_temp_topk_prob: null pointer (idx)")
    refused(call(istride=k - 1), "egk_temp_topk_prob: idx row stride")
    refused(call(pstride=k - 1), "egk_temp_topk_prob: prob row stride")
    refused(call(C=0), "egk_temp_topk_prob: C >= 1")
    refused(call(ld=C - 1), "egk_temp_topk_prob: ld >= C")
    G.check()
    assert torch.equal(before, P.bits()), "a refused call wrote the probabilities"
    out = dict(prob=P)
    if lse:
        out["lse"] = E
    return out


@case("egk_temp_scale_rows",
      variants=[dict(rows=44, C=115, dt=f32, beta=0.5), dict(rows=9, C=513, dt=bf16, beta=3.0), dict(rows=1, C=1, dt=f32, beta=20.0),
                dict(rows=8200, C=2, dt=bf16, beta=0.3), dict(rows=0, C=115, dt=f32, beta=1.0, plain=False)])
def temp_scale_rows(lib, ops, G, rows, C, dt, beta):
    z, _ = CM.stats_problem(C, rows, dt)
    L = G.m("logits", rows, C, dt, pad=B.pad_cols(dt), init=z)
    O = G.m("out", rows, C, f32, pad=3)
    BT = G.v("beta", 1, f32, init=torch.tensor([beta]))
    call = lambda **kw: lib.egk_temp_scale_rows(S(), vp(kw.get("logits", L.ptr)), kw.get("ld", L.ld), rows, C, vp(kw.get("beta", BT.ptr)),
                                                vp(kw.get("out", O.ptr)), kw.get("ldo", O.ld), kw.get("dtype", B.edt(dt)))
    ok(call(), "egk_temp_scale_rows")
    G.check()
    want = torch.tensor(CM.beta32(beta), dtype=f32) * z.float()  # (one f32 product per element)
    same(O.view.view(torch.int32), want.view(torch.int32), "out (exact)")
    before = O.bits()
    refused(call(ldo=C - 1), "egk_temp_scale_rows: ldo >= C")
    refused(call(ld=C - 1), "egk_temp_scale_rows: ld >= C")
    refused(call(beta=None), "egk_temp_scale_rows: null pointer (beta)")
    refused(call(out=O.ptr + 2), "egk_temp_scale_rows: misaligned beta or out")
    refused(call(dtype=7), "egk_temp_scale_rows: unknown logits dtype")
    G.check()
    assert torch.equal(before, O.bits()), "a refused call wrote the output"
    return dict(out=O)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_calibration(name, fn, variant, covers, plain):
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
