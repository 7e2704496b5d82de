"""Guard-band tests of include/egopack_bootstrap.h: each of the two launches touches only what its arguments name.

The form of tests/test_gpu_bounds_edge_drop.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is registered
there): every device argument sits in a sentinel-filled window.  ``num`` / ``den`` have pad columns (``ld > M``) and guard rows that
hold a huge value, the sentinel of ``cluster`` is a cluster of the batch and the one of the label matrix a class, so a read that leaves
a window moves a sum; the label is a strided column of a wider matrix; the accumulators start from non-zero values (the launch ADDS)
and sit between guards of a value no sum produces.  Outputs are held to the host model of tests/bootstrap_common.py exactly;
everything outside the windows keeps its bits, the inputs too, and a second run on plain buffers gives the same bits.  Every refusal
returns its own message and writes nothing.  The ledger of this header is tests/test_cabi_addons.py; the module imports without a GPU."""
import numpy as np
import pytest
import torch

from tests import bootstrap_common as BC
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, P, S, i64, ok, refused, same, u8

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
KEY = BC.key(0xB007)
HUGE, STRAY = 1 << 50, -(1 << 44) - 7  # outside the inputs' windows / outside the accumulators' windows


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


def _inputs(rows, M, C, seed):
    g = np.random.default_rng(seed)
    cluster = g.integers(0, max(rows // 3, 1), rows)
    cluster[g.random(rows) < 0.1] = -1 - g.integers(0, 5)
    cluster[0] = BC.MAX_CLUSTER
    den = g.integers(0, 3, (rows, M))
    num = g.integers(0, 4, (rows, M)) * (den != 0)
    num[g.integers(0, rows), g.integers(0, M)] = 1 << 40
    label = g.integers(-1, max(C, 1) + 2, (rows, 3))  # (-1 and >= C among them)
    return cluster, num, den, label


@case("egk_bootstrap_accumulate",
      variants=[dict(rows=257, M=5, R=5, C=11, cc=1, pad=3), dict(rows=300, M=8, R=5, C=1024, cc=7, pad=1),
                dict(rows=63, M=1, R=5, C=0, cc=-1, pad=2), dict(rows=1000, M=5, R=9, C=478, cc=0, pad=0)])
def accumulate(lib, ops, G, rows, M, R, C, cc, pad):
    cluster, num, den, label = _inputs(rows, M, C, rows + M)
    g = np.random.default_rng(R + C)
    start = {k: g.integers(-1000, 1000, (R, M if k.startswith("acc") else max(C, 1))) for k in ("acc_num", "acc_den", "cls_num", "cls_den")}
    CL = G.v("cluster", rows, i64, init=torch.from_numpy(cluster), poison=int(cluster[1]) if cluster[1] >= 0 else 0)
    N = G.m("num", rows, M, i64, pad=pad, init=torch.from_numpy(num), poison=HUGE)
    D = G.m("den", rows, M, i64, pad=pad, init=torch.from_numpy(den), poison=HUGE)
    L = G.m("label (a strided column)", rows, 3, i64, init=torch.from_numpy(label), poison=0)
    AN, AD = (G.v(k, R * M, i64, init=torch.from_numpy(start[k]), poison=STRAY) for k in ("acc_num", "acc_den"))
    CN, CD = (G.v(k, R * max(C, 1), i64, init=torch.from_numpy(start[k]), poison=STRAY) for k in ("cls_num", "cls_den"))
    on = cc >= 0
    call = lambda **kw: lib.egk_bootstrap_accumulate(  # noqa: E731
        S(), kw.get("cluster", P(CL)), kw.get("num", P(N)), kw.get("den", P(D)), kw.get("ld", N.ld), kw.get("rows", rows), kw.get("M", M),
        kw.get("label", P(L, 8) if on else None), L.ld, kw.get("cc", cc), kw.get("C", C), kw.get("acc_num", P(AN)), P(AD),
        kw.get("cls_num", P(CN) if on else None), P(CD) if on else None, kw.get("R", R), KEY)
    ok(call(), "egk_bootstrap_accumulate")
    G.check()
    want = {k: v.copy() for k, v in start.items()}
    if not on:
        want = {k: want[k] for k in ("acc_num", "acc_den")}
    BC.accumulate(want, cluster, num, den, KEY, label=label[:, 1], class_col=cc)
    for t, k in ((AN, "acc_num"), (AD, "acc_den"), (CN, "cls_num"), (CD, "cls_den")):
        same(t.view, torch.from_numpy(want.get(k, start[k])).reshape(-1), f"{k} against the host model" + ("" if k in want else " (class part off: untouched)"))
    for t, ref, what in ((CL, cluster, "cluster"), (N, num, "num"), (D, den, "den"), (L, label, "label")):
        same(t.view, torch.from_numpy(ref), f"{what} is read, never written")
    # every refusal has its own message and writes nothing
    before = [t.bits() for t in (AN, AD, CN, CD)]
    name = "egk_bootstrap_accumulate"
    refused(call(cluster=None), f"{name}: null cluster")
    refused(call(num=None), f"{name}: null num / den")
    refused(call(acc_num=None), f"{name}: null acc_num / acc_den")
    refused(call(rows=-1), f"{name}: rows must be >= 0")
    refused(call(rows=(1 << 24) + 1), f"{name}: more than 2^24 rows")
    refused(call(M=9, cc=-1), f"{name}: M must lie in 1..8")
    refused(call(R=0), f"{name}: R must lie in 1..65536")
    refused(call(R=65537), f"{name}: R must lie in 1..65536")
    refused(call(ld=M - 1), f"{name}: ld must be >= M")
    refused(call(cc=M), f"{name}: class_col must lie in [-1, M)")
    refused(call(cc=0, label=None), f"{name}: class_col >= 0 with a null label / cls_num / cls_den")
    if on:
        refused(call(C=1025), f"{name}: C must lie in 1..1024")
        refused(call(C=0), f"{name}: C must lie in 1..1024")
    refused(call(num=P(N, 4)), f"{name}: int64 pointers must be 8-byte aligned")
    ok(call(rows=0), name + " with rows == 0")
    G.check()
    for t, b in zip((AN, AD, CN, CD), before):
        assert torch.equal(b, t.bits()), "a refused (or empty) call wrote an output"
    return dict(acc_num=AN, acc_den=AD, cls_num=CN, cls_den=CD)


@case("egk_bootstrap_weights", variants=[dict(rows=257, R=5), dict(rows=63, R=1), dict(rows=100, R=1000), dict(rows=1, R=4)])
def weights(lib, ops, G, rows, R):
    cluster = _inputs(rows, 1, 1, rows + R)[0]
    CL = G.v("cluster", rows, i64, init=torch.from_numpy(cluster), poison=0)
    W = G.v("w", rows * R, u8)
    call = lambda **kw: lib.egk_bootstrap_weights(S(), kw.get("cluster", P(CL)), kw.get("rows", rows), kw.get("R", R), KEY, kw.get("w", P(W)))  # noqa: E731
    ok(call(), "egk_bootstrap_weights")
    G.check()
    same(W.view, torch.from_numpy(BC.weights(cluster, R, KEY)).reshape(-1), "w against the host model")
    same(CL.view, torch.from_numpy(cluster), "cluster is read, never written")
    before, name = W.bits(), "egk_bootstrap_weights"
    refused(call(cluster=None), f"{name}: null cluster")
    refused(call(w=None), f"{name}: null w")
    refused(call(rows=-1), f"{name}: rows must be >= 0")
    refused(call(R=0), f"{name}: R must lie in 1..65536")
    refused(call(cluster=P(CL, 4)), f"{name}: int64 pointers must be 8-byte aligned")
    ok(call(rows=0), name + " with rows == 0")
    G.check()
    assert torch.equal(before, W.bits()), "a refused (or empty) call wrote an output"
    return dict(w=W)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_bootstrap(name, fn, variant, covers, plain):
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
