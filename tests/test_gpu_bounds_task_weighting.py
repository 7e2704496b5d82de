"""Guard-band tests of include/egopack_task_scale.h: the six _s head launches, egk_task_scale_prepare, egk_task_scale_grad and
egk_fill_scaled_from touch only what their arguments name.

The form of tests/test_gpu_bounds_pnr_balance.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is
registered there).  The row-dot heads run the CASE FUNCTIONS of their siblings (tests/test_gpu_bounds.py::rowdot_bce, ::rowdot_ce2,
tests/test_gpu_bounds_pnr_balance.py::rowdot_bce_w) through ``ScaledLib``: the library with every seeded sibling served by its _s
form -- the seed handed over as seed / 0.5 by value and 0.5 in a ONE-element guarded device word (a power of two: the product is the
sibling's seed exactly, so the siblings' references, tolerances, workspace sizes and refusals hold word for word; a read beside the
word brings the NaN sentinel into every gradient).  The fused cross entropies get their own cases on the siblings' helpers, with a
different power-of-two scale per task in a guarded vector.  Shapes: those of tests/test_gpu_task_weighting.py (rows 13 and 70,
heads (115, 478) and (3,), one / two / four tasks; cols 64 / 256 / 1024 x rows 1 / 13 / 70; ce2 rows 1 and 9) at ragged leading
dimensions.  The ledger of this header is in tests/test_task_weighting_cpu.py; the module imports without a GPU."""
import ctypes as C

import pytest
import torch

from tests import pnr_balance_common as PB
from tests import task_weighting_common as TW
from tests import test_gpu_bounds as B
from tests import test_gpu_bounds_class_balance as CEB
from tests import test_gpu_bounds_pnr_balance as PNRB
from tests.test_gpu_bounds import Guards, P, S, bf16, close, edt, f32, f64, gen, ok, refused, same

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
SC = 0.5    # the scale of the proxied cases: seed / SC * SC == seed in f32


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
    """Every entry point some case declares it covers (the ledger in tests/test_task_weighting_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


class ScaledLib:
    """The library with the seeded row-dot siblings served by their _s forms (see the module's docstring)."""

    def __init__(self, lib, G):
        self._lib = lib
        self.word = G.v("task scale", 1, f32, init=torch.tensor([SC]))

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def egk_rowdot_bce(self, s, f, w, b, y, lg, ls, df, ws, rows, cols, seed, dt):
        return self._lib.egk_rowdot_bce_s(s, f, w, b, y, lg, ls, df, ws, rows, cols, seed / SC, P(self.word), dt)

    def egk_rowdot_bce_w(self, s, f, w, b, y, lg, ls, df, ws, rows, cols, seed, pos, neg, gamma, dt):
        return self._lib.egk_rowdot_bce_w_s(s, f, w, b, y, lg, ls, df, ws, rows, cols, seed / SC, P(self.word), pos, neg, gamma, dt)

    def egk_rowdot_ce2(self, s, f, w, b, y, lg, ls, df, dw, db, gws, rows, cols, sm, seed, dt):
        return self._lib.egk_rowdot_ce2_s(s, f, w, b, y, lg, ls, df, dw, db, gws, rows, cols, sm, seed / SC, P(self.word), dt)

    def egk_rowdot_ce2_multi(self, s, n, f, w, b, y, lg, ls, df, dw, db, gws, rows, cols, avg, sm, seed, dt):
        return self._lib.egk_rowdot_ce2_multi_s(s, n, f, w, b, y, lg, ls, df, dw, db, gws, rows, cols, avg, sm, seed / SC, P(self.word), dt)


@case("egk_rowdot_bce_s", variants=[dict(rows=r, cols=c, dt=dt) for r, c, dt in ((1, 64, f32), (13, 256, bf16), (70, 1024, bf16), (70, 1000, f32),
                                                                                 (0, 64, f32))])
def rowdot_bce_s(lib, ops, G, rows, cols, dt):
    L = ScaledLib(lib, G)
    out = B.rowdot_bce(L, ops, G, rows, cols, dt)
    if rows:
        ws = next(g for n, g in G.items if n == "ws")
        args = [P(g) for n, g in G.items if n in ("f", "w", "bias", "y", "logits", "loss", "df")]
        refused(lib.egk_rowdot_bce_s(S(), *args, P(ws), rows, cols, 0.1, None, edt(dt)), "null pointer (scale)")
        refused(lib.egk_rowdot_bce_s(S(), *args, P(ws), rows, cols, 0.1, P(L.word, 2), edt(dt)), "scale is not 4-byte aligned")
        G.check()
    return out


@case("egk_rowdot_bce_w_s", variants=[dict(rows=r, cols=c, dt=dt, grad=grad, sh=(3.0, 0.5, 2.0))
                                      for r, c, dt in ((13, 64, f32), (70, 1000, bf16), (70, 1024, bf16)) for grad in (True, False)])
def rowdot_bce_w_s(lib, ops, G, rows, cols, dt, grad, sh):
    return PNRB.rowdot_bce_w(ScaledLib(lib, G), ops, G, rows, cols, dt, grad, sh)


@case("egk_rowdot_ce2_s", "egk_rowdot_ce2_multi_s", variants=[
    dict(n_src=1, rows=1, cols=264, dt=f32, average=0, sm=0.1, entry="single"), dict(n_src=1, rows=9, cols=1024, dt=bf16, average=0, sm=0.0, entry="single"),
    dict(n_src=3, rows=9, cols=1024, dt=bf16, average=1, sm=0.1, entry="phases"), dict(n_src=3, rows=9, cols=250, dt=f32, average=0, sm=0.1, entry="multi"),
    dict(n_src=2, rows=0, cols=64, dt=f32, average=1, sm=0.0, entry="multi")])
def rowdot_ce2_s(lib, ops, G, n_src, rows, cols, dt, average, sm, entry):
    return B.rowdot_ce2(ScaledLib(lib, G), ops, G, n_src, rows, cols, dt, average, sm, entry)


# the fused cross entropies: (rows, heads, pads) per task, one / two / four tasks; a different power-of-two scale per task
CE_TASKS = [(70, (115, 478), (128, 512)), (13, (3,), (8,)), (13, (115, 478), (128, 512)), (70, (3,), (8,))]
CE_GSCALES, CE_SCALES = (0.37, 0.25, 1.0 / 13, 1.0 / 70), (0.5, 2.0, 0.25, 1.0)


def _scale_ptrs(G, count):
    SV = G.v("task scales", count, f32, init=torch.tensor(CE_SCALES[:count]))
    return SV, (C.c_void_p * count)(*[SV.ptr + 4 * i for i in range(count)])


@case("egk_ce_fused_multi_s", variants=[dict(count=c, dt=dt, lpad=lp, dpad=dp) for c in (1, 2, 4) for dt, lp, dp in ((bf16, 0, 0), (f32, 3, 5))])
def ce_fused_multi_s(lib, ops, G, count, dt, lpad, dpad):
    g = gen(91 + count)
    tasks = [B._ce_fused_task(G, f"task{i}.", g, r, cs, pd, lpad, dpad, dt, 0.1, CE_GSCALES[i]) for i, (r, cs, pd) in enumerate(CE_TASKS[:count])]
    arr = B._ce_task_array(tasks)
    SV, ptrs = _scale_ptrs(G, count)
    ok(lib.egk_ce_fused_multi_s(S(), arr, ptrs, count, 0.1, edt(dt)), "egk_ce_fused_multi_s")
    G.check()
    out = {}
    for i, t in enumerate(tasks):
        t["gscale"] = TW.scaled_seed(CE_GSCALES[i], CE_SCALES[i])  # (the reference's seed: the product, exact for these scales)
        B._ce_fused_check(t, f"task{i}.")
        out[f"loss{i}"], out[f"dlogits{i}"] = t["loss"], t["D"]
    # refused on the host, nothing launched: no scales, a null scale, a misaligned scale, and what the sibling refuses
    refused(lib.egk_ce_fused_multi_s(S(), arr, None, count, 0.1, edt(dt)), "null pointer (scales)")
    bad = (C.c_void_p * count)(*[None if i == count - 1 else SV.ptr for i in range(count)])
    refused(lib.egk_ce_fused_multi_s(S(), arr, bad, count, 0.1, edt(dt)), "null pointer (scale of task")
    bad = (C.c_void_p * count)(*[SV.ptr + 2 for _ in range(count)])
    refused(lib.egk_ce_fused_multi_s(S(), arr, bad, count, 0.1, edt(dt)), "not 4-byte aligned")
    arr[0].pad[0] = arr[0].C[0] - 1
    refused(lib.egk_ce_fused_multi_s(S(), arr, ptrs, count, 0.1, edt(dt)), "pad must be >= C")
    G.check()
    return out


@case("egk_ce_w_fused_multi_s", variants=[dict(count=c, dt=dt, lpad=lp, dpad=dp) for c in (1, 2, 4) for dt, lp, dp in ((bf16, 0, 0), (f32, 3, 5))])
def ce_w_fused_multi_s(lib, ops, G, count, dt, lpad, dpad):
    from egopack_amd import _lib
    g = gen(191 + count)
    which = [("w", "a"), ("wa",), ("a", "w"), ("w",)]
    tasks = [CEB._task(G, f"task{i}.", g, r, cs, pd, lpad, dpad, dt, 0.1, CE_GSCALES[i], which[i]) for i, (r, cs, pd) in enumerate(CE_TASKS[:count])]
    arr = (_lib.CEWTask * count)()
    for a, t in zip(arr, tasks):
        CEB._fill(a, t)
    SV, ptrs = _scale_ptrs(G, count)
    ok(lib.egk_ce_w_fused_multi_s(S(), arr, ptrs, count, 0.1, edt(dt)), "egk_ce_w_fused_multi_s")
    G.check()
    out = {}
    for i, t in enumerate(tasks):
        t["gscale"] = TW.scaled_seed(CE_GSCALES[i], CE_SCALES[i])
        CEB._check(t, f"task{i}.")
        out[f"loss{i}"], out[f"dlogits{i}"] = t["loss"], t["D"]
    refused(lib.egk_ce_w_fused_multi_s(S(), arr, None, count, 0.1, edt(dt)), "null pointer (scales)")
    arr[0].weight[0] = tasks[0]["vec"][0][0].ptr + 2
    refused(lib.egk_ce_w_fused_multi_s(S(), arr, ptrs, count, 0.1, edt(dt)), "misaligned vector pointer")
    G.check()
    return out


@case("egk_task_scale_prepare", variants=[dict(n=n) for n in (1, 3, 7, 8)])
def task_scale_prepare(lib, ops, G, n):
    s = torch.tensor((TW.LOG_VARS + (0.5,))[:n], dtype=f32)
    Sv, SC_ = G.v("log_var", n, f32, init=s), G.v("scale", n, f32)
    ok(lib.egk_task_scale_prepare(S(), P(Sv), P(SC_), n), "egk_task_scale_prepare")
    G.check()
    ref = torch.tensor([TW.prepared_scale(v) for v in s.tolist()], dtype=f32)
    close(SC_.view, ref, "scale", rtol=1e-6, atol=0)  # (one f32 ulp: tests/test_gpu_task_weighting.py states it in ulps)
    refused(lib.egk_task_scale_prepare(S(), P(Sv), P(SC_), 9), "1..8 tasks")
    refused(lib.egk_task_scale_prepare(S(), None, P(SC_), n), "null pointer")
    G.check()
    return dict(scale=SC_)


@case("egk_task_scale_grad", variants=[dict(lens=l, learned=m) for l in ((1,), (70, None, 2048), (2048, 70, 1, 13, None, 5, 64, 1025))
                                       for m in (True, False)])
def task_scale_grad(lib, ops, G, lens, learned):
    """Vectors of 1, 70 and 2048 elements (one, a ragged fraction of a pass, two passes of the 1024 threads), absent slots, a
    compacted vector (vector 0 divides by twice its length), eight tasks."""
    n = len(lens)
    g = gen(7 * n + sum(v or 0 for v in lens))
    vecs = [None if ln is None else torch.rand(ln, generator=g) * 3 for ln in lens]
    counts = [2 * lens[0]] + [0] * (n - 1)
    w = [(1.0, 0.5, 2.0)[i % 3] for i in range(n)]
    s = torch.tensor([(0.0, 0.3, -0.7)[i % 3] for i in range(n)], dtype=f32)
    scale = torch.tensor([TW.prepared_scale(v) for v in s.tolist()], dtype=f32)
    acc0 = torch.arange(n, dtype=f64) + 0.5
    V = [None if v is None else G.v(f"loss{i}", v.numel(), f32, init=v) for i, v in enumerate(vecs)]
    Sv = G.v("log_var", n, f32, init=s) if learned else None
    SCv, DS = G.v("scale", n, f32, init=scale), (G.v("ds", n, f32) if learned else None)
    OBJ, ACC = G.v("objective", 1, f32), G.v("acc", n, f64, init=acc0)
    xs = B.ptr_array(V)
    ns = (C.c_int64 * n)(*[0 if v is None else v.numel() for v in vecs])
    cn = (C.c_int64 * n)(*counts)
    wf = (C.c_float * n)(*w)
    ok(lib.egk_task_scale_grad(S(), xs, ns, cn, wf, P(Sv), P(SCv), P(DS), P(OBJ), P(ACC), n), "egk_task_scale_grad")
    G.check()
    J, ds, sums = TW.objective(vecs, w, scale.tolist(), s.tolist() if learned else None, [c or None for c in counts])
    close(OBJ.view, torch.tensor([J], dtype=f32), "objective", rtol=1e-6, atol=1e-7)
    close(ACC.view, acc0 + torch.tensor(sums, dtype=f64), "acc", rtol=1e-6, atol=0)
    out = dict(objective=OBJ, acc=ACC)
    if learned:
        close(DS.view, torch.tensor(ds, dtype=f32), "ds", rtol=1e-6, atol=1e-7)
        out["ds"] = DS
        refused(lib.egk_task_scale_grad(S(), xs, ns, cn, wf, P(Sv), P(SCv), None, P(OBJ), P(ACC), n), "null pointer (ds")
    refused(lib.egk_task_scale_grad(S(), xs, ns, cn, wf, P(Sv), None, P(DS), P(OBJ), P(ACC), n), "null pointer")
    refused(lib.egk_task_scale_grad(S(), xs, ns, cn, wf, P(Sv), P(SCv), P(DS), P(OBJ), P(ACC), 9), "1..8 tasks")
    G.check()
    return out


@case("egk_fill_scaled_from", variants=[dict(n=n) for n in (0, 1, 70, 257, 2048)])
def fill_scaled_from(lib, ops, G, n):
    W, O = G.v("task scale", 1, f32, init=torch.tensor([0.3])), G.v("out", n, f32)
    coef = 2.0 / 70
    ok(lib.egk_fill_scaled_from(S(), P(O), n, coef, P(W)), "egk_fill_scaled_from")
    G.check()
    same(O.view, torch.full((n,), TW.scaled_seed(coef, 0.3), dtype=f32), "out")
    refused(lib.egk_fill_scaled_from(S(), P(O), n, coef, None), "null pointer")
    refused(lib.egk_fill_scaled_from(S(), P(O), -1, coef, P(W)), "n must be >= 0")
    G.check()
    return dict(out=O)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_task_weighting(name, fn, variant, covers, plain):
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
