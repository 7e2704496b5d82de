"""Guard-band tests of include/egopack_mixup.h: each of the two launches touches only what its arguments name.

The form of tests/test_gpu_bounds_action.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is registered
there): every device argument sits in a sentinel-filled window -- NaN in the guard rows and in the padding columns of the inputs (a
read beyond a window puts a NaN into the result), ``src`` / ``lam`` / ``y`` / ``y_b`` between guards, the outputs with row strides
above the minimum and a sentinel between the rows.  The results are held to the float64 models of tests/mixup_common.py, everything
outside the windows keeps its bits -- columns [cols, ld) of ``x_out`` and the ``y_b`` / ``lam`` inputs included --, and a second run on
plain buffers gives the same bits.  The ledger of this header is tests/test_cabi_addons.py; the module imports without a GPU."""
import pytest
import torch

from tests import mixup_common as MC
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, S, bf16, f32, i32, i64, ok, refused, same

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
OUT16 = 2.0 ** -8  # the one rounding of a bf16 output, relative: half a unit (2^-7 of the leading bit) in the last of its 8 significand bits


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


@case("egk_mix_rows_multi",
      variants=[dict(rows=(67, 5, 9), cols=1536, dt=bf16, pad=8), dict(rows=(67, 5, 9), cols=40, dt=f32, pad=4),
                dict(rows=(5,), cols=43, dt=bf16, pad=3), dict(rows=(1,), cols=1, dt=f32, pad=1),
                dict(rows=(0, 5), cols=40, dt=f32, pad=0), dict(rows=(0,), cols=40, dt=f32, pad=4, plain=False)])
def mix_rows(lib, ops, G, rows, cols, dt, pad):
    """Segment 1 of a launch with several is a plain copy (NULL src / lam)."""
    g = MC.gen(sum(rows) * 13 + cols)
    segs, call = [], []
    for i, r in enumerate(rows):
        x = B.r16(torch.randn(r, cols, generator=g) * 2)
        copy = i == 1 and len(rows) > 2
        src = torch.randperm(r, generator=g).to(i32)
        lam = torch.rand(r, generator=g)
        if r > 2:
            lam[1], lam[2] = 1.0, 0.0
        X = G.m(f"x_in{i}", r, cols, dt, pad=pad, init=x)
        O = G.m(f"x_out{i}", r, cols, dt, pad=pad + (0 if pad % 4 else 4))
        SR = None if copy else G.v(f"src{i}", r, i32, init=src, poison=0)
        LM = None if copy else G.v(f"lam{i}", r, f32, init=lam)
        segs.append(dict(x=x, src=None if copy else src, lam=None if copy else lam, X=X, O=O, SR=SR, LM=LM))
        call.append((X.ptr, O.ptr, X.ld, O.ld, r, None if copy else SR.ptr, None if copy else LM.ptr))
    ok(MC.call_mix_rows(lib, call, cols, B.edt(dt), S()), "egk_mix_rows_multi")
    G.check()  # (columns [cols, ld) of every x_out among the rest)
    out = {}
    for i, s in enumerate(segs):
        exact, bound = MC.mix_model(s["x"], s["src"], s["lam"]), MC.mix_bound(s["x"], s["src"], s["lam"])
        got = s["O"].view.double().cpu()
        if dt == f32:
            assert bool(((got - exact).abs() <= bound).all()), f"segment {i}: beyond 3 * 2^-24 (|lam a| + |(1 - lam) b|)"
        else:  # the f32 value within its bound, then the one rounding of the store: at most 2^-8 relative, of a value that close
            assert bool(((got - exact).abs() <= bound + OUT16 * (exact.abs() + bound)).all()), f"segment {i}: beyond the f32 bound and one bf16 rounding"
        if s["src"] is not None:
            same(s["SR"].view, s["src"], f"src{i} is read, never written")
            same(s["LM"].view.view(torch.int32), s["lam"].view(torch.int32), f"lam{i} is read, never written")
        same(s["X"].view.float(), s["x"], f"x_in{i} is read, never written")
        out[f"x_out{i}"] = s["O"]
    before = [s["O"].bits() for s in segs]
    alt = lambda i, **kw: [tuple(kw.get(k, v) for k, v in zip(("xin", "out", "ld_in", "ld_out", "rows", "src", "lam"), c)) if j == i else c
                           for j, c in enumerate(call)]
    refused(MC.call_mix_rows(lib, alt(0, ld_in=cols - 1), cols, B.edt(dt), S()), "egk_mix_rows_multi: ld_in >= cols")
    refused(MC.call_mix_rows(lib, alt(0, ld_out=cols - 1), cols, B.edt(dt), S()), "egk_mix_rows_multi: ld_out >= cols")
    refused(MC.call_mix_rows(lib, alt(0, out=call[0][0]), cols, B.edt(dt), S()), "out of place")
    refused(MC.call_mix_rows(lib, call, 0, B.edt(dt), S()), "egk_mix_rows_multi: cols must be >= 1")
    refused(MC.call_mix_rows(lib, call, cols, 6, S()), "egk_mix_rows_multi: unknown element dtype")
    refused(MC.call_mix_rows(lib, call * 5, cols, B.edt(dt), S()), "egk_mix_rows_multi: 1 .. 4 segments")
    if call[0][5] is not None:
        refused(MC.call_mix_rows(lib, alt(0, lam=None), cols, B.edt(dt), S()), "egk_mix_rows_multi: src is given without lam")
    G.check()
    for s, b in zip(segs, before):
        assert torch.equal(b, s["O"].bits()), "a refused call wrote x_out"
    return out


@case("egk_ce_mix_fused_multi",
      variants=[dict(rows=(67, 5), Cs=((115, 478), (513,)), dt=bf16, sm=0.1, scale=True), dict(rows=(67, 5), Cs=((115, 478), (2,)), dt=f32, sm=0.0, scale=False),
                dict(rows=(1,), Cs=((2, 513),), dt=f32, sm=0.1, scale=True), dict(rows=(0, 5), Cs=((7,), (20, 9)), dt=f32, sm=0.1, scale=False),
                dict(rows=(0,), Cs=((7,),), dt=f32, sm=0.0, scale=False, plain=False)])
def ce_mix(lib, ops, G, rows, Cs, dt, sm, scale):
    g = MC.gen(sum(rows) * 7 + Cs[0][0])
    tasks, call = [], []
    for i, (r, cs) in enumerate(zip(rows, Cs)):
        n = len(cs)
        logits = [torch.randn(r, c, generator=g) * 3 for c in cs]
        y, yb = MC.mix_labels(r, cs, g)
        lam = torch.rand(r, generator=g)
        if r > 2:
            lam[1], lam[2] = 1.0, 0.0
        pads = [c + 3 for c in cs]
        dcol, col = [], 3
        for p in pads:
            dcol.append(col)
            col += p + 2  # two sentinel columns between the blocks
        L = [G.m(f"t{i}.logits{h}", r, cs[h], f32, pad=4, init=logits[h]) for h in range(n)]
        Y = G.v(f"t{i}.y", r * (n + 1), i64, init=y, poison=0)
        YB = G.v(f"t{i}.y_b", r * (n + 1), i64, init=yb, poison=0)
        LM = G.v(f"t{i}.lam", r, f32, init=lam)
        loss = G.v(f"t{i}.loss", r, f32)
        D = G.m(f"t{i}.dlogits", r, col, dt, pad=5)
        SC = G.v(f"t{i}.scale", 1, f32, init=torch.tensor([0.5 + 0.25 * i])) if scale else None
        gs = 0.37 + 0.1 * i
        tasks.append(dict(logits=logits, y=y, yb=yb, lam=lam, cs=cs, pads=pads, dcol=dcol, D=D, loss=loss, Y=Y, YB=YB, LM=LM,
                          g=gs * (0.5 + 0.25 * i) if scale else gs))
        call.append(dict(logits=[(L[h].ptr, L[h].ld, cs[h], pads[h], dcol[h]) for h in range(n)], y=Y.ptr, y_b=YB.ptr, y_stride=n + 1, lam=LM.ptr,
                         loss=loss.ptr, dlogits=D.ptr, ldd=D.ld, rows=r, gscale=gs, scale=SC.ptr if scale else None))
    ok(MC.call_ce_mix(lib, call, sm, B.edt(dt), S()), "egk_ce_mix_fused_multi")
    G.check()
    out = {}
    for i, t in enumerate(tasks):
        ref_loss, ref_grad = MC.ce_mix_model(t["logits"], t["y"], t["yb"], t["lam"], sm, t["g"])
        B.close(t["loss"].view, ref_loss.float(), f"task {i} loss", rtol=1e-5, atol=1e-5)  # test_cross_entropy_heads_ignore_index
        inside = torch.zeros(t["D"].cols, dtype=torch.bool)
        for h, c in enumerate(t["cs"]):
            c0, pd = t["dcol"][h], t["pads"][h]
            inside[c0:c0 + pd] = True
            B.close(t["D"].view[:, c0:c0 + c], ref_grad[h].float(), f"task {i} dlogits head {h}",
                    **(B.OUT16 if dt == bf16 else dict(rtol=1e-4, atol=1e-6)))
            assert not t["D"].view[:, c0 + c:c0 + pd].float().ne(0).any(), f"task {i} head {h}: pad columns [C, pad) are not zero"
        keep = t["D"].is_sentinel()[:, ~inside]
        assert bool(keep.all()), f"task {i}: {int((~keep).sum())} element(s) outside every head's column block were written"
        same(t["YB"].view, t["yb"].reshape(-1), f"task {i}: y_b is read, never written")
        same(t["Y"].view, t["y"].reshape(-1), f"task {i}: y is read, never written")
        same(t["LM"].view.view(torch.int32), t["lam"].view(torch.int32), f"task {i}: lam is read, never written")
        out[f"loss{i}"], out[f"dlogits{i}"] = t["loss"], t["D"]
    before = [t["D"].bits() for t in tasks]
    alt = lambda **kw: [dict(call[0], **kw)] + call[1:]
    refused(MC.call_ce_mix(lib, alt(y_b=None), sm, B.edt(dt), S()), "egk_ce_mix_fused_multi: null pointer (y or y_b")
    refused(MC.call_ce_mix(lib, alt(lam=None), sm, B.edt(dt), S()), "egk_ce_mix_fused_multi: null pointer (lam")
    refused(MC.call_ce_mix(lib, alt(dlogits=None), sm, B.edt(dt), S()), "egk_ce_mix_fused_multi: null pointer (loss or dlogits")
    refused(MC.call_ce_mix(lib, alt(rows=-1), sm, B.edt(dt), S()), "egk_ce_mix_fused_multi: rows must be >= 0")
    refused(MC.call_ce_mix(lib, alt(lam=call[0]["lam"] + 2), sm, B.edt(dt), S()), "not 4-byte aligned")
    refused(MC.call_ce_mix(lib, call * 5, sm, B.edt(dt), S()), "egk_ce_mix_fused_multi: 1 .. 4 tasks")
    refused(MC.call_ce_mix(lib, call, sm, 8, S()), "egk_ce_mix_fused_multi: unknown activation dtype")
    G.check()
    for t, b in zip(tasks, before):
        assert torch.equal(b, t["D"].bits()), "a refused call wrote dlogits"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_mixup(name, fn, variant, covers, plain):
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
