"""Guard-band tests of include/egopack_ce_balanced.h: egk_ce_w_fwd, egk_ce_w_bwd and egk_ce_w_fused_multi touch only what their
arguments name -- the weight and offset vectors included.

The form of tests/test_gpu_bounds_ema.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is registered
there): every device argument sits in a sentinel-filled window (the NaN sentinel around an input reaches the result when a read
leaves the window; labels are surrounded by a valid class), outputs are compared with the float64 host model of
tests/class_balance_common.py, everything outside the windows must keep the sentinel bits, and a second run on plain buffers must
give the same bits.  rows = 77 (ragged for 4 waves per workgroup, ignored rows), C = 115 / 478 with pads 128 / 512 and an odd
``ldd``.  The ledger of this header is in tests/test_class_balance_cpu.py; the module imports without a GPU."""
import pytest
import torch

from tests import class_balance_common as CB
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import OUT16, Guards, P, S, bf16, close, edt, f32, f64, gen, i64, ok, refused

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
    """Every entry point some case declares it covers (the ledger in tests/test_class_balance_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


def _vectors(G, tag, Cn, which):
    """(weight window | None, offset window | None, their host values): Zipf weights with a class of weight exactly 0."""
    w = CB.zipf_weights(Cn) if which in ("w", "wa") else None
    if w is not None:
        w[Cn // 2] = 0.0
    a = CB.zipf_offsets(Cn) if which in ("a", "wa") else None
    Wv = G.v(tag + "weight", Cn, f32, init=w) if w is not None else None
    Av = G.v(tag + "offset", Cn, f32, init=a) if a is not None else None
    return Wv, Av, w, a


@case("egk_ce_w_fwd", "egk_ce_w_bwd", variants=[
    dict(rows=77, Cn=115, pad=5, ys=2, sm=0.1, dt=bf16, acc=1, which="wa"),  # bf16 dlogits with ld = 125: rows not 16-byte aligned
    dict(rows=77, Cn=478, pad=3, ys=1, sm=0.0, dt=f32, acc=0, which="w"),    # dlogits ld = 478 + 7 = 485: an odd row stride
    dict(rows=77, Cn=115, pad=0, ys=1, sm=0.1, dt=f32, acc=0, which="a"),
    dict(rows=37, Cn=2, pad=4, ys=1, sm=0.1, dt=f32, acc=0, which="wa"),
    dict(rows=0, Cn=9, pad=4, ys=1, sm=0.0, dt=f32, acc=0, which="wa")])
def ce_w(lib, ops, G, rows, Cn, pad, ys, sm, dt, acc, which):
    g = gen(rows * 7 + Cn)
    logits = torch.randn(rows, Cn, generator=g) * 3
    y = torch.randint(0, Cn, (rows, ys), generator=g)
    y[::3, 0] = -1                                                   # ignored rows
    gloss, loss0 = torch.randn(rows, generator=g), torch.randn(rows, generator=g)
    L = G.m("logits", rows, Cn, f32, pad=pad, init=logits)
    Y = G.v("y", rows * ys, i64, init=y, poison=(Cn - 1))            # (a label read beyond the list is a valid class)
    Wv, Av, w, a = _vectors(G, "", Cn, which)
    loss = G.v("loss", rows, f32, init=loss0 if acc else None)
    lse = G.v("lse", rows, f32)
    GL = G.v("gloss", rows, f32, init=gloss)
    D = G.m("dlogits", rows, Cn, dt, pad=2 * pad + 1)                # an odd leading dimension
    ok(lib.egk_ce_w_fwd(S(), P(L), L.ld, P(Y), ys, P(Wv), P(Av), P(loss), P(lse), rows, Cn, sm, acc), "egk_ce_w_fwd")
    ok(lib.egk_ce_w_bwd(S(), P(L), L.ld, P(Y), ys, P(Wv), P(Av), P(lse), P(GL), P(D), D.ld, rows, Cn, sm, edt(dt)), "egk_ce_w_bwd")
    G.check()
    ref, lref, dref = CB.model(logits, y[:, 0], w, a, sm, gloss)
    close(loss.view, (ref + (loss0.double() if acc else 0)).float(), "loss", **CB.LOSS_TOL)
    close(lse.view, lref.float(), "lse", **CB.LOSS_TOL)
    close(D.view, dref.float(), "dlogits", **(OUT16 if dt == bf16 else CB.GRAD_TOL))
    if rows:
        assert not D.view[::3].float().ne(0).any(), "ignored rows have a gradient"
        if not acc:
            assert not loss.view[::3].ne(0).any(), "ignored rows have a loss"
        # refused on the host, nothing launched
        if Wv is not None:
            refused(lib.egk_ce_w_fwd(S(), P(L), L.ld, P(Y), ys, P(Wv, 2), P(Av), P(loss), P(lse), rows, Cn, sm, acc),
                    "misaligned vector pointer")
        if Av is not None:
            refused(lib.egk_ce_w_bwd(S(), P(L), L.ld, P(Y), ys, P(Wv), P(Av, 1), P(lse), P(GL), P(D), D.ld, rows, Cn, sm, edt(dt)),
                    "misaligned vector pointer")
        refused(lib.egk_ce_w_fwd(S(), P(L), L.ld, P(Y), ys, P(Wv), P(Av), P(loss), P(lse), rows, 0, sm, acc), "C must be >= 1")
        G.check()
    return dict(loss=loss, lse=lse, dlogits=D)


def _task(G, tag, g, rows, Cs, pads, lpad, dpad, dt, sm, gscale, which):
    """One task of egk_ce_w_fused_multi (tests/test_gpu_bounds.py::_ce_fused_task) + per head the vectors ``which[h]`` names."""
    t = B._ce_fused_task(G, tag, g, rows, Cs, pads, lpad, dpad, dt, sm, gscale)
    t["vec"] = [_vectors(G, f"{tag}head{h}.", Cs[h], which[h]) for h in range(len(Cs))]
    return t


def _fill(a, t):
    b = a.base
    for h in range(t["n"]):
        b.logits[h], b.ld[h], b.C[h], b.pad[h], b.dcol[h] = t["L"][h].ptr, t["L"][h].ld, t["Cs"][h], t["pads"][h], t["dcol"][h]
        Wv, Av, _, _ = t["vec"][h]
        a.weight[h], a.offset[h] = (Wv.ptr if Wv is not None else None), (Av.ptr if Av is not None else None)
    b.n_heads, b.y, b.y_stride, b.loss, b.dlogits, b.ldd = t["n"], t["Y"].ptr, t["n"] + 1, t["loss"].ptr, t["D"].ptr, t["D"].ld
    b.rows, b.gscale = t["rows"], t["gscale"]


def _check(t, tag):
    rows, n = t["rows"], t["n"]
    total = torch.zeros(rows, dtype=f64)
    inside = torch.zeros(t["D"].cols, dtype=torch.bool)
    for h in range(n):
        _, _, w, a = t["vec"][h]
        ref, _, dref = CB.model(t["logits"][h], t["y"][:, h], w, a, t["sm"], torch.full((rows,), t["gscale"]))
        total += ref
        c0, Cn, pd = t["dcol"][h], t["Cs"][h], t["pads"][h]
        inside[c0:c0 + pd] = True
        close(t["D"].view[:, c0:c0 + Cn], dref.float(), f"{tag}dlogits head {h}", **(OUT16 if t["dt"] == bf16 else CB.GRAD_TOL))
        assert not t["D"].view[:, c0 + Cn:c0 + pd].float().ne(0).any(), f"{tag}dlogits head {h}: pad columns [C, pad) are not zero"
        dead = (t["y"][:, h] < 0)
        assert not t["D"].view[dead][:, c0:c0 + pd].float().ne(0).any(), f"{tag}dlogits head {h}: ignored rows have a gradient"
    close(t["loss"].view, total.float(), tag + "loss", **CB.LOSS_TOL)
    keep = t["D"].is_sentinel()[:, ~inside]
    assert bool(keep.all()), f"{tag}dlogits: {int((~keep).sum())} element(s) outside every head's column block were written"


@case("egk_ce_w_fused_multi", variants=[dict(dt=bf16, lpad=0, dpad=0, sm=0.1), dict(dt=f32, lpad=3, dpad=5, sm=0.1),
                                        dict(dt=f32, lpad=0, dpad=1, sm=0.0)])
def ce_w_fused_multi(lib, ops, G, dt, lpad, dpad, sm):
    """Three tasks: (115, 478) in pads (128, 512) with weights on one head and offsets on the other, one head of 20 with both,
    a task without rows; the gradient matrices have sentinel columns around the blocks and (dpad odd) an odd ``ldd``."""
    from egopack_amd import _lib
    g = gen(91)
    specs = [(77, (115, 478), (128, 512), 0.5, ("w", "a")), (33, (20,), (64,), 0.25, ("wa",)), (0, (5,), (8,), 1.0, ("wa",))]
    tasks = [_task(G, f"task{i}.", g, r, cs, pd, lpad, dpad, dt, sm, gs, wh) for i, (r, cs, pd, gs, wh) in enumerate(specs)]
    arr = (_lib.CEWTask * len(tasks))()
    for a, t in zip(arr, tasks):
        _fill(a, t)
    ok(lib.egk_ce_w_fused_multi(S(), arr, len(tasks), sm, edt(dt)), "egk_ce_w_fused_multi")
    G.check()
    out = {}
    for i, t in enumerate(tasks):
        _check(t, f"task{i}.")
        out[f"loss{i}"], out[f"dlogits{i}"] = t["loss"], t["D"]
    # refused on the host, nothing launched: a misaligned vector, pad < C
    arr[0].weight[0] = tasks[0]["vec"][0][0].ptr + 2
    refused(lib.egk_ce_w_fused_multi(S(), arr, len(tasks), sm, edt(dt)), "misaligned vector pointer")
    arr[0].weight[0] = tasks[0]["vec"][0][0].ptr
    arr[0].base.pad[1] = 477
    refused(lib.egk_ce_w_fused_multi(S(), arr, len(tasks), sm, edt(dt)), "pad must be >= C")
    G.check()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_class_balance(name, fn, variant, covers, plain):
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
