"""Guard-band tests of the tail of egk_ce_task (include/egopack_hip.h): the launches that take the struct touch only
what it names -- the ``margin`` vectors and the ``gloss`` row seeds included, and no gradient matrix under ``loss_only``.

The form of tests/test_gpu_bounds_class_balance.py, whose task builder is reused (helpers and ``Guards`` of
tests/test_gpu_bounds.py; nothing is registered there, and the entry points are in the ledger already): every device argument
sits in a sentinel-filled window (the NaN sentinel around an input reaches the result when a read leaves the window), outputs are
compared with the float64 reference of tests/ce_shape_common.py, everything outside the windows must keep the sentinel bits, and a
second run on plain buffers must give the same bits.  The module imports without a GPU."""
import pytest
import torch

from tests import ce_shape_common as SH
from tests import test_gpu_bounds as B
from tests import test_gpu_bounds_class_balance as CEB
from tests.test_gpu_bounds import OUT16, Guards, S, bf16, close, edt, f32, f64, gen, ok, refused

CASES = []  # (id, function, variant dict, second run on plain buffers?)


def case(variants):
    def deco(fn):
        for v in variants:
            CASES.append((fn.__name__ + "-" + "-".join(f"{k}={B._fmt(x)}" for k, x in v.items()), fn, dict(v), True))
        return fn
    return deco


def _shape(G, t, tag, margins, gamma, gloss):
    """Add the tail's windows to a task of ``CEB._task``: a margin vector for the heads ``margins`` names, the row seeds."""
    t["m"] = [SH.ldam(c) if on else None for c, on in zip(t["Cs"], margins)]
    t["M"] = [None if m is None else G.v(f"{tag}margin{h}", m.numel(), f32, init=m) for h, m in enumerate(t["m"])]
    t["gamma"] = gamma
    t["gl"] = 2 * torch.rand(t["rows"], generator=gen(5 + t["rows"])) - 1 if gloss else None
    t["GL"] = G.v(tag + "gloss", t["rows"], f32, init=t["gl"]) if gloss else None
    return t


def _tail(b, t, loss_only=0):
    for h in range(t["n"]):
        b.margin[h] = None if t["M"][h] is None else t["M"][h].ptr
    b.gloss, b.focal_gamma, b.loss_only = (None if t["GL"] is None else t["GL"].ptr), t["gamma"], loss_only


def _check(t, tag, grad=True):
    rows, n = t["rows"], t["n"]
    ltol, gtol = SH.tols(t["gamma"])
    total = torch.zeros(rows, dtype=f64)
    inside = torch.zeros(t["D"].cols, dtype=torch.bool)
    seed = torch.full((rows,), t["gscale"]) * (1 if t["gl"] is None else t["gl"])
    for h in range(n):
        _, _, w, a = t["vec"][h]
        ref, dref, _ = SH.reference(t["logits"][h], t["y"][:, h], w, a, t["m"][h], t["sm"], t["gamma"], seed)
        total += ref
        if not grad:
            continue
        c0, Cn, pd = t["dcol"][h], t["Cs"][h], t["pads"][h]
        inside[c0:c0 + pd] = True
        close(t["D"].view[:, c0:c0 + Cn], dref.float(), f"{tag}dlogits head {h}", **(OUT16 if t["dt"] == bf16 else gtol))
        assert not t["D"].view[:, c0 + Cn:c0 + pd].float().ne(0).any(), f"{tag}dlogits head {h}: pad columns [C, pad) are not zero"
        dead = (t["y"][:, h] < 0)
        assert not t["D"].view[dead][:, c0:c0 + pd].float().ne(0).any(), f"{tag}dlogits head {h}: ignored rows have a gradient"
    close(t["loss"].view, total.float(), tag + "loss", **ltol)
    keep = t["D"].is_sentinel()[:, ~inside]
    assert bool(keep.all()), f"{tag}dlogits: {int((~keep).sum())} element(s) outside every head's column block were written"


@case([dict(dt=bf16, lpad=0, dpad=0, sm=0.1), dict(dt=f32, lpad=3, dpad=5, sm=0.1), dict(dt=f32, lpad=0, dpad=1, sm=0.0)])
def ce_shape_fused_multi(lib, ops, G, dt, lpad, dpad, sm):
    """egk_ce_w_fused_multi, three tasks: (115, 478) in pads (128, 512) with both margins, gamma 0.5, weights / offsets; one head of
    20 with a margin, gamma 2, both vectors and row seeds; a task without rows."""
    from egopack_amd import _lib
    g = gen(93)
    specs = [(77, (115, 478), (128, 512), 0.5, ("w", "a"), (True, True), 0.5, False), (33, (20,), (64,), 0.25, ("wa",), (True,), 2.0, True),
             (0, (5,), (8,), 1.0, ("wa",), (True,), 0.5, True)]
    tasks = [_shape(G, CEB._task(G, f"task{i}.", g, r, cs, pd, lpad, dpad, dt, sm, gs, wh), f"task{i}.", ms, gm, gl)
             for i, (r, cs, pd, gs, wh, ms, gm, gl) in enumerate(specs)]
    arr = (_lib.CEWTask * len(tasks))()
    for a, t in zip(arr, tasks):
        CEB._fill(a, t)
        _tail(a.base, t)
    ok(lib.egk_ce_w_fused_multi(S(), arr, len(tasks), sm, edt(dt)), "egk_ce_w_fused_multi")
    G.check()
    out = {}
    for i, t in enumerate(tasks):
        _check(t, f"task{i}.")
        out[f"loss{i}"], out[f"dlogits{i}"] = t["loss"], t["D"]
    # refused on the host, nothing launched: a misaligned margin, misaligned row seeds
    arr[0].base.margin[1] = tasks[0]["M"][1].ptr + 2
    refused(lib.egk_ce_w_fused_multi(S(), arr, len(tasks), sm, edt(dt)), "misaligned margin pointer")
    arr[0].base.margin[1] = tasks[0]["M"][1].ptr
    arr[1].base.gloss = tasks[1]["GL"].ptr + 1
    refused(lib.egk_ce_w_fused_multi(S(), arr, len(tasks), sm, edt(dt)), "not 4-byte aligned")
    G.check()
    return out


@case([dict(null_d=True, sm=0.1, gamma=0.5), dict(null_d=False, sm=0.0, gamma=2.0), dict(null_d=False, sm=0.1, gamma=0.0)])
def ce_shape_loss_only(lib, ops, G, null_d, sm, gamma):
    """egk_ce_fused_multi (no vectors) as a forward-only pass: the loss vectors are written, a gradient matrix that is passed
    anyway keeps every sentinel, a NULL one is accepted."""
    from egopack_amd import _lib
    g = gen(97)
    specs = [(77, (115, 478), (128, 512), 0.5, (True, False)), (33, (65,), (65,), 1.0, (True,))]
    tasks = []
    for i, (r, cs, pd, gs, ms) in enumerate(specs):
        t = B._ce_fused_task(G, f"task{i}.", g, r, cs, pd, 3, 1, f32, sm, gs)
        t["vec"] = [(None, None, None, None)] * len(cs)
        tasks.append(_shape(G, t, f"task{i}.", ms, gamma, False))
    arr = (_lib.CETask * len(tasks))()
    for b, t in zip(arr, tasks):
        for h in range(t["n"]):
            b.logits[h], b.ld[h], b.C[h], b.pad[h], b.dcol[h] = t["L"][h].ptr, t["L"][h].ld, t["Cs"][h], t["pads"][h], t["dcol"][h]
        b.n_heads, b.y, b.y_stride, b.loss, b.ldd, b.rows, b.gscale = t["n"], t["Y"].ptr, t["n"] + 1, t["loss"].ptr, t["D"].ld, t["rows"], t["gscale"]
        b.dlogits = None if null_d else t["D"].ptr
        _tail(b, t, loss_only=1)
    ok(lib.egk_ce_fused_multi(S(), arr, len(tasks), sm, edt(f32)), "egk_ce_fused_multi")
    G.check()
    out = {}
    for i, t in enumerate(tasks):
        _check(t, f"task{i}.", grad=False)   # (no column block is "inside": the whole gradient matrix must keep its sentinel)
        out[f"loss{i}"] = t["loss"]
    arr[0].loss_only = 0
    if null_d:
        refused(lib.egk_ce_fused_multi(S(), arr, len(tasks), sm, edt(f32)), "null pointer")
    G.check()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_ce_shape(name, fn, variant, plain):
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
