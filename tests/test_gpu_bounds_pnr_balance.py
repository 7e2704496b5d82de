"""Guard-band tests of include/egopack_bce_balanced.h: egk_bce_w_fwd, egk_bce_w_bwd and egk_rowdot_bce_w (finished by the unchanged
egk_rowdot_reduce) touch only what their arguments name.

The form of tests/test_gpu_bounds_class_balance.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is
registered there): every device argument sits in a sentinel-filled window (the NaN sentinel around an input reaches the result when
a read leaves the window; labels are surrounded by a valid label), outputs are compared with the float64 host model of
tests/pnr_balance_common.py, everything outside the windows must keep the sentinel bits, and a second run on plain buffers must give
the same bits.  n = 0, 1, 255, 257 (nothing, one thread, one workgroup less one thread, a second workgroup of one thread);
rows x cols = 77 x 1000 bf16, 333 x 256 f32, 2048 x 1024 bf16 -- the variants of the plain case: the general 4-register kernel with
a ragged tail, the 1-register kernel in f32, the exact-1024 specialisation on a full grid -- with and without ``df``; each with the
scalar triples (31, 1, 0), (0.25, 0.75, 2), (1, 1, 0.5).  The ledger of this header is in tests/test_pnr_balance_cpu.py; the module
imports without a GPU."""
import pytest
import torch

from tests import pnr_balance_common as PB
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import OUT16, Guards, P, S, _pad8, _ws_guard, bf16, close, edt, f32, i64, ok, r16, refused, same

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
    """Every entry point some case declares it covers (the ledger in tests/test_pnr_balance_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


@case("egk_bce_w_fwd", "egk_bce_w_bwd",
      variants=[dict(n=n, dt=dt, sh=sh) for n in (0, 1, 255, 257) for dt in (f32, bf16) for sh in PB.TRIPLES])
def bce_w(lib, ops, G, n, dt, sh):
    x, y, gl = PB.problem(n, 53 + n)
    X, Y, GL = G.v("logits", n, f32, init=x), G.v("y", n, i64, init=y, poison=1), G.v("gloss", n, f32, init=gl)
    loss, D = G.v("loss", n, f32), G.v("dlogits", n, dt)
    ok(lib.egk_bce_w_fwd(S(), P(X), P(Y), P(loss), n, *sh), "egk_bce_w_fwd")
    ok(lib.egk_bce_w_bwd(S(), P(X), P(Y), P(GL), P(D), n, *sh, edt(dt)), "egk_bce_w_bwd")
    G.check()
    ref, dref = PB.model(x, y, *sh, gl)
    close(loss.view, ref.float(), "loss", **PB.LOSS_TOL)
    close(D.view, dref.float(), "dlogits", **(OUT16 if dt == bf16 else PB.grad_tol(sh[0], sh[1])))
    if n:
        assert bool(torch.isfinite(loss.view).all()) and bool(torch.isfinite(D.view.float()).all())
        # refused on the host, nothing launched
        refused(lib.egk_bce_w_fwd(S(), P(X), P(Y), P(loss), n, -1.0, sh[1], sh[2]), "must be finite and >= 0")
        refused(lib.egk_bce_w_bwd(S(), P(X), P(Y), P(GL), P(D), n, sh[0], sh[1], float("nan"), edt(dt)), "must be finite and >= 0")
        refused(lib.egk_bce_w_bwd(S(), P(X), P(Y), P(GL), P(D), -n, *sh, edt(dt)), "n must be >= 0")
        G.check()
    return dict(loss=loss, dlogits=D)


@case("egk_rowdot_bce_w",
      variants=[dict(rows=r, cols=c, dt=dt, grad=grad, sh=sh) for r, c, dt in ((77, 1000, bf16), (333, 256, f32), (2048, 1024, bf16))
                for grad in (True, False) for sh in PB.TRIPLES])
def rowdot_bce_w(lib, ops, G, rows, cols, dt, grad, sh):
    """tests/test_gpu_bounds.py::rowdot_bce with the scalars: its operands, scales and tolerances; the reference is the host model
    on the float64 logits of the same (rounded) operands, the logit gradient for g = seed."""
    g = B.gen(rows + cols)
    f, w = r16(torch.randn(rows, cols, generator=g)), r16(torch.randn(cols, generator=g) * 0.05)
    bias, y = torch.randn(1, generator=g), PB.labels(rows, g)
    assert 0 < int(y.sum()) < rows
    seed = 0.7 / rows
    Fm, W, Bz = G.m("f", rows, cols, dt, init=f), G.v("w", cols, dt, init=w), G.v("bias", 1, f32, init=bias)
    Y = G.v("y", rows, i64, init=y, poison=1)
    LG, LS = G.v("logits", rows), G.v("loss", rows)
    z = f.double() @ w.double() + bias.double()
    ref, dz = PB.model(z, y, *sh, seed)
    f32m = dt == f32
    lt = dict(rtol=1e-4, atol=1e-4) if f32m else dict(rtol=1e-2, atol=2e-2)
    if not grad:
        ok(lib.egk_rowdot_bce_w(S(), P(Fm), P(W), P(Bz), P(Y), P(LG), P(LS), None, None, rows, cols, seed, *sh, edt(dt)), "egk_rowdot_bce_w")
        G.check()
        close(LG.view, z.float(), "logits", **lt), close(LS.view, ref.float(), "loss", **lt)
        return dict(logits=LG, loss=LS)
    DF = G.m("df", rows, cols, dt)
    WS = G.v("ws", lib.egk_rowdot_ws_rows(rows) * (cols + 4), f32, guard=_ws_guard(cols))   # exactly egk_rowdot_ws_rows(rows) * (cols + 4)
    slot0 = torch.randn(_pad8(cols) + 8, generator=g)
    FL = G.v("flat_g (dw slot | db slot)", _pad8(cols) + 8, f32, init=slot0)
    ok(lib.egk_rowdot_bce_w(S(), P(Fm), P(W), P(Bz), P(Y), P(LG), P(LS), P(DF), P(WS), rows, cols, seed, *sh, edt(dt)), "egk_rowdot_bce_w")
    ok(lib.egk_rowdot_reduce(S(), P(WS), P(FL), P(FL, _pad8(cols) * 4), rows, cols), "egk_rowdot_reduce")
    G.check()
    close(LG.view, z.float(), "logits", **lt), close(LS.view, ref.float(), "loss", **lt)
    dfr, dwr, dbr = dz[:, None] * w.double()[None, :], dz @ f.double(), dz.sum()
    gs, wsc = float(dfr.abs().max()), float(dwr.abs().max())
    c8, got = _pad8(cols), FL.view.cpu().double()
    assert (DF.view.float().cpu().double() - dfr).abs().max() <= (1e-5 if f32m else 1.5e-2) * gs, "df"
    assert (got[:cols] - slot0[:cols].double() - dwr).abs().max() <= (2e-5 if f32m else 1.5e-2) * wsc + 1e-6, "dw"
    assert abs(float(got[c8] - slot0[c8].double() - dbr)) <= (2e-5 if f32m else 1e-2) * max(1.0, abs(float(dbr)) * 100), "db"
    same(FL.view[cols:c8], slot0[cols:c8], "padding behind the dw slot"), same(FL.view[c8 + 1:], slot0[c8 + 1:], "behind the db word")
    # refused on the host, nothing launched: a bad scalar, df without its workspace, an unaligned f
    refused(lib.egk_rowdot_bce_w(S(), P(Fm), P(W), P(Bz), P(Y), P(LG), P(LS), P(DF), P(WS), rows, cols, seed, sh[0], -sh[1], sh[2], edt(dt)),
            "must be finite and >= 0")
    refused(lib.egk_rowdot_bce_w(S(), P(Fm), P(W), P(Bz), P(Y), P(LG), P(LS), P(DF), None, rows, cols, seed, *sh, edt(dt)),
            "gradients need the partial-row workspace")
    refused(lib.egk_rowdot_bce_w(S(), P(Fm, 2), P(W), P(Bz), P(Y), P(LG), P(LS), P(DF), P(WS), rows, cols, seed, *sh, edt(dt)),
            "unaligned pointer")
    G.check()
    return dict(logits=LG, loss=LS, df=DF, flat=FL)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_pnr_balance(name, fn, variant, covers, plain):
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
