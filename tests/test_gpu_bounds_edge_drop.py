"""Guard-band tests of include/egopack_edge_drop.h: each of the two launches touches only what its arguments name.

The form of tests/test_gpu_bounds_mixup.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is registered
there): every device argument sits in a sentinel-filled window.  ``x`` / ``dout`` carry one POISON ROW (NaN) behind their rows and
the sentinel of ``col`` / ``t_col`` names it, ``rowptr``'s sentinel is the edge count, ``inv_deg`` and the gate sit between NaN
guards, the device word between zeros.  Outputs are held to the float64 models of tests/edge_drop_common.py on the kept edges of
the host model, ``keep_out`` to the host model exactly; everything outside the windows keeps its bits, the inputs too, and a second
run on plain buffers gives the same bits.  Every refusal of the header returns its own message and writes nothing.  The ledger of
this header is tests/test_cabi_addons.py; the module imports without a GPU."""
import pytest
import torch

from tests import edge_drop_common as EC
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, P, S, bf16, f32, i32, i64, ok, refused, same, u8

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
SEED, OFF, WORD = 0xC0FFEE_1234_5678, 640, (1 << 41) + 7


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


@case("egk_csr_mean_drop_fwd", "egk_csr_mean_drop_bwd",
      variants=[dict(kind="band", cols=1024, dt=bf16, p=0.3, fl=3), dict(kind="lta", cols=40, dt=f32, p=0.3, fl=3),
                dict(kind="wrap", cols=43, dt=bf16, p=0.5, fl=0), dict(kind="wrap", cols=260, dt=f32, p=0.3, fl=1),
                dict(kind="single", cols=1, dt=f32, p=1.0, fl=2), dict(kind="lta", cols=2048, dt=f32, p=0.0, fl=3)])
def mean_drop(lib, ops, G, kind, cols, dt, p, fl):
    from egopack_amd import data as D
    ei, n = EC.GRAPHS[kind]()
    gr = D.build_csr(ei, n)
    E = ei.shape[1]
    sym, ks = bool(fl & 1), bool(fl & 2)
    g = B.gen(n * 31 + cols)
    x, dout, gate = (B.r16(torch.randn(n, cols, generator=g)) for _ in range(3))
    nan_row = torch.full((1, cols), float("nan"))
    X = G.m("x (+ poison row)", n + 1, cols, dt, init=torch.cat([x, nan_row]))
    DO = G.m("dout (+ poison row)", n + 1, cols, dt, init=torch.cat([dout, nan_row]))
    GT = G.m("gate", n, cols, dt, init=gate)
    RP, CL = G.v("rowptr", n + 1, i32, init=gr.rowptr, poison=E), G.v("col", E, i32, init=gr.col, poison=n)
    TRP, TCL = G.v("t_rowptr", n + 1, i32, init=gr.t_rowptr, poison=E), G.v("t_col", E, i32, init=gr.t_col, poison=n)
    W = G.v("word", 1, i64, init=torch.tensor([WORD]), poison=0)
    O, DX = G.m("out", n, cols, dt), G.m("dx", n, cols, dt)
    INV = G.v("inv_deg", n, f32)
    KF, KB = G.v("keep_out fwd", E, u8), G.v("keep_out bwd", E, u8)
    fwd = lambda **kw: lib.egk_csr_mean_drop_fwd(  # noqa: E731
        S(), kw.get("x", P(X)), kw.get("rowptr", P(RP)), kw.get("col", P(CL)), kw.get("out", P(O)), kw.get("inv", P(INV)), P(KF),
        kw.get("rows", n), kw.get("cols", cols), kw.get("dtype", B.edt(dt)), kw.get("p", p), kw.get("flags", fl), SEED, OFF,
        kw.get("word", P(W)))
    bwd = lambda **kw: lib.egk_csr_mean_drop_bwd(  # noqa: E731
        S(), kw.get("x", P(DO)), kw.get("rowptr", P(TRP)), kw.get("col", P(TCL)), kw.get("inv", P(INV)), kw.get("gate", P(GT)),
        kw.get("out", P(DX)), P(KB), kw.get("rows", n), kw.get("cols", cols), kw.get("dtype", B.edt(dt)), kw.get("p", p),
        kw.get("flags", fl), SEED, OFF, kw.get("word", P(W)))
    ok(fwd(), "egk_csr_mean_drop_fwd")
    ok(bwd(), "egk_csr_mean_drop_bwd")
    G.check()
    kf, kb = EC.keep_fwd(gr, SEED, OFF, p, sym, ks, WORD), EC.keep_bwd(gr, SEED, OFF, p, sym, ks, WORD)
    same(KF.view, torch.from_numpy(kf), "keep_out (forward order) against the host model")
    same(KB.view, torch.from_numpy(kb), "keep_out (transposed order) against the host model")
    want, cnt = EC.fwd_model(x, gr, kf)
    same(INV.view.view(torch.int32), EC.inv_deg_bits(cnt.numpy()).view(torch.int32), "inv_deg = 1 / kept count, bit for bit")
    tol = dict(rtol=1e-5, atol=1e-5) if dt == f32 else dict(rtol=1e-2, atol=1e-2)  # the plain gather's (tests/test_gpu_kernels.py)
    B.close(O.view.double(), want, "out against the float64 model", **tol)
    B.close(DX.view.double(), EC.bwd_model(dout, gr, kb, cnt, gate=gate), "dx against the float64 model", **tol)
    same(X.view[:n].float(), x, "x is read, never written")
    same(DO.view[:n].float(), dout, "dout is read, never written")
    same(GT.view.float(), gate, "gate is read, never written")
    for t, ref, what in ((RP, gr.rowptr, "rowptr"), (CL, gr.col, "col"), (TRP, gr.t_rowptr, "t_rowptr"), (TCL, gr.t_col, "t_col")):
        same(t.view, ref, f"{what} is read, never written")
    same(W.view, torch.tensor([WORD]), "the device word is read, never written")
    # every refusal has its own message and writes nothing
    before = [t.bits() for t in (O, DX, INV, KF, KB)]
    for name, call in (("egk_csr_mean_drop_fwd", fwd), ("egk_csr_mean_drop_bwd", bwd)):
        refused(call(p=1.5), f"{name}: p must lie in [0, 1]")
        refused(call(p=-0.1), f"{name}: p must lie in [0, 1]")
        refused(call(p=float("nan")), f"{name}: p must lie in [0, 1]")
        refused(call(cols=0), f"{name}: cols must be >= 1")
        refused(call(cols=4097), f"{name}: rows wider than 4096")
        refused(call(rows=-1), f"{name}: rows must be >= 0")
        refused(call(x=None), f"{name}: null input matrix")
        refused(call(out=None), f"{name}: null output matrix")
        refused(call(inv=None), f"{name}: null inv_deg")
        refused(call(rowptr=None), f"{name}: null rowptr")
        refused(call(col=None), f"{name}: null col")
        refused(call(dtype=5), f"{name}: unknown element dtype")
        refused(call(flags=4), f"{name}: unknown flag bits")
        refused(call(word=P(W, 4)), f"{name}: inv_deg, rowptr and col must be 4-byte aligned, the device word 8-byte")
        refused(call(x=P(X if name.endswith("fwd") else DO, 1)), f"{name}: unaligned pointer")
        ok(call(rows=0), name + " with rows == 0")
    G.check()
    for t, b in zip((O, DX, INV, KF, KB), before):
        assert torch.equal(b, t.bits()), "a refused (or empty) call wrote an output"
    return dict(out=O, dx=DX, inv_deg=INV, keep_fwd=KF, keep_bwd=KB)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_edge_drop(name, fn, variant, covers, plain):
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
