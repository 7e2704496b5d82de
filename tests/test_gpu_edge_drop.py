"""The two launches of include/egopack_edge_drop.h and ``ops.csr_mean_aggregate(drop=)`` / ``ops.sage_mean_layer(drop=)`` against the
host model of tests/edge_drop_common.py.

Keep bits (forward and transposed order) and ``inv_deg``: exact.  Outputs and gradients: the float64 model on the thinned graph at
the tolerances tests/test_gpu_kernels.py uses for the plain gather (f32 1e-5, bf16 1e-2), rows without a kept edge exactly 0.
Bitwise, from the header's order rule: every row whose degree in the ORIGINAL graph is at most 12 (``HEAVY`` of graph_ops.hip, up to
which the existing gather sums a row in edge order in one wave) has the bits of the existing ``ops._csr_gather`` on the thinned graph
-- forward unweighted, backward with that graph's ``t_wgt``, with and without a gate; with p = 0 that is the plain launch on the
same graph.  Two runs give the same bits; the bf16 output is the f32 twin's rounded once."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import edge_drop_common as EC

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32T = torch.bfloat16, torch.float32
HEAVY = 12  # graph_ops.hip
TOL = {F32T: dict(rtol=1e-5, atol=1e-5), BF: dict(rtol=1e-2, atol=1e-2)}  # test_csr_mean_aggregate_fwd_bwd
SEED, OFF = 0x1234_5678_9ABC_DEF1, 4096
WORD = (1 << 40) + 12345


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ops(lib):
    from egopack_amd import ops
    return ops


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ok(rc):
    from egopack_amd import _lib
    assert rc == 0, _lib.last_error()


def edt(dt):
    return 1 if dt == BF else 0  # EGK_BF16 / EGK_F32


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32T else torch.int16).cpu()


def r16(t):
    return t.to(BF).float()


_graphs = {}


def graph_of(name):
    """(edge_index, CSRGraph on the host, CSRGraph on the device), built once."""
    if name not in _graphs:
        from egopack_amd import data
        ei, n = EC.GRAPHS[name]()
        g = data.build_csr(ei, n)
        _graphs[name] = (ei, g, g.to(DEV))
    return _graphs[name]


_inputs = {}


def inputs(name, cols):
    """x, dout, gate on the host (bf16-representable f32: both element types see the same values), built once per shape."""
    key = (name, cols)
    if key not in _inputs:
        n = graph_of(name)[1].num_nodes
        g = torch.Generator().manual_seed(977 * cols + n)
        _inputs[key] = tuple(r16(torch.randn(n, cols, generator=g)) for _ in range(3))
    return _inputs[key]


def launch(lib, name, cols, dt, p, sym, ks, word=None, gate=True):
    """Both launches through the C ABI with keep_out -> dict of device results."""
    _, g, gd = graph_of(name)
    x, dout, gt = (t.to(DEV).to(dt) for t in inputs(name, cols))
    n, E = g.num_nodes, g.col.numel()
    out, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    inv = torch.full((n,), 7.0, device=DEV)
    kf, kb = torch.full((E,), 9, dtype=torch.uint8, device=DEV), torch.full((E,), 9, dtype=torch.uint8, device=DEV)
    w = torch.tensor([word], dtype=torch.int64, device=DEV) if word is not None else None
    fl = EC.flags_of(sym, ks)
    ok(lib.egk_csr_mean_drop_fwd(S(), P(x), P(gd.rowptr), P(gd.col), P(out), P(inv), P(kf), n, cols, edt(dt), p, fl, SEED, OFF, P(w)))
    ok(lib.egk_csr_mean_drop_bwd(S(), P(dout), P(gd.t_rowptr), P(gd.t_col), P(inv), P(gt) if gate else None, P(dx), P(kb), n, cols,
                                 edt(dt), p, fl, SEED, OFF, P(w)))
    torch.cuda.synchronize()
    return dict(out=out, dx=dx, inv=inv, kf=kf, kb=kb)


FLAGS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("sym,ks", FLAGS, ids=lambda v: str(int(v)))
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("name", list(EC.GRAPHS))
def test_keep_bits_and_inv_deg_are_the_host_models(lib, name, p, sym, ks):
    """cols = 1 (the element path), f32; the device word nonzero, above 2^40, on the flagship flags."""
    word = WORD if (sym and ks) else None
    _, g, _ = graph_of(name)
    r = launch(lib, name, 1, F32T, p, sym, ks, word=word)
    kf = EC.keep_fwd(g, SEED, OFF, p, sym, ks, word or 0)
    kb = EC.keep_bwd(g, SEED, OFF, p, sym, ks, word or 0)
    assert torch.equal(r["kf"].cpu(), torch.from_numpy(kf)), "forward-order keep bits"
    assert torch.equal(r["kb"].cpu(), torch.from_numpy(kb)), "transposed-order keep bits"
    cnt = np.bincount(EC.rows_of(g.rowptr.numpy())[kf.astype(bool)], minlength=g.num_nodes)
    assert torch.equal(bits(r["inv"]), bits(EC.inv_deg_bits(cnt))), "inv_deg is not 1 / count, correctly rounded"
    if p == 0.0:
        assert kf.all() and kb.all()
    if p == 1.0:
        src, dst = g.col.numpy(), EC.rows_of(g.rowptr.numpy())
        assert np.array_equal(kf.astype(bool), (src == dst) & ks)


@pytest.mark.parametrize("dt", [F32T, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("cols", [1, 40, 43, 1024])
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("name", list(EC.GRAPHS))
def test_launches_against_float64_and_bitwise_against_the_gather_on_the_thinned_graph(lib, ops, name, p, cols, dt):
    from egopack_amd import data
    sym, ks = (True, True) if cols != 43 else (False, False)
    word = WORD if cols == 40 else None
    ei, g, gd = graph_of(name)
    x, dout, gt = inputs(name, cols)
    r = launch(lib, name, cols, dt, p, sym, ks, word=word)
    kf, kb = r["kf"].cpu().numpy(), r["kb"].cpu().numpy()
    assert np.array_equal(kf, EC.keep_fwd(g, SEED, OFF, p, sym, ks, word or 0))
    # float64 on the thinned graph
    want, cnt = EC.fwd_model(x, g, kf)
    torch.testing.assert_close(r["out"].double().cpu(), want, **TOL[dt])
    empty = (cnt == 0).to(DEV)
    assert not r["out"][empty].float().ne(0).any() and not torch.signbit(r["out"][empty].float()).any(), "a row without a kept edge is +0"
    want_dx = EC.bwd_model(dout, g, kb, cnt, gate=gt)
    torch.testing.assert_close(r["dx"].double().cpu(), want_dx, **TOL[dt])
    # reproducibility
    r2 = launch(lib, name, cols, dt, p, sym, ks, word=word)
    for k in ("out", "dx", "inv", "kf", "kb"):
        assert torch.equal(r[k], r2[k]), f"{k}: two runs differ"
    # bitwise: the existing gather on the thinned graph, rows of at most HEAVY edges in the original graph
    tg = data.build_csr(EC.thin(ei, SEED, OFF, p, sym, ks, word or 0), g.num_nodes).to(DEV)
    xd, dd, gd_ = (t.to(DEV).to(dt) for t in (x, dout, gt))
    light_in = ((g.rowptr[1:] - g.rowptr[:-1]) <= HEAVY).to(DEV)
    light_out = ((g.t_rowptr[1:] - g.t_rowptr[:-1]) <= HEAVY).to(DEV)
    ref = torch.empty_like(xd)
    ops._csr_gather(xd, tg.rowptr, tg.col, None, None, ref, tg.heavy, tg.heavy_mode)
    assert torch.equal(bits(r["out"][light_in]), bits(ref[light_in])), "forward: not the bits of the gather on the thinned graph"
    ops._csr_gather(dd, tg.t_rowptr, tg.t_col, tg.t_wgt, gd_, ref, tg.t_heavy, tg.t_heavy_mode)
    assert torch.equal(bits(r["dx"][light_out]), bits(ref[light_out])), "gated backward: not the bits of the gather on the thinned graph"
    ungated = launch(lib, name, cols, dt, p, sym, ks, word=word, gate=False)
    ops._csr_gather(dd, tg.t_rowptr, tg.t_col, tg.t_wgt, None, ref, tg.t_heavy, tg.t_heavy_mode)
    assert torch.equal(bits(ungated["dx"][light_out]), bits(ref[light_out])), "backward: not the bits of the gather on the thinned graph"
    torch.testing.assert_close(ungated["dx"].double().cpu(), EC.bwd_model(dout, g, kb, cnt), **TOL[dt])
    torch.cuda.synchronize()


@pytest.mark.parametrize("cols", [1, 40, 43, 1024])
@pytest.mark.parametrize("name", ["band", "wrap"])
def test_bf16_is_the_f32_twin_rounded_once(lib, name, cols):
    f = launch(lib, name, cols, F32T, 0.3, True, True)
    h = launch(lib, name, cols, BF, 0.3, True, True)
    assert torch.equal(f["kf"], h["kf"]) and torch.equal(bits(f["inv"]), bits(h["inv"]))
    for k in ("out", "dx"):  # (the inputs are bf16-representable: both runs perform the same f32 operations)
        assert torch.equal(bits(f[k].to(BF)), bits(h[k])), f"{k}: bf16 is not the f32 result rounded once"


# ---- the ops ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32T, BF], ids=["f32", "bf16"])
def test_csr_mean_aggregate_drop(ops, dt):
    ei, g, gd = graph_of("lta")
    x, dout, _ = inputs("lta", 40)
    ops.manual_seed(77)
    xd = x.to(DEV).to(dt).requires_grad_(True)
    drop = ops.EdgeDrop(0.3)
    tap = ops.tap_dropout_masks()
    with tap, ops.tap_edge_keep() as keep:
        out = ops.csr_mean_aggregate(xd, gd, drop=drop)
        out.backward(dout.to(DEV).to(dt))
    torch.cuda.synchronize()
    (kind, seed, off, rows, E), = tap.launches
    assert (kind, rows, E) == ("edge", g.num_nodes, g.col.numel())
    word = int(ops.rng_device_offset(xd.device).item())
    assert torch.equal(keep.fwd[0].cpu(), torch.from_numpy(EC.keep_fwd(g, seed, off, 0.3, True, True, word))), "the tap's record"
    assert torch.equal(keep.bwd[0].cpu(), torch.from_numpy(EC.keep_bwd(g, seed, off, 0.3, True, True, word)))
    assert ops.rng_snapshot() == off + EC.reserved(g.num_nodes), "a launch reserves rows + 64 counters"
    x64 = x.double().requires_grad_(True)
    want = EC.mean_ref(x64, EC.thin(ei, seed, off, 0.3, True, True, word), g.num_nodes)
    want.backward(dout.double())
    torch.testing.assert_close(out.detach().double().cpu(), want.detach(), **TOL[dt])
    torch.testing.assert_close(xd.grad.double().cpu(), x64.grad, **TOL[dt])
    # drop=None, p = 0 and a pass without gradients: the bits (and the launches) of today's call
    plain = ops.csr_mean_aggregate(xd.detach(), gd)
    snap = ops.rng_snapshot()
    for d in (None, ops.EdgeDrop(0.0)):
        assert torch.equal(bits(ops.csr_mean_aggregate(xd.detach().requires_grad_(True), gd, drop=d).detach()), bits(plain))
    with torch.no_grad():
        assert torch.equal(bits(ops.csr_mean_aggregate(xd, gd, drop=drop)), bits(plain))
    assert ops.rng_snapshot() == snap, "an inactive drop drew counters"
    # a pre-drawn (seed, offset): two launches, one mask
    shared = drop.with_rng(ops.edge_drop_rng(g.num_nodes))
    with ops.tap_edge_keep() as keep2:
        a = ops.csr_mean_aggregate(xd, gd, drop=shared)
        b = ops.csr_mean_aggregate(xd, gd, drop=shared)
    assert torch.equal(keep2.fwd[0], keep2.fwd[1]) and torch.equal(bits(a.detach()), bits(b.detach()))
    with pytest.raises(ValueError, match="p must lie in"):
        ops.EdgeDrop(1.5)
    torch.cuda.synchronize()


GEMM_F32 = dict(out=(1e-4, 1e-3), grad=(1e-4, 2e-3))  # tests/test_gpu_layouts.py, sage_mean_layer in f32
BLOCK_REL = 5e-3                                      # ... and in bf16: relative Frobenius distance per tensor


@pytest.mark.parametrize("dt", [F32T, BF], ids=["f32", "bf16"])
def test_sage_mean_layer_drop(ops, dt):
    from oracle import storage as ST
    ei, g, gd = graph_of("lta")
    n, K, N = g.num_nodes, 48, 40
    gen = torch.Generator().manual_seed(40)
    rnd = lambda *s, scale=1.0: r16(torch.randn(*s, generator=gen) * scale)  # noqa: E731
    par = dict(Wp=rnd(K, K, scale=0.3), bp=torch.randn(K, generator=gen), Wl=rnd(N, K, scale=0.3), bl=torch.randn(N, generator=gen),
               Wr=rnd(N, K, scale=0.3))
    h, dy = rnd(n, K), rnd(n, N)
    NS = types.SimpleNamespace
    dev = {k: v.to(DEV).requires_grad_(True) for k, v in par.items()}
    conv = NS(lin=NS(weight=dev["Wp"], bias=dev["bp"]), lin_l=NS(weight=dev["Wl"], bias=dev["bl"]), lin_r=NS(weight=dev["Wr"]))
    hd = h.to(DEV).to(dt).requires_grad_(True)
    ops.manual_seed(5)
    drop = ops.EdgeDrop(0.3, symmetric=False, keep_self=False)
    tap = ops.tap_dropout_masks()
    mode = "f32" if dt == F32T else "bf16"  # (as tests/test_gpu_layouts.py runs the layer)
    with tap, ops.compute_mode(mode):
        out = ops.sage_mean_layer(hd, conv, gd, drop=drop)
        out.backward(dy.to(DEV).to(dt))
    torch.cuda.synchronize()
    (kind, seed, off, rows, E), = tap.launches
    assert kind == "edge"
    word = int(ops.rng_device_offset(hd.device).item())
    tei = EC.thin(ei, seed, off, 0.3, False, False, word)
    p64 = {k: v.double().requires_grad_(True) for k, v in par.items()}
    h64 = h.double().requires_grad_(True)
    with ST.bf16_storage(dt == BF):
        xp = ST.act(torch.relu(F.linear(h64, p64["Wp"], p64["bp"])))
        agg = ST.act(EC.mean_ref(xp, tei, n))
        want = ST.act(F.linear(agg, p64["Wl"], p64["bl"]) + F.linear(h64, p64["Wr"]))
        want.backward(dy.double())

    def close(got, ref, tol, what):
        got, ref = got.detach().double().cpu(), ref.detach()
        if dt == BF:
            rel = float((got - ref).norm() / ref.norm().clamp(min=1e-30))
            assert rel < BLOCK_REL, f"{what}: relative distance {rel:.3e}"
        else:
            torch.testing.assert_close(got, ref, rtol=tol[0], atol=tol[1], msg=lambda s: f"{what}: {s}")
    close(out, want, GEMM_F32["out"], "out")
    close(hd.grad, h64.grad, GEMM_F32["grad"], "d_h")
    for k in par:
        close(dev[k].grad, p64[k].grad, GEMM_F32["grad"], f"d_{k}")
    # drop=None and p = 0: the bits of today's call
    with ops.compute_mode(mode):
        plain = ops.sage_mean_layer(hd.detach(), conv, gd)
        for d in (None, ops.EdgeDrop(0.0)):
            got = ops.sage_mean_layer(hd.detach().requires_grad_(True), conv, gd, drop=d)
            assert torch.equal(bits(got.detach()), bits(plain.detach()))
    torch.cuda.synchronize()
