"""bf16 row kernels against their rounded f32 twins (bf16 in HBM, f32 in registers, ONE rounding at the store).

Every case runs one op twice on the same bf16-representable inputs -- once with f32 tensors, once with bf16 tensors; parameters,
banks and frequencies stay f32 in both -- and hands every output and gradient to ``round_once_common``:
  * bf16-stored tensors: ``check_round_once`` (each element one of the two bf16 neighbours of the f32 twin, at most 1 % not the
    nearest; ``cap=0`` where the op does no arithmetic),
  * f32 side outputs: ``check_same_f32`` at the tolerance of the op's f32 test in test_gpu_kernels.py; integer outputs bit-equal,
  * the f32 run against an fp64 model at that same tolerance, so the pair cannot be wrong together.
tests/test_round_once_cpu.py checks the helper and, for the same inputs, that the reference alone stays a factor ten inside the cap.
With EGK_ROUND_ONCE_OUT=<file> the measured shares are written there, one line per tensor (profiles/round_once.txt).
"""
import ctypes as C
import itertools
import os

import pytest
import torch

from tests import round_once_common as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32T = torch.bfloat16, torch.float32
DTS = (F32T, BF)
_REC = []


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops as _ops
    yield _ops
    out = os.environ.get("EGK_ROUND_ONCE_OUT")
    if out and _REC:
        with open(out, "w") as fh:
            fh.write("# op shape tensor share-of-roundings-that-differ-from-the-rounded-f32-twin (cap 1 %; 'exact' cases must be 0)\n")
            fh.writelines(f"{op} {shape} {tensor} {share:.5%}\n" for op, shape, tensor, share in _REC)


@pytest.fixture(scope="module")
def lib(ops):
    from egopack_amd import _lib
    return _lib.load()


def ok(rc):
    from egopack_amd import _lib
    assert rc == 0, _lib.last_error()


def act(t, dt):
    return t.to(DEV).to(dt).contiguous()


def once(op, shape, pairs, cap=RO.CAP):
    """``pairs``: name -> (bf16 run, f32 run).  The helper on each, the share recorded."""
    for name, (g, r) in pairs.items():
        share = RO.check_round_once(g, r, f"{op} {shape} {name}", cap)
        print(f"round-once {op} {shape} {name}: {share:.5%}")
        _REC.append((op, str(shape).replace(" ", ""), name, share))


# ---------------------------------------------------------------------------------------------------------------------------
# row LayerNorm (+ReLU, +dropout), single and grouped launch
# ---------------------------------------------------------------------------------------------------------------------------
def _rowln(ops, lib, inp, dt, relu):
    x, dy, w, b = act(inp["x"], dt), act(inp["dy"], dt), inp["w"].to(DEV), inp["b"].to(DEV)
    rows, cols = x.shape
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    P, s = ops._p, ops._stream()
    ok(lib.egk_rowln_fwd(s, P(x), P(w), P(b), P(y), P(mean), P(rstd), None, rows, cols, RO.EPS, int(relu), 0.0, 0, 0, None, ops._dt(x)))
    dw, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
    ws = torch.empty(2 * lib.egk_rowln_bwd_ws_rows(rows) * cols, device=DEV)
    ok(lib.egk_rowln_bwd(s, P(dy), P(x), P(w), P(b), P(mean), P(rstd), None, P(dx), P(dw), P(db), P(ws), rows, cols, int(relu), 0.0,
                         ops._dt(x)))
    torch.cuda.synchronize()
    return dict(y=y, dx=dx, mean=mean, rstd=rstd, dw=dw, db=db)


def _ln_checks(op, shape, f, h, ref, fam, side, rows=0):
    """f / h: outputs of the f32 / bf16 run, ref: the fp64 model; y and dx are storage tensors, ``side`` the f32 outputs."""
    for k in ("y", "dx"):
        RO.close_to_model(f[k], ref[k], f"{fam}.{k}")
    for k in side:
        RO.close_to_model(f[k], ref[k], f"{fam}.{k}", rows)
        RO.check_same_f32(h[k], f[k], rows, f"{fam}.{k}")
    once(op, shape, {k: (h[k], f[k]) for k in ("y", "dx")})


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows,cols", RO.ROWLN_SHAPES)
def test_row_layernorm(ops, lib, rows, cols, relu):
    """egk_rowln_fwd / _bwd: ragged and unvectorised widths (40, 250), the exact-width 1024 kernel, NV > 4 (1280) and the
    workgroup-per-row kernels (2048, 4096)."""
    inp = RO.rowln_inputs(rows, cols, RO.ROWLN_SEEDS.get((rows, cols, relu), 0))
    f, h = (_rowln(ops, lib, inp, dt, relu) for dt in DTS)
    _ln_checks("rowln" + ("+relu" if relu else ""), (rows, cols), f, h, RO.rowln_model(inp, torch.float64, relu), "rowln",
               ("mean", "rstd", "dw", "db"))


def test_row_layernorm_with_dropout(ops):
    """ops.row_layernorm(relu, p = 0.5) under the same ops.manual_seed: the keep masks bit-equal, y and dx round once."""
    rows, cols, p = RO.ROWLN_DROPOUT
    inp = RO.rowln_inputs(rows, cols, seed=1)
    runs = []
    for dt in DTS:
        ops.manual_seed(1234)
        x = act(inp["x"], dt).requires_grad_(True)
        y = ops.row_layernorm(x, inp["w"].to(DEV), inp["b"].to(DEV), RO.EPS, relu=True, p=p, training=True)
        mask = ops.last_rowln_mask(y)
        y.backward(act(inp["dy"], dt))
        runs.append(dict(y=y.detach(), dx=x.grad, mask=mask))
    f, h = runs
    assert f["mask"].dtype == torch.uint8 and abs(float(f["mask"].float().mean()) - (1 - p)) < 0.02
    RO.check_same_f32(h["mask"], f["mask"], 0, "mask")
    _ln_checks("rowln+relu+dropout", (rows, cols), f, h, RO.rowln_model(inp, torch.float64, True, f["mask"].cpu(), p), "rowln", ())


def test_row_layernorm_grouped_launch(ops, lib):
    """egk_rowln_group_fwd / _bwd at cols 256, row ranges [64, 192, 5], each with its own affine pair."""
    cols, rows = RO.ROWLN_GROUP
    inp = RO.rowln_group_inputs()
    G, n = len(rows), sum(rows)
    ptr = list(itertools.accumulate([0] + rows))
    row_ptr = (C.c_int32 * (G + 1))(*ptr)
    ws_, bs_ = [t.to(DEV) for t in inp["ws"]], [t.to(DEV) for t in inp["bs"]]
    P, s = ops._p, ops._stream()
    runs = []
    for dt in DTS:
        x, dy = act(inp["x"], dt), act(inp["dy"], dt)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, rstd = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        ok(lib.egk_rowln_group_fwd(s, P(x), ops._ptr_array(ws_), ops._ptr_array(bs_), row_ptr, G, P(y), P(mean), P(rstd), cols, RO.EPS, 1,
                                   ops._dt(x)))
        grid = lib.egk_rowln_bwd_ws_rows(max(rows))
        ws = torch.zeros(G * grid * 2 * cols, device=DEV)
        ok(lib.egk_rowln_group_bwd(s, P(dy), P(x), ops._ptr_array(ws_), ops._ptr_array(bs_), row_ptr, G, P(mean), P(rstd), P(dx), P(ws),
                                   cols, 1, ops._dt(x)))
        dws, dbs = [torch.zeros(cols, device=DEV) for _ in rows], [torch.zeros(cols, device=DEV) for _ in rows]
        for k in range(G):
            ok(lib.egk_ln_bwd_reduce(s, P(ws[k * grid * 2 * cols:]), P(dws[k]), P(dbs[k]), max(rows), cols, 0))
        torch.cuda.synchronize()
        runs.append([dict(y=y[ptr[k]:ptr[k + 1]], dx=dx[ptr[k]:ptr[k + 1]], mean=mean[ptr[k]:ptr[k + 1]], rstd=rstd[ptr[k]:ptr[k + 1]],
                          dw=dws[k], db=dbs[k]) for k in range(G)])
    ref = RO.rowln_group_model(inp, torch.float64)
    for k in range(G):
        _ln_checks("rowln_group", (rows[k], cols), runs[0][k], runs[1][k], ref[k], "rowln", ("mean", "rstd", "dw", "db"))


# ---------------------------------------------------------------------------------------------------------------------------
# graph LayerNorm + LeakyReLU: one launch each way, and statistics-then-apply
# ---------------------------------------------------------------------------------------------------------------------------
def _graphln(ops, lib, inp, dt, segs, split):
    x, dy, w, b = act(inp["x"], dt), act(inp["dy"], dt), inp["w"].to(DEV), inp["b"].to(DEV)
    rows, cols = x.shape
    n_seg = len(segs) - 1
    seg = torch.tensor(segs, dtype=torch.int32, device=DEV)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    stats = torch.empty(n_seg * 2, device=DEV)
    dw, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
    ws = torch.empty(lib.egk_graphln_ws_bytes(rows, cols, n_seg), dtype=torch.uint8, device=DEV)
    P, s, d = ops._p, ops._stream(), ops._dt(x)
    if not split:
        ok(lib.egk_graphln_fwd(s, P(x), P(w), P(b), P(y), P(stats), P(seg), n_seg, rows, cols, RO.EPS, RO.SLOPE, P(ws), d))
        ok(lib.egk_graphln_bwd(s, P(dy), P(x), P(w), P(b), P(stats), P(dx), P(dw), P(db), P(seg), n_seg, rows, cols, RO.EPS, RO.SLOPE,
                               P(ws), d))
    else:
        nb = lib.egk_graphln_stats_blocks(rows)
        part = torch.empty(nb * n_seg * 2, dtype=torch.float64, device=DEV)
        ok(lib.egk_graphln_stats(s, P(x), P(seg), n_seg, rows, cols, P(part), d))
        ok(lib.egk_graphln_fwd_apply(s, P(x), P(w), P(b), P(y), P(stats), P(seg), n_seg, rows, cols, RO.EPS, RO.SLOPE, P(part), nb, d))
        ok(lib.egk_graphln_bwd_stats(s, P(dy), P(x), P(w), P(b), P(stats), P(seg), n_seg, rows, cols, RO.SLOPE, P(ws), d))
        ok(lib.egk_graphln_bwd_finish(s, P(dy), P(x), P(w), P(b), P(stats), P(dx), P(dw), P(db), P(seg), n_seg, rows, cols, RO.EPS,
                                      RO.SLOPE, P(ws), nb, P(ws), d))
    torch.cuda.synchronize()
    return dict(y=y, dx=dx, stats=stats, dw=dw, db=db)


@pytest.mark.parametrize("split", [False, True], ids=["one_launch", "stats_then_apply"])
@pytest.mark.parametrize("rows,cols,segs", RO.GRAPHLN_CASES)
def test_graph_layernorm(ops, lib, rows, cols, segs, split):
    """egk_graphln_fwd / _bwd, and egk_graphln_stats + _fwd_apply / _bwd_stats + _bwd_finish: the bf16 backward as a kernel."""
    inp = RO.graphln_inputs(rows, cols)
    f, h = (_graphln(ops, lib, inp, dt, segs, split) for dt in DTS)
    _ln_checks("graphln" + ("_split" if split else ""), (rows, cols, len(segs) - 1), f, h, RO.graphln_model(inp, torch.float64, segs),
               "graphln", ("stats", "dw", "db"))


# ---------------------------------------------------------------------------------------------------------------------------
# CSR gathers, PE add
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", RO.CSR_COLS)
@pytest.mark.parametrize("kind", RO.CSR_GRAPHS)
def test_csr_gather(ops, kind, cols):
    """Forward mean and the transposed, weighted, gated orientation of the backward: light rows, heavy_mode 1 (a fan-out node with
    31 edges) and rows cut over several workgroups (69 edges)."""
    from egopack_amd import data as D
    ei, n = RO.csr_edges(kind)
    graph = D.build_csr(ei, n)
    want = {"light": (0, 0, 0), "heavy1": (1, 1, 1), "cut": (1, 0, 0)}[kind]
    assert (int(graph.t_heavy.numel() > 0), graph.heavy_mode, graph.t_heavy_mode) == want
    gd = graph.to(DEV)
    inp = RO.csr_inputs(n, cols, RO.CSR_SEED)
    runs = []
    for dt in DTS:
        x, gate = act(inp["x"], dt), act(inp["gate"], dt)
        fwd, bwd = torch.empty_like(x), torch.empty_like(x)
        ops._csr_gather(x, gd.rowptr, gd.col, None, None, fwd, gd.heavy, gd.heavy_mode)
        ops._csr_gather(x, gd.t_rowptr, gd.t_col, gd.t_wgt, gate, bwd, gd.t_heavy, gd.t_heavy_mode)
        torch.cuda.synchronize()
        runs.append(dict(fwd=fwd, bwd=bwd))
    f, h = runs
    ref = RO.csr_model(inp, torch.float64, ei, n)
    for k in ("fwd", "bwd"):
        RO.close_to_model(f[k], ref[k], "csr")
    once(f"csr_{kind}", (n, cols), {k: (h[k], f[k]) for k in ("fwd", "bwd")})


@pytest.mark.parametrize("cols", RO.BANDED_COLS)
def test_banded_gather(ops, cols):
    from egopack_amd import data as D
    ei, n = RO.band_edges()
    gd = D.build_csr(ei, n).to(DEV)
    assert not bool((gd.band == 0xFF).any())
    inp = RO.csr_inputs(n, cols, RO.BAND_SEED)
    runs = []
    for dt in DTS:
        x = act(inp["x"], dt)
        out = torch.empty_like(x)
        ops._csr_gather(x, gd.rowptr, gd.col, None, None, out, gd.heavy, gd.heavy_mode, band=gd.band)
        torch.cuda.synchronize()
        runs.append(out)
    RO.close_to_model(runs[0], RO.csr_model(inp, torch.float64, ei, n)["fwd"], "csr")
    once("csr_banded", (n, cols), {"fwd": (runs[1], runs[0])})


@pytest.mark.parametrize("table", [False, True], ids=["direct", "table"])
@pytest.mark.parametrize("cols", RO.PE_COLS)
def test_pe_add(ops, cols, table):
    """ops.pe_add, evaluated per node and from the per-position table; dx is the incoming gradient itself."""
    inp = RO.pe_inputs(cols, RO.PE_SEED)
    pos, freq = inp["pos"].to(DEV), inp["freq"].to(DEV)
    dy = RO.r16(torch.randn(inp["x"].shape, generator=RO.gen(cols)))
    runs = []
    for dt in DTS:
        x = act(inp["x"], dt).requires_grad_(True)
        y = ops.pe_add(x, pos, freq, pos_range=(-64, 63) if table else None)
        y.backward(act(dy, dt))
        runs.append(dict(y=y.detach(), dx=x.grad))
    f, h = runs
    RO.close_to_model(f["y"], RO.pe_model(inp, torch.float64)["y"], "pe")
    assert torch.equal(f["dx"].cpu(), dy)
    once("pe_add_" + ("table" if table else "direct"), tuple(inp["x"].shape), {"y": (h["y"], f["y"])})
    once("pe_add_" + ("table" if table else "direct"), tuple(inp["x"].shape), {"dx": (h["dx"], f["dx"])}, cap=0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# maxima: no arithmetic, so no flips; winners bit-equal
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,H", RO.GATHER_MAX)
def test_gather_max(ops, lib, k, H):
    """ops.gather_max forward and backward per task, and egk_gather_max_group_fwd over the three tasks in one launch: bf16 f, f32
    banks.  m = bf16(max) exactly, the winners bit-equal, df exactly the routed dm."""
    inp = RO.gather_max_inputs(k, H)
    N, G = inp["N"], len(inp["banks"])
    banks, nns = [t.to(DEV) for t in inp["banks"]], [t.to(DEV) for t in inp["nns"]]
    runs = []
    for dt in DTS:
        ms, args, dfs = [], [], []
        for i in range(G):
            f = act(inp["f"][i * N:(i + 1) * N], dt).requires_grad_(True)
            m = ops.gather_max(f, banks[i], nns[i])
            args.append(m.grad_fn.saved_tensors[0])
            m.backward(act(inp["dm"][i * N:(i + 1) * N], dt))
            ms.append(m.detach())
            dfs.append(f.grad)
        fall = act(inp["f"], dt)
        gm, garg = torch.empty_like(fall), torch.empty((G * N, H), dtype=torch.uint8, device=DEV)
        ok(lib.egk_gather_max_group_fwd(ops._stream(), ops._p(fall), ops._ptr_array(banks), ops._ptr_array(nns), G, ops._p(gm), ops._p(garg),
                                        N, H, k, ops._dt(fall)))
        torch.cuda.synchronize()
        runs.append(dict(m=torch.cat(ms), arg=torch.cat(args), df=torch.cat(dfs), gm=gm, garg=garg))
    f, h = runs
    ref = torch.cat([torch.cat([inp["banks"][i][inp["nns"][i]], inp["f"][i * N:(i + 1) * N].unsqueeze(1)], 1).max(1).values for i in range(G)])
    assert torch.equal(f["m"].cpu(), ref) and torch.equal(f["gm"].cpu(), ref)  # a maximum is exact
    assert torch.equal(f["df"].cpu(), inp["dm"] * (f["arg"].cpu() == k))
    assert int((f["arg"] == k).sum()) > 0 and int((f["arg"] < k).sum()) > 0
    RO.check_same_f32(h["arg"], f["arg"], 0, "winners")
    RO.check_same_f32(h["garg"], f["garg"], 0, "winners")
    RO.check_same_f32(f["garg"], f["arg"], 0, "winners")
    once("gather_max", (G * N, H, k), {"m": (h["m"], f["m"]), "group_m": (h["gm"], f["gm"]), "df": (h["df"], f["df"])}, cap=0.0)


@pytest.mark.parametrize("lens,cols", RO.SEGMAX)
def test_segment_max_and_its_multi_input_form(ops, lens, cols):
    inp = RO.segmax_inputs(lens, cols)
    ptr = inp["ptr"].to(DEV)
    runs = []
    for dt in DTS:
        xs = [act(x, dt).requires_grad_(True) for x in inp["xs"]]
        douts = [act(d, dt) for d in inp["douts"]]
        out = ops.segment_max(xs[0], ptr)
        arg = out.grad_fn.saved_tensors[0]
        out.backward(douts[0])
        dx0, xs[0].grad = xs[0].grad, None
        outs = ops.segment_max_multi(xs, ptr)
        margs = outs[0].grad_fn.saved_tensors[0]
        torch.autograd.backward(outs, douts)
        runs.append(dict(out=out.detach(), arg=arg, dx=dx0, mout=torch.stack([o.detach() for o in outs]), marg=margs,
                         mdx=torch.stack([x.grad for x in xs])))
    f, h = runs
    lo, hi = inp["ptr"][:-1].tolist(), inp["ptr"][1:].tolist()
    for j, x in enumerate(inp["xs"]):
        ref = torch.stack([x[a:b].max(0).values if b > a else torch.zeros(cols) for a, b in zip(lo, hi)])
        assert torch.equal(f["mout"][j].cpu(), ref)
        rdx = torch.zeros_like(x)
        for sgm, (a, b) in enumerate(zip(lo, hi)):
            if b > a:
                rdx[f["marg"][j][sgm].cpu().long(), torch.arange(cols)] = inp["douts"][j][sgm]
        assert torch.equal(f["mdx"][j].cpu(), rdx)
    assert torch.equal(f["out"], f["mout"][0]) and torch.equal(f["dx"], f["mdx"][0])
    RO.check_same_f32(h["arg"], f["arg"], 0, "winners")
    RO.check_same_f32(h["marg"], f["marg"], 0, "winners")
    once("segment_max", (len(lens), cols), {k: (h[k], f[k]) for k in ("out", "dx", "mout", "mdx")}, cap=0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# dropout, ReLU gate, casts, gathers, norms, column sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 0.3])
@pytest.mark.parametrize("n", RO.DROPOUT_N)
def test_dropout_and_relu_gate(ops, lib, n, p):
    """egk_dropout_fwd / _bwd with the same seed and offset: masks bit-equal; p = 0.5 scales by 2 (exact), p = 0.3 rounds once.
    egk_relu_gate: dx = y > 0 ? dy : 0, exact."""
    inp = RO.dropout_inputs(n)
    P, s = ops._p, ops._stream()
    runs = []
    for dt in DTS:
        x, dy = act(inp["x"], dt), act(inp["dy"], dt)
        y, dx, gated = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        mask = torch.empty(n, dtype=torch.uint8, device=DEV)
        ok(lib.egk_dropout_fwd(s, P(x), P(y), P(mask), n, p, 4321, 96, None, ops._dt(x)))
        ok(lib.egk_dropout_bwd(s, P(dy), P(mask), P(dx), n, p, ops._dt(x)))
        ok(lib.egk_relu_gate(s, P(dy), P(x), P(gated), n, ops._dt(x)))
        torch.cuda.synchronize()
        runs.append(dict(y=y, dx=dx, mask=mask, gated=gated))
    f, h = runs
    RO.check_same_f32(h["mask"], f["mask"], 0, "mask")
    assert abs(float(f["mask"].float().mean()) - (1 - p)) < 0.03
    ref = RO.dropout_model(inp, torch.float64, f["mask"].cpu(), p)
    for k in ("y", "dx"):
        RO.close_to_model(f[k], ref[k], "dropout")
    assert torch.equal(f["gated"].cpu(), inp["dy"] * (inp["x"] > 0))
    once(f"dropout_p{p}", (n,), {k: (h[k], f[k]) for k in ("y", "dx")}, cap=0.0 if p == 0.5 else RO.CAP)
    once("relu_gate", (n,), {"dx": (h["gated"], f["gated"])}, cap=0.0)


@pytest.mark.parametrize("rows,cols", [(37, 250), (5, 1024)])
def test_row_casts_and_gathers_are_exact(ops, lib, rows, cols):
    """egk_cast_rows and egk_gather_rows over the four table / output type pairs on representable values: the same values."""
    g = RO.gen(rows + cols)
    src = RO.r16(torch.randn(rows, cols, generator=g))
    idx = torch.randint(-2, rows + 2, (3 * rows,), generator=g)
    want = torch.where(((idx >= 0) & (idx < rows))[:, None], src[idx.clamp(0, rows - 1)], torch.zeros(1))
    P, s = ops._p, ops._stream()
    idx_d = idx.to(DEV)
    for a, b in itertools.product(DTS, DTS):
        t = act(src, a)
        cast = torch.empty(rows, cols, dtype=b, device=DEV)
        ok(lib.egk_cast_rows(s, P(t), ops._dt(t), cols, P(cast), ops._dt(cast), cols, rows, cols, 0))
        out = torch.empty(idx.numel(), cols, dtype=b, device=DEV)
        ok(lib.egk_gather_rows(s, P(t), ops._dt(t), cols, rows, P(idx_d), P(out), ops._dt(out), idx.numel(), cols))
        torch.cuda.synchronize()
        assert torch.equal(cast.float().cpu(), src) and torch.equal(out.float().cpu(), want)


@pytest.mark.parametrize("rows,cols", [(37, 260), (130, 250), (9, 1024)])
def test_row_norms_and_column_sums_read_bf16_as_the_same_values(ops, lib, rows, cols):
    """egk_row_inv_norm, egk_row_sq_norm, egk_colsum with bf16 and f32 input of the same values: f32 outputs, no storage rounding."""
    x = RO.r16(torch.randn(rows, cols, generator=RO.gen(rows * cols)) + 0.1)
    P, s = ops._p, ops._stream()
    runs = []
    for dt in DTS:
        xd = act(x, dt)
        inv, sq, cs = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV), torch.empty(cols, device=DEV)
        ws = torch.empty(lib.egk_colsum_ws_len(rows, cols), device=DEV)
        ok(lib.egk_row_inv_norm(s, P(xd), P(inv), rows, cols, ops._dt(xd)))
        ok(lib.egk_row_sq_norm(s, P(xd), P(sq), rows, cols, ops._dt(xd)))
        ok(lib.egk_colsum(s, P(xd), cols, rows, cols, P(cs), 0, P(ws), ops._dt(xd)))
        torch.cuda.synchronize()
        runs.append(dict(inv=inv, sq=sq, cs=cs))
    f, h = runs
    xd = x.double()
    for k, ref, tol in (("inv", 1 / xd.norm(dim=1), "norm"), ("sq", (xd * xd).sum(1), "norm"), ("cs", xd.sum(0), "colsum")):
        RO.close_to_model(f[k], ref, tol)
        RO.check_same_f32(h[k], f[k], 0, tol)


# ---------------------------------------------------------------------------------------------------------------------------
# contraction epilogue
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [None, 0], ids=["policy", "generic"])
@pytest.mark.parametrize("M,N,K", RO.GEMM_SHAPES)
def test_contraction_epilogue(ops, lib, M, N, K, pipeline):
    """ops.gemm with bf16 operands, bias, ReLU and a bf16 residual, once with f32 and once with bf16 output: the accumulators are
    the same bits, the epilogue the same f32 operations -- the bf16 output is the rounding of the f32 output."""
    inp = RO.gemm_inputs(M, N, K, RO.GEMM_SEED)
    A, B, res, bias = act(inp["A"], BF), act(inp["B"], BF), act(inp["res"], BF), inp["bias"].to(DEV)
    prev = lib.egk_gemm_set_pipeline(pipeline) if pipeline is not None else None
    try:
        outs = []
        for dt in DTS:
            out = torch.empty(M, N, device=DEV, dtype=dt)
            ops.gemm(M, N, A, K, B, K, K, out, N, bias=bias, residual=res, ldr=N, act=1)
            torch.cuda.synchronize()
            outs.append(out)
    finally:
        if prev is not None:
            lib.egk_gemm_set_pipeline(prev)
    RO.close_to_model(outs[0], RO.gemm_model(inp, torch.float64)["c"], "gemm")
    once("gemm_" + ("policy" if pipeline is None else "generic"), (M, N, K), {"c": (outs[1], outs[0])})


# ---------------------------------------------------------------------------------------------------------------------------
# the heads with a designed second rounding
# ---------------------------------------------------------------------------------------------------------------------------
def _near_midpoint(g, seed):
    """Elements of the f64 gradient so close to a bf16 rounding midpoint that the kernel's f32 evaluation (expf, and the
    cancellation of sigmoid(z) - 1) may round to the other neighbour."""
    lo, hi = RO.bracket(g.float())
    mid = (lo.double() + hi.double()) / 2
    return (lo != hi) & ((g - mid).abs() <= 1e-4 * g.abs() + 1e-6 * seed)


@pytest.mark.parametrize("rows,cols", RO.HEAD_SHAPES)
@pytest.mark.parametrize("n_out", [1, 2], ids=["linear1_bce", "linear2_ce"])
def test_heads_round_their_loss_gradient_to_the_operand_type(ops, rows, cols, n_out):
    """ops.linear1_bce / ops.linear2_ce.  Their bf16 form has a DESIGNED second rounding (egk_rowdot_bce / egk_rowdot_ce2 in
    egopack_hip.h): the logit gradient g = seed * dloss/dz is rounded to bf16 -- the operand type of the contraction path these
    launches replace -- before df = g W, dW = g^T f, db = sum g.  So the bf16 df is NOT the rounding of the f32 df, and the pair is
    not handed to the helper.  The model, in fp64: z = f W^T + b; loss(z); g; g16 = bf16(g); df16 = g16 W.  A product of two bf16
    values is exact in f32 and the two-logit form adds two of them with one fma, so the bf16 df must be EXACTLY bf16(df16): the
    helper with cap 0 against the model.  Where the f64 g lies within 1e-4 relative of a rounding midpoint the kernel's f32
    evaluation may pick either neighbour: there the neighbour that explains the row of df is taken, and it must explain it exactly.
    dW and db of the bf16 run follow from the same g16 at the f32 tolerance; logits and loss carry no rounding at all.  The f32 form
    is pinned to the unrounded model at the tolerances of its test in test_gpu_kernels.py."""
    smoothing = 0.1 if n_out == 2 else 0.0
    inp = RO.head_inputs(rows, cols, n_out)
    m = RO.head_model(inp, n_out, smoothing)
    seed, y = inp["seed"], inp["y"].to(DEV)
    runs = []
    for dt, mode in zip(DTS, ("f32", "bf16")):
        with ops.compute_mode(mode):
            f = act(inp["f"], dt).requires_grad_(True)
            W, b = inp["W"].to(DEV).requires_grad_(True), inp["b"].to(DEV).requires_grad_(True)
            with ops.loss_seed(seed):
                if n_out == 1:
                    assert ops.linear1_bce_ok(f, W)
                    loss, logits = ops.linear1_bce(f, W, b, y)
                else:
                    assert ops.linear2_ce_ok(rows, f, W)
                    loss, logits = ops.linear2_ce(f, W, b, y, smoothing)
            loss.backward(torch.full_like(loss, seed))
            torch.cuda.synchronize()
            runs.append(dict(loss=loss.detach(), logits=logits.detach(), df=f.grad, dw=W.grad, db=b.grad))
    f, h = runs
    for k in ("logits", "loss"):
        RO.close_to_model(f[k], m[k], f"head.{k}")
        RO.check_same_f32(h[k], f[k], 0, f"head.{k}")
    gscale, wscale = float(m["df"].abs().max()), float(m["dw"].abs().max())
    dbtol = 2e-5 * max(1.0, float(m["db"].abs().max()) * 100)
    assert float((f["df"].cpu().double() - m["df"]).abs().max()) <= 1e-5 * gscale
    assert float((f["dw"].cpu().double() - m["dw"]).abs().max()) <= 2e-5 * wscale
    assert float((f["db"].cpu().double() - m["db"]).abs().max()) <= dbtol
    # the bf16 form: pick g16 per row (the RNE neighbour unless the f64 value is at a midpoint), then everything is exact
    Wd, g16, df_h = inp["W"].double(), m["g16"].clone(), h["df"].cpu()
    near = _near_midpoint(m["g"], seed)
    lo, hi = RO.bracket(m["g"].float())
    for r in near.any(1).nonzero().flatten().tolist():
        cands = [torch.stack(c) for c in itertools.product(*[(lo[r, j].double(), hi[r, j].double()) if near[r, j] else (g16[r, j],)
                                                               for j in range(n_out)])]
        g16[r] = min(cands, key=lambda c: float(((c @ Wd).float().to(BF).float() - df_h[r].float()).abs().sum()))
    print(f"head n_out={n_out} ({rows}, {cols}): {int(near.any(1).sum())} rows with a gradient at a rounding midpoint")
    once("linear1_bce" if n_out == 1 else "linear2_ce", (rows, cols), {"df_vs_model": (h["df"], (g16 @ Wd).float())}, cap=0.0)
    assert float((h["dw"].cpu().double() - g16.t() @ inp["f"].double()).abs().max()) <= 2e-5 * wscale
    assert float((h["db"].cpu().double() - g16.sum(0)).abs().max()) <= dbtol
    if n_out == 2:
        assert float(h["df"][::5].float().abs().max()) == 0.0 and float(h["loss"][::5].abs().max()) == 0.0
