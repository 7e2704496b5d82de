"""The rows epilogue of the pipelined contractions: the descriptor-once, mode-specialised store loop (egk_gemm_set_pipeline(891),
the default) against the branch-ladder loop it replaces (890), against the generic kernel (egk_gemm_set_pipeline(0): its own
epilogue, which shares no code with either) and against f64 products.

Shapes: M in {192 + 8, 3 * 128 + 40} (a ragged last tile, more than one tile row), N in {128, 136} (a column tile whose groups of 8
columns are partly outside N), K in {64, 192} (one and three K tiles) and K = 256 (four K tiles: the fewest at which the 192 x 128
tile runs with its loader waves, whose compute waves fetch the epilogue's operands at kernel entry).

Bounds:
  * new loop == old loop, new loop == generic kernel: bit for bit (torch.equal);
  * against f64 products of the bf16 operands: rtol 2e-2 / atol 2e-1 (the bounds of test_gemm_192_row_tile_with_loader_waves_bit_equal,
    for bf16 operands at these K);
  * st_ws against f64 sums of the stored values: a thread adds at most 192 * 8 terms in f32 (sequential summation of n terms:
    |error| <= n * 2^-24 * sum |term|), the rest is f64 -- so 1536 * 2^-24 * sum |term| per (tile, segment, moment).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
TILE_ROWS = {3: 128, 8: 96, 11: 64, 16: 192}
SHAPES = [(M, N, K) for M in (192 + 8, 3 * 128 + 40) for N in (128, 136) for K in (64, 192)] + [(200, 128, 256), (424, 136, 256)]
U32 = 2.0 ** -24
SLOPE = 0.125


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from egopack_amd import _lib
    return _lib.load()


class knobs:
    """Forced tile variant, loader waves on / off, new / old store loop -- restored on exit."""

    def __init__(self, lib, tile, loaders=1, fast=1):
        self.lib, self.tile, self.loaders, self.fast = lib, tile, loaders, fast

    def __enter__(self):
        self.prev = self.lib.egk_gemm_set_pipeline(self.tile)
        self.lib.egk_gemm_set_pipeline(870 + self.loaders)
        self.lib.egk_gemm_set_pipeline(890 + self.fast)

    def __exit__(self, *exc):
        self.lib.egk_gemm_set_pipeline(871)
        self.lib.egk_gemm_set_pipeline(891)
        self.lib.egk_gemm_set_pipeline(self.prev)


_inputs = {}


def inputs(M, N, K, tb):
    """Operands and their f64 product, computed once per shape and shared (never written)."""
    key = (M, N, K, tb)
    if key not in _inputs:
        g = torch.Generator(device=DEV).manual_seed(1000 * M + 10 * N + K + int(tb))
        r = lambda *s: torch.randn(*s, device=DEV, generator=g)
        A = r(M, K).to(BF)
        B = r(*((K, N) if tb else (N, K))).to(BF)
        d = dict(A=A, B=B, bias=r(N), C0=r(M, N), res16=r(M, N).to(BF), res32=r(M, N), x16=r(M, N).to(BF), w=r(N), b=r(N))
        d["prod"] = A.double() @ (B.double() if tb else B.double().t())
        _inputs[key] = d
    return _inputs[key]


def segments(M, tile_rows):
    """Two row segments whose boundary falls inside a tile, each at least one tile high; one segment where M is too short."""
    if M >= 2 * tile_rows + 8:
        cut = 200 if M == 424 else M // 2
        assert cut % tile_rows != 0
        return [0, cut, M]
    return [0, M]


def run_mode(ops, mode, M, N, K, tb, tile_rows, slabs=True):
    """One launch of ``mode`` under the knobs in force: dict of the tensors it wrote."""
    i = inputs(M, N, K, tb)
    args = lambda out: (M, N, i["A"], K, i["B"], i["B"].shape[1], K, out, N)
    kw = dict(transB=tb, compute=ops.BF16, allow_splitk=False)
    if mode in ("bias", "bias_relu", "alpha", "res_bf16", "res_f32", "bias_f32"):
        out = torch.zeros(M, N, device=DEV, dtype=torch.float32 if mode == "bias_f32" else BF)
        extra = dict(bias_relu=dict(act=1), alpha=dict(alpha=0.375), res_bf16=dict(residual=i["res16"], ldr=N),
                     res_f32=dict(residual=i["res32"], ldr=N)).get(mode, {})
        ops.gemm(*args(out), bias=i["bias"], **extra, **kw)
        return dict(C=out)
    if mode in ("f32", "f32_acc"):
        out = i["C0"].clone() if mode == "f32_acc" else torch.zeros(M, N, device=DEV)
        ops.gemm(*args(out), accumulate=mode == "f32_acc", **kw)
        return dict(C=out)
    if mode == "splitk2":
        out = torch.zeros(M, N, device=DEV)
        kw2 = dict(kw, allow_splitk=True)
        ops.gemm(*args(out), bias=i["bias"], splitk=2, **kw2)
        got = dict(C=out)
        if slabs:  # (the pipelined kernels leave their two slabs on request; the generic kernel does not)
            ws = ops.gemm(*args(torch.zeros(M, N, device=DEV)), bias=i["bias"], splitk=2, defer_reduce=True, **kw2)
            assert ws is not None
            got["slabs"] = ws.view(torch.float32).view(2, M, N).clone()
        return got
    if mode in ("st1", "st2"):
        ptr = segments(M, tile_rows)
        seg_ptr = torch.tensor(ptr, dtype=torch.int32, device=DEV)
        out = torch.zeros(M, N, device=DEV, dtype=BF)
        req = dict(mode=1 if mode == "st1" else 2, seg_ptr=seg_ptr, n_seg=len(ptr) - 1, min_rows=tile_rows)
        kws = dict(transB=tb, compute=ops.BF16)  # (no split-K option: the statistics need the finished tile)
        if mode == "st1":
            kws["bias"] = i["bias"]
        else:
            st = torch.tensor([[0.1 * s - 0.05, 1.5 - 0.25 * s] for s in range(len(ptr) - 1)], dtype=torch.float32, device=DEV)
            req.update(x=i["x16"], stats=st, w=i["w"], b=i["b"], slope=SLOPE)
        got = ops._gemm_with_stats(args(out), kws, req)
        assert got is not None, "the forced tile variant must take the statistics epilogue"
        return dict(C=out, st_ws=got[0].view(got[1], len(ptr) - 1, 2).clone(), ptr=ptr, st=req.get("stats"))
    raise AssertionError(mode)


def f64_reference(mode, i):
    p = i["prod"]
    if mode in ("bias", "bias_f32", "st1", "splitk2"):
        return p + i["bias"].double()
    if mode == "bias_relu":
        return torch.relu(p + i["bias"].double())
    if mode == "alpha":
        return 0.375 * p + i["bias"].double()
    if mode == "res_bf16":
        return p + i["bias"].double() + i["res16"].double()
    if mode == "res_f32":
        return p + i["bias"].double() + i["res32"].double()
    if mode == "f32_acc":
        return p + i["C0"].double()
    return p  # f32, st2


def check_st_ws(mode, got, i, N, tile_rows):
    """st_ws against f64 sums of the rounded C actually stored, per tile and segment."""
    C, ws, ptr = got["C"].double(), got["st_ws"], got["ptr"]
    M = C.shape[0]
    tiles_m, tiles_n = -(-M // tile_rows), -(-N // 128)
    assert ws.shape[0] == tiles_m * tiles_n
    if mode == "st1":
        t1, t2, slack = C, C * C, torch.zeros_like(C)
    else:
        seg_of_row = torch.bucketize(torch.arange(M, device=DEV), torch.tensor(ptr[1:-1], dtype=torch.long, device=DEV), right=True)
        mu, ri = got["st"][:, 0].double()[seg_of_row][:, None], got["st"][:, 1].double()[seg_of_row][:, None]
        w, b = i["w"].double(), i["b"].double()
        xh = (i["x16"].double() - mu) * ri
        pre = xh * w + b
        t1 = C * torch.where(pre > 0, 1.0, SLOPE) * w
        t2 = t1 * xh
        # a term whose pre-activation is within rounding of zero may take the other slope in f32
        near = pre.abs() <= 1e-5 * ((xh * w).abs() + b.abs())
        slack = torch.where(near, (C * w).abs() * (1 + xh.abs()), torch.zeros_like(C))
    for tm in range(tiles_m):
        for tn in range(tiles_n):
            for s in range(len(ptr) - 1):
                r0, r1 = max(tm * tile_rows, ptr[s]), min((tm + 1) * tile_rows, ptr[s + 1], M)
                c0, c1 = tn * 128, min((tn + 1) * 128, N)
                for k, t in enumerate((t1, t2)):
                    blk = t[r0:r1, c0:c1] if r1 > r0 else t[:0]
                    ref, mag = blk.sum().item(), blk.abs().sum().item()
                    # bound: 1536 f32 additions per thread (n * 2^-24 * sum |term|) + 8 roundings inside a mode-2 term; the rest is f64
                    bound = (1536 + 8) * U32 * mag + (slack[r0:r1, c0:c1].sum().item() if r1 > r0 else 0.0) + 1e-300
                    assert abs(ws[tm * tiles_n + tn, s, k].item() - ref) <= bound, (mode, tm, tn, s, k)


MODES = ["bias", "bias_relu", "alpha", "bias_f32", "f32", "f32_acc", "res_bf16", "res_f32", "splitk2", "st1", "st2"]


@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("tile,loaders", [(3, 1), (8, 1), (11, 1), (16, 0), (16, 1)])
def test_row_epilogue_modes(ops, lib, tile, loaders, tb):
    rows = TILE_ROWS[tile]
    for M, N, K in SHAPES:
        i = inputs(M, N, K, tb)
        for mode in MODES:
            with knobs(lib, tile, loaders, 1):
                new = run_mode(ops, mode, M, N, K, tb, rows)
            with knobs(lib, tile, loaders, 0):
                old = run_mode(ops, mode, M, N, K, tb, rows)
            tag = (mode, M, N, K)
            # 1. new loop against old loop
            assert torch.equal(new["C"], old["C"]), tag
            if mode == "splitk2":
                assert "slabs" in new and torch.equal(new["slabs"], old["slabs"]), tag
                torch.testing.assert_close(new["slabs"].double().sum(0), i["prod"], rtol=2e-2, atol=2e-1)
            if mode in ("st1", "st2"):
                assert torch.equal(new["st_ws"], old["st_ws"]), tag
                check_st_ws(mode, new, i, N, rows)  # 4.
            else:  # 2. against the generic kernel (no statistics epilogue there)
                with knobs(lib, 0, loaders, 1):
                    generic = run_mode(ops, mode, M, N, K, tb, rows, slabs=False)
                assert torch.equal(new["C"], generic["C"]), tag
            # 3. against the f64 product
            torch.testing.assert_close(new["C"].double(), f64_reference(mode, i), rtol=2e-2, atol=2e-1)


@pytest.mark.parametrize("tile", [3, 8, 11])
@pytest.mark.parametrize("tb", [False, True])
def test_row_epilogue_grouped_launch(ops, lib, tile, tb):
    """A grouped launch of three problems of different row counts: new loop == old loop == the generic kernel problem by problem."""
    N, K = 136, 192
    rows = (200, 424, 72)
    g = torch.Generator(device=DEV).manual_seed(tile + int(tb))
    A = [torch.randn(m, K, device=DEV, generator=g).to(BF) for m in rows]
    B = [torch.randn(*((K, N) if tb else (N, K)), device=DEV, generator=g).to(BF) for _ in rows]
    bias = [torch.randn(N, device=DEV, generator=g) for _ in rows]

    def grouped():
        outs = [torch.zeros(m, N, device=DEV, dtype=BF) for m in rows]
        ops.gemm_grouped([((m, N, A[p], K, B[p], B[p].shape[1], K, outs[p], N), dict(transB=tb, bias=bias[p], act=1, compute=ops.BF16))
                          for p, m in enumerate(rows)])
        return outs

    with knobs(lib, tile, 1, 1):
        new = grouped()
    with knobs(lib, tile, 1, 0):
        old = grouped()
    with knobs(lib, 0, 1, 1):
        generic = []
        for p, m in enumerate(rows):
            out = torch.zeros(m, N, device=DEV, dtype=BF)
            ops.gemm(m, N, A[p], K, B[p], B[p].shape[1], K, out, N, transB=tb, bias=bias[p], act=1, compute=ops.BF16, allow_splitk=False)
            generic.append(out)
    for p in range(len(rows)):
        assert torch.equal(new[p], old[p]) and torch.equal(new[p], generic[p]), p
        ref = torch.relu(A[p].double() @ (B[p].double() if tb else B[p].double().t()) + bias[p].double())
        torch.testing.assert_close(new[p].double(), ref, rtol=2e-2, atol=2e-1)


@pytest.mark.parametrize("tb", [False, True])
def test_row_epilogue_grouped_192_row_tile(ops, lib, tb):
    """The grouped launch that the policy puts on the 192 x 128 tile with loader waves (one round of such tiles that more than half
    fills the chip: the projection heads of three task batches), ragged row counts: new == old == generic."""
    N, K = 1024, 512
    rows = (64, 2048, 2000)
    g = torch.Generator(device=DEV).manual_seed(7 + int(tb))
    A = [torch.randn(m, K, device=DEV, generator=g).to(BF) for m in rows]
    B = [torch.randn(*((K, N) if tb else (N, K)), device=DEV, generator=g).to(BF) for _ in rows]
    bias = [torch.randn(N, device=DEV, generator=g) for _ in rows]
    res = [torch.randn(m, N, device=DEV, generator=g).to(BF) for m in rows]

    def grouped():
        outs = [torch.zeros(m, N, device=DEV, dtype=BF) for m in rows]
        ops.gemm_grouped([((m, N, A[p], K, B[p], B[p].shape[1], K, outs[p], N),
                           dict(transB=tb, bias=bias[p], residual=res[p], ldr=N, compute=ops.BF16)) for p, m in enumerate(rows)])
        return outs

    with knobs(lib, 1, 1, 1):
        new = grouped()
    with knobs(lib, 1, 1, 0):
        old = grouped()
    with knobs(lib, 0, 1, 1):
        generic = []
        for p, m in enumerate(rows):
            out = torch.zeros(m, N, device=DEV, dtype=BF)
            ops.gemm(m, N, A[p], K, B[p], B[p].shape[1], K, out, N, transB=tb, bias=bias[p], residual=res[p], ldr=N, compute=ops.BF16,
                     allow_splitk=False)
            generic.append(out)
    for p in range(len(rows)):
        assert torch.equal(new[p], old[p]) and torch.equal(new[p], generic[p]), p
        ref = A[p].double() @ (B[p].double() if tb else B[p].double().t()) + bias[p].double() + res[p].double()
        torch.testing.assert_close(new[p].double(), ref, rtol=2e-2, atol=2e-1)


@pytest.mark.parametrize("with_dbias", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
def test_row_epilogue_weight_gradient_form(ops, lib, accumulate, with_dbias):
    """tt on the 128 x 128 tile with an f32 result, stored and accumulated, with and without the fused bias gradient."""
    for M, N, K in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(M + N + K)
        A = torch.randn(K, M, device=DEV, generator=g).to(BF)  # op(A) = A^T
        B = torch.randn(K, N, device=DEV, generator=g).to(BF)
        C0 = torch.randn(M, N, device=DEV, generator=g)
        db0 = torch.randn(M, device=DEV, generator=g)

        def run():
            out, db = C0.clone(), db0.clone()
            ops.gemm(M, N, A, M, B, N, K, out, N, transA=True, transB=True, accumulate=accumulate, compute=ops.BF16,
                     allow_splitk=False, dbias=db if with_dbias else None, slot_final=False)
            return out, db

        with knobs(lib, 3, 1, 1):
            new = run()
        with knobs(lib, 3, 1, 0):
            old = run()
        with knobs(lib, 0, 1, 1):
            generic = run()
        assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]), (M, N, K)
        assert torch.equal(new[0], generic[0]), (M, N, K)
        ref = A.double().t() @ B.double() + (C0.double() if accumulate else 0)
        torch.testing.assert_close(new[0].double(), ref, rtol=2e-2, atol=2e-1)
        if with_dbias:  # (f32 sums of K bf16 values per row; the generic kernel's column sums run in another order)
            torch.testing.assert_close(new[1].double(), db0.double() + A.double().sum(0), rtol=1e-4, atol=1e-3)
