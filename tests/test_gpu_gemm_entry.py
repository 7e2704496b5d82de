"""The entry of the bf16 pipelined contractions: one descriptor batch at kernel entry and tile 0 requested piece by piece
(egk_gemm_set_pipeline(881), the default) against the kernels that read each descriptor field where it is first used (880) and
against the generic kernel (egk_gemm_set_pipeline(0), which shares no entry code with either): bit for bit (torch.equal) in every
case, plus one loose comparison with f64 products of the bf16 operands (rtol 2e-2 / atol 2e-1, the bounds of
test_gemm_192_row_tile_with_loader_waves_bit_equal for bf16 operands at these K) so that three equal wrong answers cannot pass.

The shapes are the smallest at which an entry can go wrong: K tiles against the ring depth (fewer than, exactly, one more than the
prologue issues, and the first steady-state round), a second K source that begins at tile 1 or at the last tile (the cursor is
re-initialised right behind the early issue), ragged last tiles, k-major operands with and without the fused bias gradient, grouped
launches whose virtual tiles belong to different problems, uneven split-K halves, and every mode of the rows epilogue (whose
operands the compute waves of the loader-wave tile fetch at entry).

The 192-row tile runs with its loader waves from four K tiles on (K >= 256); below that the same tile's compute waves issue their
own pieces.  Cases that name "the loader-wave tile" at a smaller K therefore run at that K AND at K = 256.
"""
import re
from pathlib import Path

import pytest
import torch

from tests import test_gpu_gemm_row_epilogue as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


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
    """Forced tile variant (0: the generic kernel) and the entry switch -- restored on exit."""

    def __init__(self, lib, tile, entry=1):
        self.lib, self.tile, self.entry = lib, tile, entry

    def __enter__(self):
        self.prev = self.lib.egk_gemm_set_pipeline(self.tile)
        assert self.lib.egk_gemm_set_pipeline(880 + self.entry) == 0

    def __exit__(self, *exc):
        self.lib.egk_gemm_set_pipeline(881)
        self.lib.egk_gemm_set_pipeline(self.prev)


def three_ways(lib, tile, run):
    """run() under the new entry, the old entry and the generic kernel."""
    with knobs(lib, tile, 1):
        new = run()
    with knobs(lib, tile, 0):
        old = run()
    with knobs(lib, 0, 1):
        generic = run()
    return new, old, generic


def rand(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return lambda *s: torch.randn(*s, device=DEV, generator=g)


def check(new, old, generic, ref, tag, generic_bits=True):
    assert torch.equal(new, old), tag
    if generic_bits:
        assert torch.equal(new, generic), tag
    else:  # two wave groups sum even and odd K tiles apart: equal to rounding only (test_gemm_pipelined_transposed_operands_...)
        torch.testing.assert_close(new, generic, rtol=1e-5, atol=2e-3)
    torch.testing.assert_close(new.double(), ref, rtol=2e-2, atol=2e-1)


def test_entry_switch_codes(lib):
    """880 / 881 are accepted and return 0, their unused neighbours change nothing and return -1, and the new entry is the default."""
    try:
        assert lib.egk_gemm_set_pipeline(880) == 0
        assert lib.egk_gemm_set_pipeline(881) == 0
        for code in (879, 882, 885):
            assert lib.egk_gemm_set_pipeline(code) == -1
    finally:
        lib.egk_gemm_set_pipeline(881)
    src = (Path(__file__).resolve().parents[1] / "egopack_amd" / "csrc" / "gemm.hip").read_text()
    assert re.search(r"^static int g_entry_fast = 1;", src, re.M), "the library starts with the new entry on"


@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("tile,M", [(16, 192), (3, 128)])
def test_entry_k_tiles_against_ring_depth(ops, lib, tile, M, tb):
    """One workgroup; 1 .. 4 K tiles on the 3-stage 192-row tile and the 2-stage 128-row tile (K = 256: the loader waves' first
    steady-state round), and 6 tiles."""
    N = 128
    for K in (64, 128, 192, 256, 384):
        r = rand(7 * K + M + int(tb))
        A, B, bias = r(M, K).to(BF), r(*((K, N) if tb else (N, K))).to(BF), r(N)

        def run():
            out = torch.zeros(M, N, device=DEV, dtype=BF)
            ops.gemm(M, N, A, K, B, B.shape[1], K, out, N, transB=tb, bias=bias, act=1, compute=ops.BF16, allow_splitk=False)
            return out

        ref = torch.relu(A.double() @ (B.double() if tb else B.double().t()) + bias.double())
        check(*three_ways(lib, tile, run), ref, (tile, M, K, tb))


@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("tile,M", [(16, 192), (3, 128)])
def test_entry_two_k_sources(ops, lib, tile, M, tb):
    """The SAGE combine form: the second source begins at tile 1 or at the last tile; (64, 192) and (192, 64) are the same on the
    loader waves (four K tiles)."""
    N = 128
    for K1, K2 in ((64, 64), (64, 128), (128, 64), (64, 192), (192, 64)):
        r = rand(K1 + 3 * K2 + M + int(tb))
        op = lambda rows, K, tr: r(*((K, rows) if tr else (rows, K))).to(BF)
        A1, A2, B1, B2 = op(M, K1, False), op(M, K2, False), op(N, K1, tb), op(N, K2, tb)

        def run():
            out = torch.zeros(M, N, device=DEV, dtype=BF)
            ops.gemm(M, N, A1, K1, B1, B1.shape[1], K1, out, N, A2=A2, lda2=K2, B2=B2, ldb2=B2.shape[1], K2=K2, transB=tb,
                     compute=ops.BF16, allow_splitk=False)
            return out

        prod = lambda a, b: a.double() @ (b.double() if tb else b.double().t())
        check(*three_ways(lib, tile, run), prod(A1, B1) + prod(A2, B2), (tile, K1, K2, tb))


@pytest.mark.parametrize("tile,M", [(16, 193), (16, 191), (3, 129)])
def test_entry_ragged_edges(ops, lib, tile, M):
    """A last row tile of one row, a first tile one row short, and a column tile partly outside N: the clamped rows of tile 0."""
    for N in (128, 136):
        for K in (64, 256):
            for tb in (False, True):
                r = rand(M + N + K + int(tb))
                A, B, bias = r(M, K).to(BF), r(*((K, N) if tb else (N, K))).to(BF), r(N)

                def run():
                    out = torch.zeros(M, N, device=DEV, dtype=BF)
                    ops.gemm(M, N, A, K, B, B.shape[1], K, out, N, transB=tb, bias=bias, compute=ops.BF16, allow_splitk=False)
                    return out

                ref = A.double() @ (B.double() if tb else B.double().t()) + bias.double()
                check(*three_ways(lib, tile, run), ref, (tile, M, N, K, tb))


@pytest.mark.parametrize("with_dbias", [False, True])
@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("tile", [3, 5])
def test_entry_k_major_operands(ops, lib, tile, tb, with_dbias):
    """tt and tn at M = N = 128 with the fused bias gradient (the workgroups of the first column tile) on and off; the two wave
    groups of variant 5 walk alternate K tiles (the same bits as the old entry; the generic kernel sums in another order)."""
    M = N = 128
    for K in (64, 128, 192):
        r = rand(K + tile + int(tb))
        A, B = r(K, M).to(BF), r(*((K, N) if tb else (N, K))).to(BF)
        C0, db0 = r(M, N), r(M)

        def run():
            out, db = C0.clone(), db0.clone()
            ops.gemm(M, N, A, M, B, B.shape[1], K, out, N, transA=True, transB=tb, accumulate=True, compute=ops.BF16,
                     allow_splitk=False, dbias=db if with_dbias else None, slot_final=False)
            return out, db

        new, old, generic = three_ways(lib, tile, run)
        ref = A.double().t() @ (B.double() if tb else B.double().t()) + C0.double()
        check(new[0], old[0], generic[0], ref, (tile, K, tb), generic_bits=tile == 3)
        assert torch.equal(new[1], old[1]), (tile, K, tb)
        if with_dbias:  # (f32 sums of K bf16 values per row; the generic kernel's column sums run in another order)
            torch.testing.assert_close(new[1].double(), db0.double() + A.double().sum(0), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("form", ["nn", "nt", "tt"])
def test_entry_grouped_launches(ops, lib, form):
    """Three problems of 64 / 192 / 384 rows in one launch: every XCD's run of virtual tiles crosses from one problem into the next.
    One and three K tiles; the policy's variant and every forced one of the form."""
    ta, tb = form[0] == "t", form[1] == "t"
    N, rows = 128, (64, 192, 384)
    for K in (64, 192):
        r = rand(K + len(form) + int(ta) + 2 * int(tb))
        A = [r(*((K, m) if ta else (m, K))).to(BF) for m in rows]
        B = [r(*((K, N) if tb else (N, K))).to(BF) for _ in rows]
        bias = [r(N) for _ in rows]
        kw = lambda p: dict(transA=ta, transB=tb, compute=ops.BF16, **({} if ta else dict(bias=bias[p], act=1)))
        dt = torch.float32 if ta else BF
        ref = [A[p].double().t() @ B[p].double() if ta else
               torch.relu(A[p].double() @ (B[p].double() if tb else B[p].double().t()) + bias[p].double()) for p in range(len(rows))]

        def grouped():
            outs = [torch.zeros(m, N, device=DEV, dtype=dt) for m in rows]
            ops.gemm_grouped([((m, N, A[p], A[p].shape[1], B[p], B[p].shape[1], K, outs[p], N), kw(p)) for p, m in enumerate(rows)])
            return outs

        with knobs(lib, 0, 1):
            generic = []
            for p, m in enumerate(rows):
                out = torch.zeros(m, N, device=DEV, dtype=dt)
                ops.gemm(m, N, A[p], A[p].shape[1], B[p], B[p].shape[1], K, out, N, allow_splitk=False, **kw(p))
                generic.append(out)
        for tile in ((1, 3, 13) if ta else (1, 3, 8, 11)):
            with knobs(lib, tile, 1):
                new = grouped()
            with knobs(lib, tile, 0):
                old = grouped()
            for p in range(len(rows)):
                check(new[p], old[p], generic[p], ref[p], (form, K, tile, p))


@pytest.mark.parametrize("tb", [False, True])
def test_entry_grouped_192_row_tile(ops, lib, tb):
    """The grouped launch that the policy puts on the 192 x 128 tile with loader waves (the projection heads of three task batches),
    ragged row counts."""
    N, K, rows = 1024, 512, (64, 2048, 2000)
    r = rand(11 + int(tb))
    A = [r(m, K).to(BF) for m in rows]
    B = [r(*((K, N) if tb else (N, K))).to(BF) for _ in rows]
    bias = [r(N) for _ in rows]

    def grouped():
        outs = [torch.zeros(m, N, device=DEV, dtype=BF) for m in rows]
        ops.gemm_grouped([((m, N, A[p], K, B[p], B[p].shape[1], K, outs[p], N), dict(transB=tb, bias=bias[p], compute=ops.BF16))
                          for p, m in enumerate(rows)])
        return outs

    with knobs(lib, 1, 1):
        new = grouped()
    with knobs(lib, 1, 0):
        old = grouped()
    with knobs(lib, 0, 1):
        for p, m in enumerate(rows):
            generic = torch.zeros(m, N, device=DEV, dtype=BF)
            ops.gemm(m, N, A[p], K, B[p], B[p].shape[1], K, generic, N, transB=tb, bias=bias[p], compute=ops.BF16, allow_splitk=False)
            ref = A[p].double() @ (B[p].double() if tb else B[p].double().t()) + bias[p].double()
            check(new[p], old[p], generic, ref, (tb, p))


@pytest.mark.parametrize("form", ["nn", "nt", "tt", "tn"])
@pytest.mark.parametrize("tile", [3, 5])
def test_entry_split_k_uneven_halves(ops, lib, tile, form):
    """Split-K = 2 over three K tiles (slab 0 walks two, slab 1 one) on the variants the policy lets split: 128 x 128 tiles with one
    and with two wave groups."""
    ta, tb = form[0] == "t", form[1] == "t"
    M = N = 128
    K = 192
    r = rand(tile + 2 * int(ta) + int(tb))
    A, B, bias = r(*((K, M) if ta else (M, K))).to(BF), r(*((K, N) if tb else (N, K))).to(BF), r(N)

    def run():
        out = torch.zeros(M, N, device=DEV)
        ops.gemm(M, N, A, A.shape[1], B, B.shape[1], K, out, N, transA=ta, transB=tb, bias=bias, compute=ops.BF16, splitk=2)
        return out

    ref = (A.double().t() if ta else A.double()) @ (B.double() if tb else B.double().t()) + bias.double()
    check(*three_ways(lib, tile, run), ref, (tile, form), generic_bits=tile == 3)


ROW_MODES = ["bias", "bias_relu", "res_bf16", "st1", "st2", "f32", "f32_acc", "splitk2"]


@pytest.mark.parametrize("K", [128, 256])
def test_entry_rows_epilogue_modes(ops, lib, K):
    """Every mode of the rows epilogue the step uses, once each at M = 192, N = 128 on the 192-row tile: K = 128 (its compute waves issue)
    and K = 256 (loader waves: the compute waves fetch the epilogue's operands at entry, beside the loaders' first requests).  The
    slab mode runs on 128-row tiles (the 192-row tile does not split)."""
    M, N, tb = 192, 128, False
    i = R.inputs(M, N, K, tb)

    def plain_bf16():  # (bf16 result, no bias: the mode R.run_mode has no name for)
        out = torch.zeros(M, N, device=DEV, dtype=BF)
        ops.gemm(M, N, i["A"], K, i["B"], K, K, out, N, compute=ops.BF16, allow_splitk=False)
        return dict(C=out)

    for mode in ["plain_bf16"] + ROW_MODES:
        run = plain_bf16 if mode == "plain_bf16" else (lambda: R.run_mode(ops, mode, M, N, K, tb, 192))
        with knobs(lib, 16, 1):
            new = run()
        with knobs(lib, 16, 0):
            old = run()
        assert torch.equal(new["C"], old["C"]), (mode, K)
        if mode == "splitk2":
            assert torch.equal(new["slabs"], old["slabs"]), K
        if mode in ("st1", "st2"):
            assert torch.equal(new["st_ws"], old["st_ws"]), (mode, K)
        else:  # (the generic kernel has no statistics epilogue)
            with knobs(lib, 0, 1):
                generic = plain_bf16() if mode == "plain_bf16" else R.run_mode(ops, mode, M, N, K, tb, 192, slabs=False)
            assert torch.equal(new["C"], generic["C"]), (mode, K)
        ref = i["prod"] if mode == "plain_bf16" else R.f64_reference(mode, i)
        torch.testing.assert_close(new["C"].double(), ref, rtol=2e-2, atol=2e-1)
