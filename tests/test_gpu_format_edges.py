"""Every f32 / bf16 / f16 conversion site of the library against the host models of tests/format_edges_common.py, bit for bit, on
the input set S of that module: every bf16 tie with both its neighbours, every exponent, the subnormal range, the finite -> inf
threshold, +-0, +-inf, NaNs and 2^20 random patterns.

The launches move values without arithmetic (a cast, a copy, a gather by the identity index, a contraction with the identity
matrix), so what a site stores IS its rounding.  Every comparison is ``same_bits``: a NaN input needs a NaN output, everything
else all 16 / 32 bits, zero's sign included; there is no tolerance (the one exception, named there: the residual ratios, which
are arithmetic).  S is laid out flat, in rows of 1536 columns (16-byte accesses) and in rows of 37 columns (element accesses),
and each test also holds the two layouts against each other element for element.

With EGK_FORMAT_EDGES_OUT=<file> the per-site mismatch counts by class and the NaN patterns each site produced are written there
(profiles/format_edges.txt); nothing asserts the NaN patterns.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import format_edges_common as FE

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = 0, 1  # EGK_F32, EGK_BF16
WIDE, NARROW = FE.WIDE_COLS, FE.NARROW_COLS
SENTINEL16, SENTINEL32 = 0x5A5A, 0x5A5A5A5A
_REC = []


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops as _ops
    yield _ops
    out = os.environ.get("EGK_FORMAT_EDGES_OUT")
    if out and _REC:
        with open(out, "w") as fh:
            fh.write("# site | elements | mismatches by class (" + " ".join(FE.CLASSES) + ") | what the site stored for NaN inputs\n")
            fh.writelines(line + "\n" for line in _REC)


@pytest.fixture(scope="module")
def lib(ops):
    from egopack_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def data(ops):
    """S and all bf16 patterns: flat, wide and narrow, on the host and (as integer tensors: raw bits) on the device."""
    S, H = FE.input_bits(), FE.all_bf16_bits()
    d = {"S": S, "H": H}
    for name, bits in (("S", S), ("H", H)):
        for tag, cols in (("wide", WIDE), ("narrow", NARROW)):
            d[f"{name}_{tag}"] = FE.rows_of(bits, cols)
    return d


def ok(rc):
    from egopack_amd import _lib
    assert rc == 0, _lib.last_error()


def dev(bits):
    """Bit patterns to the device, as an int16 / int32 tensor of the same shape."""
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(np.int16 if a.dtype == np.uint16 else np.int32).copy()).to(DEV)


def host(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}[a.dtype])


def filled(shape, width):
    """A device buffer of 16- or 32-bit words, every word the sentinel."""
    dt, val = (torch.int16, SENTINEL16) if width == 16 else (torch.int32, SENTINEL32)
    return torch.full(shape if isinstance(shape, tuple) else (shape,), val, dtype=dt, device=DEV)


def ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def check(site, got, want, nan_in, src, fmt="bf16"):
    """``same_bits`` with the site's line in the record (written before the comparison can raise)."""
    bad = FE.mismatches(got, want, nan_in, fmt)
    counts = FE.class_counts(bad, src, fmt)
    _REC.append(f"{site} | {bad.size} | " + " ".join(str(counts[k]) for k in FE.CLASSES) + " | " + FE.nan_summary(got, src, nan_in, fmt))
    FE.same_bits(got, want, nan_in, src, fmt, site)


def no_nan(a):
    return np.zeros(np.asarray(a).shape, dtype=bool)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the hardware convert behind f2bf: st4t / st1t of egk_cast, egk_cast_rows, egk_gather_rows, egk_split_bf16
# ---------------------------------------------------------------------------------------------------------------------------
def test_cast_to_bf16(ops, lib, data):
    """egk_cast f32 -> bf16: 16-byte aligned with n % 4 == 0 (st4t all the way), n - 1 elements (a scalar tail), and both pointers
    moved on by one element (the launch takes its scalar path, st1t)."""
    S = data["S"]
    n, s = S.size, ops._stream()
    x = dev(S)
    want, nan_in = FE.bf16_rne(S), FE.is_nan32(S)
    vec, tail, sca = filled(n, 16), filled(n, 16), filled(n, 16)
    ok(lib.egk_cast(s, ptr(x), F32, ptr(vec), BF16, n))
    ok(lib.egk_cast(s, ptr(x), F32, ptr(tail), BF16, n - 1))
    ok(lib.egk_cast(s, ptr(x, 4), F32, ptr(sca, 2), BF16, n - 1))
    torch.cuda.synchronize()
    vec, tail, sca = host(vec), host(tail), host(sca)
    check("a egk_cast f32->bf16 vector", vec, want, nan_in, S)
    check("a egk_cast f32->bf16 vector+tail", tail[:-1], want[:-1], nan_in[:-1], S[:-1])
    check("a egk_cast f32->bf16 scalar", sca[1:], want[1:], nan_in[1:], S[1:])
    assert tail[-1] == SENTINEL16 and sca[0] == SENTINEL16  # (nothing outside the n - 1 elements)
    keep = ~nan_in
    assert np.array_equal(vec[keep][1:], sca[keep][1:]) and np.array_equal(vec[:-1][keep[:-1]], tail[:-1][keep[:-1]])


def test_cast_rows_to_bf16(ops, lib, data):
    """egk_cast_rows f32 -> bf16 at 37 and 1536 columns, both leading dimensions beyond the row, zero columns behind it: +0."""
    s, outs = ops._stream(), {}
    for tag, cols in (("wide", WIDE), ("narrow", NARROW)):
        src = data[f"S_{tag}"]
        rows, ld_src, ld_dst, zero_cols = src.shape[0], cols + 3, cols + 12, cols + 8
        padded = np.full((rows, ld_src), 0x7FC00000, dtype=np.uint32)
        padded[:, :cols] = src
        x, out = dev(padded), filled((rows, ld_dst), 16)
        ok(lib.egk_cast_rows(s, ptr(x), F32, ld_src, ptr(out), BF16, ld_dst, rows, cols, zero_cols))
        torch.cuda.synchronize()
        out = host(out)
        check(f"a egk_cast_rows f32->bf16 cols {cols}", out[:, :cols], FE.bf16_rne(src), FE.is_nan32(src), src)
        assert not out[:, cols:zero_cols].any(), "the zero columns are +0"
        assert (out[:, zero_cols:] == SENTINEL16).all()
        outs[tag] = out[:, :cols].ravel()[:data["S"].size]
    keep = ~FE.is_nan32(data["S"])
    assert np.array_equal(outs["wide"][keep], outs["narrow"][keep])


def _gather(ops, lib, table_bits, t_dtype, out_dtype, extra=(-1, None, -5, None, 1 << 40)):
    """egk_gather_rows by the identity index followed by a few negative / out-of-range indices.  Returns the identity rows and
    the extra rows, as bits."""
    rows, cols = table_bits.shape
    idx = list(range(rows)) + [rows + 7 * k if e is None else e for k, e in enumerate(extra)]
    idx_d = torch.tensor(idx, dtype=torch.int64, device=DEV)
    out = filled((len(idx), cols), 16 if out_dtype == BF16 else 32)
    table = dev(table_bits)
    ok(lib.egk_gather_rows(ops._stream(), ptr(table), t_dtype, cols, rows, ptr(idx_d), ptr(out), out_dtype, len(idx), cols))
    torch.cuda.synchronize()
    out = host(out)
    return out[:rows], out[rows:]


def test_gather_rows_to_bf16(ops, lib, data):
    """egk_gather_rows f32 -> bf16 by the identity index: 1536 columns (16-byte loads, st4t) and 37 (st1t); rows of a negative or
    out-of-range index are +0."""
    outs = {}
    for tag, cols in (("wide", WIDE), ("narrow", NARROW)):
        src = data[f"S_{tag}"]
        got, extra = _gather(ops, lib, src, F32, BF16)
        check(f"a egk_gather_rows f32->bf16 cols {cols}", got, FE.bf16_rne(src), FE.is_nan32(src), src)
        assert extra.shape[0] == 5 and not extra.any(), "rows without a source are +0"
        outs[tag] = got.ravel()[:data["S"].size]
    keep = ~FE.is_nan32(data["S"])
    assert np.array_equal(outs["wide"][keep], outs["narrow"][keep])


@pytest.mark.parametrize("with_hi", [True, False], ids=["hi_and_lo", "lo_only"])
def test_split_bf16(ops, lib, data, with_hi):
    """egk_split_bf16: hi = rne(x), lo = rne(x - hi), with and without the hi output; leading dimensions that are multiples of 4 (the
    16-byte load, 8-byte stores) and that are not (element by element)."""
    s, outs = ops._stream(), {}
    for tag, cols, pad in (("wide", WIDE, 4), ("narrow", NARROW, 0), ("wide_scalar", WIDE, 1)):
        src = data["S_wide" if cols == WIDE else "S_narrow"]
        rows, ld = src.shape[0], cols + pad
        padded = np.zeros((rows, ld), dtype=np.uint32)
        padded[:, :cols] = src
        x, hi, lo = dev(padded), filled((rows, ld), 16), filled((rows, ld), 16)
        ok(lib.egk_split_bf16(s, ptr(x), ld, ptr(hi) if with_hi else None, ptr(lo), ld, rows, cols))
        torch.cuda.synchronize()
        hi, lo = host(hi), host(lo)
        w_hi, w_lo, lo_nan = FE.split_model(src)
        if with_hi:
            check(f"a egk_split_bf16 hi cols {cols} ld {ld}", hi[:, :cols], w_hi, FE.is_nan32(src), src)
        else:
            assert (hi == SENTINEL16).all()
        check(f"a egk_split_bf16 lo{'' if with_hi else ' (no hi)'} cols {cols} ld {ld}", lo[:, :cols], w_lo, lo_nan, src)
        assert (lo[:, cols:] == SENTINEL16).all() and (hi[:, cols:] == SENTINEL16).all()
        outs[tag] = (hi[:, :cols].ravel()[:data["S"].size], lo[:, :cols].ravel()[:data["S"].size])
    keep = ~FE.split_model(data["S"])[2]
    for other in ("narrow", "wide_scalar"):
        for k in (0, 1):
            assert np.array_equal(outs["wide"][k][keep], outs[other][k][keep]), (other, "hi lo"[3 * k:3 * k + 2])


# ---------------------------------------------------------------------------------------------------------------------------
# (b) bf16_rne_bits: the interpolating gather
# ---------------------------------------------------------------------------------------------------------------------------
def _lerp(ops, lib, table_bits, lo, hi, w, out_dtype):
    rows, cols = table_bits.shape
    table = dev(table_bits)
    lo_d, hi_d = (torch.tensor(np.asarray(v), dtype=torch.int64, device=DEV) for v in (lo, hi))
    w_d = torch.tensor(np.asarray(w, dtype=np.float64), dtype=torch.float64, device=DEV)
    n = lo_d.numel()
    out = filled((n, cols), 16 if out_dtype == BF16 else 32)
    ok(lib.egk_gather_lerp_rows(ops._stream(), ptr(table), F32, cols, rows, ptr(lo_d), ptr(hi_d), ptr(w_d), ptr(out), out_dtype, n, cols))
    torch.cuda.synchronize()
    return host(out)


def test_lerp_gather_rounds_on_the_bits(ops, lib, data):
    """egk_gather_lerp_rows with a bf16 output.  lo == hi is a copy (the store helper).  lo != hi with w = 0.0 and a partner row that
    does not exist (an all-zero row) evaluates 1.0 * x + 0.0 * 0.0 = x (-0 becomes +0: the sum's business, and the model's too) and
    rounds it with the bit routine."""
    outs = {}
    for tag, cols in (("wide", WIDE), ("narrow", NARROW)):
        src = data[f"S_{tag}"]
        rows = src.shape[0]
        ident, none = np.arange(rows), np.full(rows, -1)
        copy = _lerp(ops, lib, src, ident, ident, np.zeros(rows), BF16)
        check(f"a egk_gather_lerp_rows copy f32->bf16 cols {cols}", copy, FE.bf16_rne(src), FE.is_nan32(src), src)
        _, r32 = FE.lerp_model(src, np.zeros_like(src), 0.0)
        got32 = _lerp(ops, lib, src, ident, none, np.zeros(rows), F32)
        check(f"b egk_gather_lerp_rows w=0 f32->f32 cols {cols}", got32, r32, FE.is_nan32(src), src, "f32")
        got16 = _lerp(ops, lib, src, ident, none, np.zeros(rows), BF16)
        check(f"b egk_gather_lerp_rows w=0 f32->bf16 cols {cols}", got16, FE.bf16_rne(r32), FE.is_nan32(src), src)
        assert int(((src == 0x80000000) & (got16 == 0)).sum()) == int((src == 0x80000000).sum()) > 0  # (-0 + 0 = +0)
        outs[tag] = (copy.ravel()[:data["S"].size], got16.ravel()[:data["S"].size])
    keep = ~FE.is_nan32(data["S"])
    for k in (0, 1):
        assert np.array_equal(outs["wide"][k][keep], outs["narrow"][k][keep])


def test_lerp_gather_double_rounding(ops, lib):
    """The triples on which float32(r64) is a bf16 tie although r64 is not: the f32 output is that tie, the bf16 output its even
    neighbour -- not the neighbour on r64's side, which ONE f64 -> bf16 rounding gives."""
    x, y, w, r32, above = FE.lerp_double_rounding_cases()
    n = x.size
    table = np.stack([x, y], 1).reshape(2 * n, 1)
    lo, hi = 2 * np.arange(n), 2 * np.arange(n) + 1
    got32 = _lerp(ops, lib, table, lo, hi, w, F32).ravel()
    got16 = _lerp(ops, lib, table, lo, hi, w, BF16).ravel()
    check("b egk_gather_lerp_rows double-rounding cases f32 out", got32, r32, no_nan(r32), r32, "f32")
    check("b egk_gather_lerp_rows double-rounding cases bf16 out", got16, FE.bf16_rne(r32), no_nan(r32), r32)
    assert bool((got16 != FE.single_rounding(r32, above)).all())


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the IEEE-half casts, and the bf16 output of the search-prep launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_search_prep_casts(ops, lib, data):
    """egk_row_inv_norm_cast (rows of 1536 columns; the launch takes multiples of 4 only): its bf16 output against the bf16 model,
    its half output against the half model -- inf from 65520 on, half subnormals, ties.  egk_cast_f16 over the same values, with
    n % 4 == 0 and with a scalar tail, must agree with it element for element."""
    S, src = data["S"], data["S_wide"]
    rows, s = src.shape[0], ops._stream()
    x = dev(src)
    inv, hi, h16 = torch.empty(rows, device=DEV), filled((rows, WIDE), 16), filled((rows, WIDE), 16)
    ok(lib.egk_row_inv_norm_cast(s, ptr(x), ptr(inv), ptr(hi), ptr(h16), rows, WIDE))
    flat, tail = filled(S.size, 16), filled(S.size, 16)
    ok(lib.egk_cast_f16(s, ptr(x), ptr(flat), S.size))
    ok(lib.egk_cast_f16(s, ptr(x), ptr(tail), S.size - 1))
    torch.cuda.synchronize()
    hi, h16, flat, tail = host(hi), host(h16), host(flat), host(tail)
    nan_in = FE.is_nan32(src)
    check("a egk_row_inv_norm_cast bf16 out", hi, FE.bf16_rne(src), nan_in, src)
    check("d egk_row_inv_norm_cast f16 out", h16, FE.f16_rne(src), nan_in, src, "f16")
    check("d egk_cast_f16 vector", flat, FE.f16_rne(S), FE.is_nan32(S), S, "f16")
    check("d egk_cast_f16 vector+tail", tail[:-1], FE.f16_rne(S)[:-1], FE.is_nan32(S)[:-1], S[:-1], "f16")
    assert tail[-1] == SENTINEL16
    keep = ~FE.is_nan32(S)
    assert np.array_equal(h16.ravel()[:S.size][keep], flat[keep]) and np.array_equal(flat[:-1][keep[:-1]], tail[:-1][keep[:-1]])
    # every half tie with both its f32 neighbours, the inf threshold 65520 among them (S holds half ties only by chance)
    E = FE.half_edge_bits()
    e, out = dev(E), filled(E.size, 16)
    ok(lib.egk_cast_f16(s, ptr(e), ptr(out), E.size))
    torch.cuda.synchronize()
    check("d egk_cast_f16 every half tie and its neighbours", host(out), FE.f16_rne(E), no_nan(E), E, "f16")


# ---------------------------------------------------------------------------------------------------------------------------
# (c) bf16_rne_f32 / f16_rne_f32: only inside residual ratios
# ---------------------------------------------------------------------------------------------------------------------------
RATIO_ROWS, RATIO_COLS = 64, 256
# f32 evaluation of sqrt(sum d^2 / sum v^2) over 256 columns: d = v - round(v) is exact; each sum is 4 products and additions per lane
# and a 6-level wave tree (relative error <= 11 * 2^-24 each, all terms positive), one division, one square root (which halves what
# the quotient carries): <= (11 + 11 + 1) / 2 + 1 = 12.5 units of 2^-24.  The bound is 32 units.
RATIO_RTOL = 32 * 2.0 ** -24


def test_residual_ratios(ops, lib, data):
    """egk_bf16_residual_ratio and egk_residual_ratio16(f16 = 1) -- the only users of bf16_rne_f32 / f16_rne_f32, whose rounded value
    reaches no output: r = |x - round(x)| / |x| per row against an fp64 model built from the integer roundings, on rows of values
    that are no ties (a tie's two neighbours have equal residuals: the ratio cannot see the tie rule) with exponents in
    [-14, 15] (normal in half precision).  Truncation instead of rounding doubles the ratio; the bound is RATIO_RTOL."""
    S = data["S"]
    expo = (S >> 23) & 0xFF
    pick = (expo >= 127 - 14) & (expo <= 127 + 15) & ((S & 0xFFFF) != 0x8000) & ((S & 0x1FFF) != 0x1000)
    vals = S[pick][:RATIO_ROWS * RATIO_COLS].reshape(RATIO_ROWS, RATIO_COLS)
    ld = RATIO_COLS + 5
    padded = np.full((RATIO_ROWS, ld), 0x7FC00000, dtype=np.uint32)
    padded[:, :RATIO_COLS] = vals
    x, s = dev(padded), ops._stream()
    v64 = FE.f32_of(vals).astype(np.float64)
    rounded = {0: FE.f32_of(FE.widen(FE.bf16_rne(vals))).astype(np.float64), 1: FE.f32_of(vals).astype(np.float16).astype(np.float64)}
    for f16 in (0, 1):
        r, rmax = torch.empty(RATIO_ROWS, device=DEV), torch.empty(1, device=DEV)
        if f16:
            ok(lib.egk_residual_ratio16(s, ptr(x), ld, ptr(r), ptr(rmax), RATIO_ROWS, RATIO_COLS, 1))
        else:
            ok(lib.egk_bf16_residual_ratio(s, ptr(x), ld, ptr(r), ptr(rmax), RATIO_ROWS, RATIO_COLS))
        torch.cuda.synchronize()
        want = np.sqrt(((v64 - rounded[f16]) ** 2).sum(1) / (v64 ** 2).sum(1))
        got = r.cpu().numpy().astype(np.float64)
        err = float(np.abs(got / want - 1).max())
        print(f"residual ratio f16={f16}: largest relative error {err:.3e} (bound {RATIO_RTOL:.3e}), ratios {want.min():.3e} .. {want.max():.3e}")
        _REC.append(f"c egk_residual_ratio16 f16={f16} | {RATIO_ROWS} rows | largest relative error {err:.3e}, bound {RATIO_RTOL:.3e} | -")
        assert err <= RATIO_RTOL
        assert float(rmax.item()) == float(r.max().item())


# ---------------------------------------------------------------------------------------------------------------------------
# the widenings, and the copies
# ---------------------------------------------------------------------------------------------------------------------------
def test_widen_cast(ops, lib, data):
    """egk_cast bf16 -> f32 over all 65 536 patterns: aligned (the packed unpack of ld4t) and moved on by one element (bf2f)."""
    H = data["H"]
    n, s = H.size, ops._stream()
    x = dev(H)
    vec, sca = filled(n, 32), filled(n, 32)
    ok(lib.egk_cast(s, ptr(x), BF16, ptr(vec), F32, n))
    ok(lib.egk_cast(s, ptr(x, 2), BF16, ptr(sca, 4), F32, n - 1))
    torch.cuda.synchronize()
    vec, sca = host(vec), host(sca)
    want, nan_in = FE.widen(H), FE.is_nan_bf16(H)
    check("widen egk_cast bf16->f32 vector", vec, want, nan_in, H, "f32")
    check("widen egk_cast bf16->f32 scalar", sca[1:], want[1:], nan_in[1:], H[1:], "f32")
    assert sca[0] == SENTINEL32
    assert np.array_equal(vec[1:][~nan_in[1:]], sca[1:][~nan_in[1:]])


def test_widen_rows_and_gathers(ops, lib, data):
    """egk_cast_rows and egk_gather_rows from a bf16 table over all 65 536 patterns: to f32 (the packed unpack at 1536 columns, bf2f
    at 37) and to bf16 (at 1536 columns a 16-byte copy: every pattern exact, NaN payloads included; at 37 through the store
    helper: a NaN stays a NaN)."""
    s = ops._stream()
    outs = {}
    for tag, cols in (("wide", WIDE), ("narrow", NARROW)):
        src = data[f"H_{tag}"]
        rows, nan_in = src.shape[0], FE.is_nan_bf16(src)
        x = dev(src)
        for out_dtype, fmt, want in ((F32, "f32", FE.widen(src)), (BF16, "bf16", src)):
            out = filled((rows, cols + 4), 32 if out_dtype == F32 else 16)
            ok(lib.egk_cast_rows(s, ptr(x), BF16, cols, ptr(out), out_dtype, cols + 4, rows, cols, 0))
            torch.cuda.synchronize()
            out = host(out)
            check(f"widen egk_cast_rows bf16->{fmt} cols {cols}", out[:, :cols], want, nan_in, src, fmt)
            assert (out[:, cols:] == (SENTINEL32 if out_dtype == F32 else SENTINEL16)).all()
            got, extra = _gather(ops, lib, src, BF16, out_dtype)
            exact = out_dtype == BF16 and cols == WIDE
            check(f"widen egk_gather_rows bf16->{fmt} cols {cols}", got, want, no_nan(src) if exact else nan_in, src, fmt)
            assert not extra.any()
            outs[tag, fmt] = got.ravel()[:65536]
    keep = ~FE.is_nan_bf16(data["H"])
    for fmt in ("f32", "bf16"):
        assert np.array_equal(outs["wide", fmt][keep], outs["narrow", fmt][keep])


def test_gather_rows_f32_copies_all_bits(ops, lib, data):
    for tag, cols in (("wide", WIDE), ("narrow", NARROW)):
        src = data[f"S_{tag}"]
        got, extra = _gather(ops, lib, src, F32, F32)
        check(f"copy egk_gather_rows f32->f32 cols {cols}", got, src, no_nan(src), src, "f32")
        assert not extra.any()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the contractions: f32_to_bf16 in every store loop, pack8 in the operand loaders, bf16_to_f32 on a residual
# ---------------------------------------------------------------------------------------------------------------------------
K = N = 64


def _finite_subset(S):
    """The finite members of S that are +0 or of magnitude >= 2^-126 (what the matrix cores do with subnormals is not the
    conversion's business, nor is -0 + 0)."""
    mag = S & 0x7FFFFFFF
    return S[(S == 0) | ((mag >= 0x00800000) & (mag < 0x7F800000))]


def _as_matrix(bits, cols=K):
    return FE.rows_of(bits, cols)


def _f32_tensor(bits):
    return dev(bits).view(torch.float32)


def _bf16_tensor(bits):
    return dev(bits).view(torch.bfloat16)


class _forced:
    """egk_gemm_set_pipeline(tile) -- and the store loop of the rows epilogue (890 / 891) -- restored on exit."""

    def __init__(self, lib, tile, rows_fast=1):
        self.lib, self.tile, self.rows_fast = lib, tile, rows_fast

    def __enter__(self):
        self.prev = self.lib.egk_gemm_set_pipeline(self.tile)
        self.lib.egk_gemm_set_pipeline(890 + self.rows_fast)

    def __exit__(self, *exc):
        self.lib.egk_gemm_set_pipeline(891)
        self.lib.egk_gemm_set_pipeline(self.prev)


class _counted:
    """The library's launch counters around a block: ``.names`` = {kernel name: launches} (egk_prof_reset / egk_prof_get)."""

    def __init__(self, lib):
        self.lib, self.names = lib, {}

    def __enter__(self):
        self.lib.egk_prof_enable(1)
        self.lib.egk_prof_reset()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        name, n, ms, fl, by = C.create_string_buffer(64), C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        for i in range(self.lib.egk_prof_count()):
            assert self.lib.egk_prof_get(i, name, 64, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)) == 0
            if n.value:
                self.names[name.value.decode()] = n.value
        self.lib.egk_prof_enable(0)
        self.lib.egk_prof_reset()


def _eye(dtype):
    return torch.eye(N, K, device=DEV, dtype=dtype)


@pytest.mark.parametrize("name,tile,rows_fast", [("generic", 0, 1), ("tile128", 3, 1), ("tile128_ladder", 3, 0), ("tile96", 8, 1)])
def test_gemm_store_to_bf16(ops, lib, data, name, tile, rows_fast):
    """C = A . I^T in exact f32 with a bf16 C: the accumulator is A's element, the store its rounding.  The generic kernel and the
    128- and 96-row tiles of the exact-f32 family, the rows epilogue by both of its store loops; ldc = 64 (packed 8-byte / 16-byte
    stores) and ldc = 67 (element stores); the last row tile is ragged."""
    A_bits = _as_matrix(_finite_subset(data["S"]))
    M = A_bits.shape[0]
    assert M % 128 and M % 96
    A, outs = _f32_tensor(A_bits), {}
    with _forced(lib, tile, rows_fast):
        for ldc in (N, N + 3):
            out = filled((M, ldc), 16).view(torch.bfloat16)
            ops.gemm(M, N, A, K, _eye(torch.float32), K, K, out, ldc, compute=ops.F32, allow_splitk=False)
            torch.cuda.synchronize()
            got = host(out.view(torch.int16))
            check(f"a gemm f32 compute, bf16 C, {name}, ldc {ldc}", got[:, :N], FE.bf16_rne(A_bits), no_nan(A_bits), A_bits)
            assert (got[:, N:] == SENTINEL16).all()
            outs[ldc] = got[:, :N]
    assert np.array_equal(outs[N], outs[N + 3])


@pytest.mark.parametrize("name,tile", [("generic", 0), ("policy", 1), ("tile128", 3), ("tile192", 16)])
def test_gemm_store_to_bf16_from_bf16_operands(ops, lib, data, name, tile):
    """The store loops of the bf16-operand kernels (the 192-row tile among them): C = hi(x) . I^T + lo(x) . I^T as two K sources, on
    the members x of the finite subset with at most 16 significant bits -- every tie is one -- whose lo is zero or normal: both
    products and their sum are exact, so the accumulator is x and the store its rounding, hi(x)."""
    sub = _finite_subset(data["S"])
    sub = sub[(sub & 0xFF) == 0]
    hi, lo, _ = FE.split_model(sub)
    lo_mag = lo & 0x7FFF
    sel = ((lo_mag == 0) | (lo_mag >= 0x0080)) & ((hi & 0x7FFF) < 0x7F80)  # (and hi finite: the rest of the subset rounds to inf)
    sub, hi, lo = sub[sel], hi[sel], lo[sel]
    exact = FE.f32_of(FE.widen(hi)).astype(np.float64) + FE.f32_of(FE.widen(lo)).astype(np.float64)
    sel = exact == FE.f32_of(sub).astype(np.float64)  # (drops the few x whose x - hi is an f32 subnormal that rounds to lo = 0)
    sub, hi, lo = sub[sel], hi[sel], lo[sel]
    assert sub.size > 130000 and int(((sub & 0xFFFF) == 0x8000).sum()) > 60000
    X, HI, LO = _as_matrix(sub), _as_matrix(hi), _as_matrix(lo)
    M = X.shape[0]
    assert M % 192 and M % 128
    A1, A2, I = _bf16_tensor(HI), _bf16_tensor(LO), _eye(torch.bfloat16)
    outs = {}
    for ldc in (N, N + 3):  # (the rows epilogue's packed stores / element stores)
        with _forced(lib, tile), _counted(lib) as ran:
            out = filled((M, ldc), 16).view(torch.bfloat16)
            ops.gemm(M, N, A1, K, I, K, K, out, ldc, A2=A2, lda2=K, B2=I, ldb2=K, K2=K, compute=ops.BF16, allow_splitk=False)
            torch.cuda.synchronize()
        print(f"{name}, ldc {ldc}: {ran.names}")
        if name != "policy":  # (the forced kernel is the one that ran)
            assert ran.names == {{"generic": "gemm_bf16_generic", "tile128": "gemm_bf16_nn", "tile192": "gemm_bf16_nn_r192"}[name]: 1}
        got = host(out.view(torch.int16))
        check(f"a gemm bf16 operands hi + lo, bf16 C, {name}, ldc {ldc}", got[:, :N], FE.bf16_rne(X), no_nan(X), X)
        assert (got[:, N:] == SENTINEL16).all()
        outs[ldc] = got[:, :N]
    assert np.array_equal(outs[N], outs[N + 3])


def test_gemm_operand_pack(ops, lib, data):
    """The 8-wide pack of f32 operands of a bf16-compute contraction (the generic mixed-operand kernel; no pipelined family takes f32
    operands in that mode): C = A . I^T with an f32 C must be widen(rne(A)).  Row-major A through 16-byte loads (lda = 64) and
    element loads (lda = 67), and A stored K-major (the transposed loader).  The members that round to inf sit one per row, since
    inf * 0 in the other columns is not the conversion's business; only their own column is compared."""
    sub = _finite_subset(data["S"])
    to_inf = (FE.bf16_rne(sub) & 0x7FFF) == 0x7F80
    A_bits = _as_matrix(sub[~to_inf])
    M = A_bits.shape[0]
    want = FE.widen(FE.bf16_rne(A_bits))
    I = _eye(torch.float32)
    outs = {}
    for layout, lda in (("rows", K), ("rows", K + 3), ("kmajor", M)):
        if layout == "rows":
            padded = np.zeros((M, lda), dtype=np.uint32)
            padded[:, :K] = A_bits
            A = _f32_tensor(padded)
        else:
            A = _f32_tensor(np.ascontiguousarray(A_bits.T))
        out = filled((M, N), 32).view(torch.float32)
        with _counted(lib) as ran:
            ops.gemm(M, N, A, lda, I, K, K, out, N, transA=layout == "kmajor", compute=ops.BF16, allow_splitk=False)
            torch.cuda.synchronize()
        assert ran.names == {"gemm_bf16_generic": 1}
        outs[layout, lda] = host(out.view(torch.int32))
        check(f"a gemm operand pack, {layout}, lda {lda}", outs[layout, lda], want, no_nan(want), A_bits, "bf16")
    assert np.array_equal(outs["rows", K], outs["rows", K + 3]) and np.array_equal(outs["rows", K], outs["kmajor", M])
    big = sub[to_inf]
    assert big.size == 30
    B_bits = np.zeros((big.size, K), dtype=np.uint32)
    B_bits[np.arange(big.size), np.arange(big.size) % K] = big
    out = filled((big.size, N), 32).view(torch.float32)
    ops.gemm(big.size, N, _f32_tensor(B_bits), K, I, K, K, out, N, compute=ops.BF16, allow_splitk=False)
    torch.cuda.synchronize()
    got = host(out.view(torch.int32))[np.arange(big.size), np.arange(big.size) % K]
    check("a gemm operand pack, finite -> inf", got, FE.widen(FE.bf16_rne(big)), no_nan(big), big, "bf16")


@pytest.mark.parametrize("name,tile", [("generic", 0), ("policy", 1)])
def test_gemm_residual_widen(ops, lib, data, name, tile):
    """A bf16 residual on a zero product, f32 C: 0 + widen(r), over all 65 536 patterns (-0 comes out as +0: the sum's business);
    ldr = 64 (the packed unpack) and ldr = 67 (bf16_to_f32)."""
    H = data["H"].reshape(-1, N)
    M = H.shape[0]
    want = FE.widen(H)
    want[H == 0x8000] = 0
    A, I = torch.zeros(M, K, device=DEV), _eye(torch.float32)
    with _forced(lib, tile):
        for ldr in (N, N + 3):
            padded = np.zeros((M, ldr), dtype=np.uint16)
            padded[:, :N] = H
            out = filled((M, N), 32).view(torch.float32)
            ops.gemm(M, N, A, K, I, K, K, out, N, residual=_bf16_tensor(padded), ldr=ldr, compute=ops.F32, allow_splitk=False)
            torch.cuda.synchronize()
            check(f"widen gemm bf16 residual, {name}, ldr {ldr}", host(out.view(torch.int32)), want, FE.is_nan_bf16(H), H, "f32")
