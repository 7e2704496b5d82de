"""The rounding contract of every f32 / bf16 / f16 conversion site, as host models on bit patterns (numpy + torch, no GPU).

The contract is IEEE round to nearest, ties to even -- what torch's CPU casts do: tests/test_format_edges_cpu.py holds the integer
models below against those casts over all of ``input_bits()``, and tests/test_gpu_format_edges.py holds every conversion site of
egopack_amd/csrc against the models.  The code under test is never its own reference.

  * ``input_bits()``       the input set S (uint32 patterns of f32 values): every bf16 tie, both neighbours of every tie, every
                           exponent, +-0, +-inf, every subnormal high half, and 2^20 seeded random patterns,
  * ``bf16_rne`` ...       the models,
  * ``same_bits``          the one comparison: a NaN input needs a NaN output, everything else all bits (zero's sign included),
  * ``mutants``            wrong roundings the comparison must catch (truncation, half-up, flushed subnormals, saturation, ...),
  * ``lerp_double_rounding_cases``   inputs of the interpolating gather on which ONE f64 -> bf16 rounding gives the other neighbour,
  * ``SITES`` / ``scan_sites``       the ledger: every conversion routine of the library and the GPU test that reaches it.
"""
import re
from pathlib import Path

import numpy as np

LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
N_GRID, N_RANDOM = 65536 * len(LOW_HALVES), 1 << 20
WIDE_COLS, NARROW_COLS = 1536, 37  # rows of whole 16-byte groups (the vector paths) / of element accesses (the scalar paths)

_U32, _U16 = np.uint32, np.uint16


# ---------------------------------------------------------------------------------------------------------------------------
# the input set
# ---------------------------------------------------------------------------------------------------------------------------
def input_bits():
    """S: 393 216 grid patterns (high half x LOW_HALVES) followed by 2^20 patterns of PCG64(1); uint32, 1 441 792 values."""
    grid = ((np.arange(65536, dtype=_U32) << 16)[:, None] | np.array(LOW_HALVES, dtype=_U32)[None, :]).ravel()
    rnd = np.random.Generator(np.random.PCG64(1)).integers(0, 1 << 32, size=N_RANDOM, dtype=np.uint64).astype(_U32)
    return np.concatenate([grid, rnd])


def half_edge_bits():
    """S holds the half-precision ties only by chance (its grid is the bf16 one).  For the f16 casts, in addition: the midpoint of
    every pair of adjacent non-negative halves -- the half subnormals, and 65520 = the midpoint of 65504 and 2^16, the inf
    threshold, among them -- with both its f32 neighbours, in both signs; 190 464 f32 patterns."""
    h = np.arange(0x7C00, dtype=_U16)  # the finite halves
    lo = h.view(np.float16).astype(np.float64)
    hi = np.append(lo[1:], 65536.0)
    mid = ((lo + hi) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)
    m = bits_of(mid)
    pos = np.stack([m - _U32(1), m, m + _U32(1)], 1).ravel()
    return np.concatenate([pos, pos | _U32(0x80000000)])


def all_bf16_bits():
    return np.arange(65536, dtype=np.uint32).astype(_U16)


def rows_of(bits, cols):
    """``bits`` laid out as whole rows of ``cols`` columns; the last row is filled up from the start of ``bits``."""
    rows = -(-bits.size // cols)
    return np.resize(bits, rows * cols).reshape(rows, cols)


def is_nan32(u):
    return (u & _U32(0x7FFFFFFF)) > _U32(0x7F800000)


def is_nan_bf16(h):
    return (h & _U16(0x7FFF)) > _U16(0x7F80)


def is_nan_f16(h):
    return (h & _U16(0x7FFF)) > _U16(0x7C00)


def f32_of(u):
    return np.ascontiguousarray(u, dtype=_U32).view(np.float32)


def bits_of(f):
    return np.ascontiguousarray(f, dtype=np.float32).view(_U32)


# ---------------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------------
def bf16_rne(u):
    """f32 bits -> bf16 bits, round to nearest even, on uint64 (no wrap).  Defined for non-NaN inputs; a NaN input gives some
    pattern that ``same_bits`` never looks at."""
    w = np.asarray(u).astype(np.uint64)
    return ((w + np.uint64(0x7FFF) + ((w >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(_U16)


def f16_rne(u):
    """f32 bits -> IEEE half bits: numpy's cast (round to nearest even, inf beyond 65504, gradual underflow)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return f32_of(u).astype(np.float16).view(_U16)


def widen(h):
    """bf16 bits -> f32 bits."""
    return np.asarray(h).astype(_U32) << _U32(16)


def split_model(u):
    """egk_split_bf16: hi = rne(x), lo = rne(float32(x) - widen(hi)) in numpy float32.  Returns hi, lo and where lo's input is NaN."""
    hi = bf16_rne(u)
    with np.errstate(invalid="ignore", over="ignore"):
        d = f32_of(u) - f32_of(widen(hi))
    return hi, bf16_rne(bits_of(d)), np.isnan(d)


def lerp_model(x_bits, y_bits, w):
    """The interpolating gather's documented formula: float64 (1 - w) * x + w * y with each product and the sum rounded separately,
    then float32.  Returns the f64 value and the f32 bits."""
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r64 = (1.0 - w) * f32_of(x_bits).astype(np.float64) + w * f32_of(y_bits).astype(np.float64)
        return r64, bits_of(r64.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------
CLASSES = ("nan", "zero", "subnormal", "overflow", "tie", "other")
_NAN_OF = {"bf16": is_nan_bf16, "f16": is_nan_f16, "f32": is_nan32}


def classify(src, fmt):
    """Class index (into CLASSES) of every input, for a conversion to ``fmt``.  ``src``: uint32 f32 bits, or uint16 bf16 bits (a
    widening: no ties, no overflow)."""
    src = np.asarray(src)
    sub_top = _U32(0x00800000)
    if src.dtype == _U16:
        mag = (src.astype(_U32) << _U32(16)) & _U32(0x7FFFFFFF)
        low_tie = np.zeros(src.shape, dtype=bool)
        over = np.zeros(src.shape, dtype=bool)
    else:
        mag = src & _U32(0x7FFFFFFF)
        if fmt == "f16":  # (ties of the normal half range; below 2^-14 the result is a half subnormal or zero)
            low_tie = ((src & _U32(0x1FFF)) == _U32(0x1000)) & (mag >= _U32(0x38800000))
            over = (mag >= _U32(0x477FF000)) & (mag < _U32(0x7F800000))
            sub_top = _U32(0x38800000)
        elif fmt == "bf16":
            low_tie = (src & _U32(0xFFFF)) == _U32(0x8000)
            over = (mag >= _U32(0x7F7F8000)) & (mag < _U32(0x7F800000))
        else:  # (f32 -> f32: a copy)
            low_tie = np.zeros(src.shape, dtype=bool)
            over = np.zeros(src.shape, dtype=bool)
    cls = np.full(src.shape, CLASSES.index("other"), dtype=np.uint8)
    cls[low_tie] = CLASSES.index("tie")
    cls[over] = CLASSES.index("overflow")
    cls[(mag > 0) & (mag < sub_top)] = CLASSES.index("subnormal")
    cls[mag == 0] = CLASSES.index("zero")
    cls[mag > _U32(0x7F800000)] = CLASSES.index("nan")
    return cls


def mismatches(got, want, nan_in, fmt):
    """Boolean mask of the elements that break the contract: a NaN input whose output is no NaN, any other input whose output
    differs from ``want`` in any bit."""
    got, want, nan_in = np.asarray(got), np.asarray(want), np.asarray(nan_in, dtype=bool)
    assert got.dtype == want.dtype and got.shape == want.shape == nan_in.shape, (got.dtype, want.dtype, got.shape, want.shape, nan_in.shape)
    return np.where(nan_in, ~_NAN_OF[fmt](got), got != want)


def class_counts(bad, src, fmt):
    cls = classify(src, fmt)
    return {name: int((bad & (cls == i)).sum()) for i, name in enumerate(CLASSES)}


def same_bits(got, want, nan_in, src=None, fmt="bf16", what=""):
    """The comparison of this suite; no tolerance.  ``src``: the input patterns (for the report and its classes).  Returns the
    per-class mismatch counts (all zero) or raises with the count, the classes and the first ten (input, got, want) in hex."""
    bad = mismatches(got, want, nan_in, fmt)
    src = np.asarray(want if src is None else src)
    counts = class_counts(bad, src, fmt)
    if bad.any():
        idx = np.flatnonzero(bad.ravel())[:10]
        cls = classify(src, fmt).ravel()
        w_in, w_out = (8 if src.dtype == _U32 else 4), (8 if np.asarray(got).dtype == _U32 else 4)
        rows = [f"  [{i}] in {int(src.ravel()[i]):0{w_in}x} got {int(np.asarray(got).ravel()[i]):0{w_out}x} want "
                f"{int(np.asarray(want).ravel()[i]):0{w_out}x} ({CLASSES[cls[i]]})" for i in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ from the {fmt} model, by class "
                             f"{ {k: v for k, v in counts.items() if v} }\n" + "\n".join(rows))
    return counts


def nan_summary(got, src, nan_in, fmt, limit=3):
    """What a site stored for NaN inputs, in words (informational; nothing asserts it): how many distinct patterns, whether all are
    quiet, whether the sign is the input's, whether the pattern is the input's leading bits with the quiet bit set, and the most
    frequent patterns."""
    got, src, nan_in = np.asarray(got), np.asarray(src), np.asarray(nan_in, dtype=bool)
    if not nan_in.any() or src.shape != got.shape:
        return "-"
    g, s = got[nan_in].astype(np.uint64), src[nan_in].astype(np.uint64)
    gbits, sbits = 8 * got.dtype.itemsize, 8 * src.dtype.itemsize
    quiet = {"bf16": 0x0040, "f16": 0x0200, "f32": 0x00400000}[fmt]
    words = [f"{np.unique(g).size} distinct",
             "all quiet" if bool((g & np.uint64(quiet) != 0).all()) else f"{int((g & np.uint64(quiet) == 0).sum())} signalling",
             "sign kept" if bool(((g >> np.uint64(gbits - 1)) == (s >> np.uint64(sbits - 1))).all()) else "sign not kept"]
    if fmt != "f16":
        lead = (s >> np.uint64(sbits - gbits)) if sbits >= gbits else (s << np.uint64(gbits - sbits))
        if bool((g == lead).all()):
            words.append("the input's leading bits unchanged")
        elif bool((g == (lead | np.uint64(quiet))).all()):
            words.append("the input's leading bits with the quiet bit set")
        else:
            words.append("not the input's leading bits")
    vals, cnt = np.unique(g, return_counts=True)
    order = np.argsort(-cnt, kind="stable")[:limit]
    return ", ".join(words) + "; e.g. " + " ".join(f"{int(vals[i]):0{gbits // 4}x}" for i in order)


# ---------------------------------------------------------------------------------------------------------------------------
# wrong roundings the comparison must catch
# ---------------------------------------------------------------------------------------------------------------------------
def mutants(u):
    """name -> (bf16 bits of a wrong rounding of the f32 bits ``u``, the class it must be caught in)."""
    u = np.asarray(u, dtype=_U32)
    good = bf16_rne(u)
    sign = (u >> _U32(16)).astype(_U16) & _U16(0x8000)
    mag = u & _U32(0x7FFFFFFF)
    out = {}
    out["truncation"] = ((u >> _U32(16)).astype(_U16), "other")
    out["round_half_up"] = (((u.astype(np.uint64) + np.uint64(0x8000)) >> np.uint64(16)).astype(_U16), "tie")
    out["flush_subnormals"] = (np.where((mag > 0) & (mag < _U32(0x00800000)), sign, good), "subnormal")
    finite_to_inf = (mag < _U32(0x7F800000)) & ((good & _U16(0x7FFF)) == _U16(0x7F80))
    out["saturate_to_max"] = (np.where(finite_to_inf, sign | _U16(0x7F7F), good), "overflow")
    out["positive_zero_only"] = (np.where(mag == 0, _U16(0), good), "zero")
    out["nan_to_inf"] = (np.where(is_nan32(u), sign | _U16(0x7F80), good), "nan")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# double rounding in the interpolating gather
# ---------------------------------------------------------------------------------------------------------------------------
LERP_MIN_EACH = 256


def lerp_double_rounding_cases(want_each=320, seed=5):
    """Triples (x, y, w), x and y f32 values, on which float32(r64) is a bf16 tie although r64 itself is not: the documented two
    roundings send the tie to the even neighbour, ONE f64 -> bf16 rounding to the side r64 lies on -- and only triples on which
    these two differ are kept.  Found by search: for random x < y of one sign and a tie t between them, the weights within a few
    ulps of (t - x) / (y - x) are evaluated with ``lerp_model`` and those that land on t in f32, off t in f64, kept.  Returns
    x_bits, y_bits, w, r32_bits, above (|r64| > |t|); asserts at least LERP_MIN_EACH of either side."""
    rng = np.random.Generator(np.random.PCG64(seed))
    keep = {True: [], False: []}
    for _ in range(64):
        n = 1 << 14
        sign = rng.integers(0, 2, n).astype(_U32) << _U32(31)
        # t: a tie with an exponent well inside the normal range; x below it, y above it, within a factor of two in magnitude
        t_bits = (rng.integers(0x3000, 0x5000, n).astype(_U32) << _U32(16)) | _U32(0x8000)
        t = f32_of(t_bits).astype(np.float64)
        x = (t * rng.uniform(0.55, 0.95, n)).astype(np.float32)
        y = (t * rng.uniform(1.05, 1.9, n)).astype(np.float32)
        x_bits, y_bits, t_bits = bits_of(x) | sign, bits_of(y) | sign, t_bits | sign
        x64, y64, t64 = f32_of(x_bits).astype(np.float64), f32_of(y_bits).astype(np.float64), f32_of(t_bits).astype(np.float64)
        w0 = (t64 - x64) / (y64 - x64)
        for k in range(-6, 7):
            w = w0
            for _ in range(abs(k)):
                w = np.nextafter(w, 2.0 if k > 0 else -1.0)
            r64, r32 = lerp_model(x_bits, y_bits, w)
            hit = (r32 == t_bits) & (r64 != t64) & (w > 0.0) & (w < 1.0)
            above = np.abs(r64) > np.abs(t64)
            lower = (t_bits >> _U32(16)).astype(_U16)  # (in magnitude; the bits grow with the magnitude for either sign)
            single = np.where(above, lower + _U16(1), lower)
            hit &= single != bf16_rne(r32)
            for side in (True, False):
                sel = np.flatnonzero(hit & (above == side))
                keep[side].append((x_bits[sel], y_bits[sel], w[sel], r32[sel]))
        if all(sum(c[0].size for c in keep[s]) >= want_each for s in (True, False)):
            break
    out = []
    for side in (True, False):
        cols = [np.concatenate([c[i] for c in keep[side]])[:want_each] for i in range(4)]
        assert cols[0].size >= LERP_MIN_EACH, f"only {cols[0].size} double-rounding cases with r64 {'above' if side else 'below'} the tie"
        out.append(cols + [np.full(cols[0].size, side)])
    x_bits, y_bits, w, r32, above = (np.concatenate([out[0][i], out[1][i]]) for i in range(5))
    # what makes the cases sharp, re-derived from the returned arrays
    r64, r32_again = lerp_model(x_bits, y_bits, w)
    t64 = f32_of(r32).astype(np.float64)
    assert np.array_equal(r32, r32_again) and bool(((r32 & _U32(0xFFFF)) == _U32(0x8000)).all()) and bool((r64 != t64).all())
    assert np.array_equal(above, np.abs(r64) > np.abs(t64))
    assert int(above.sum()) >= LERP_MIN_EACH and int((~above).sum()) >= LERP_MIN_EACH
    return x_bits, y_bits, w, r32, above


def single_rounding(r32_bits, above):
    """What ONE f64 -> bf16 rounding gives on the cases above: the neighbour on r64's side of the tie."""
    lower = (np.asarray(r32_bits) >> _U32(16)).astype(_U16)
    return np.where(above, lower + _U16(1), lower)


# ---------------------------------------------------------------------------------------------------------------------------
# the ledger of conversion sites
# ---------------------------------------------------------------------------------------------------------------------------
CSRC = Path(__file__).resolve().parents[1] / "egopack_amd" / "csrc"
GPU_TESTS = "tests/test_gpu_format_edges.py"

# Every occurrence of these in code (comments stripped) is a conversion written out in place: a defining occurrence.
_INLINE_IDIOMS = ("(__bf16)", "(_Float16)", "0x7fffu", "(bf16_t)(")
# The helpers: only the line that DEFINES one counts (their uses convert through the definition).
_HELPER_IDIOMS = ("f2bf(", "bf2f(", "f32_to_bf16(", "bf16_to_f32(")
_HELPER_DEF = re.compile(r"\b(?:bf16_t|float)\s+(f2bf|bf2f|f32_to_bf16|bf16_to_f32)\s*\(")
_NAME = re.compile(r"([A-Za-z_]\w*)\s*\(")
_NOT_A_NAME = {"__launch_bounds__", "__attribute__", "if", "for", "while", "switch", "return", "sizeof"}


def _enclosing_function(lines, i):
    """The name in the nearest line at or above ``i`` that starts a definition at column 0."""
    for j in range(i, -1, -1):
        ln = lines[j]
        if not ln or ln[0] in " \t/#{}" or ln.startswith(("template", "typedef", "using", "namespace", "extern \"C\" {")) or "(" not in ln:
            continue
        for name in _NAME.findall(ln):
            if name not in _NOT_A_NAME:
                return name
    return "<file scope>"


def scan_sites(csrc=CSRC):
    """{(file, function, idiom)} of every defining occurrence of a conversion idiom in csrc/*.hip and csrc/*.h."""
    found = set()
    for path in sorted([*csrc.glob("*.hip"), *csrc.glob("*.h")]):
        lines = [ln.split("//", 1)[0] for ln in path.read_text().splitlines()]
        for i, ln in enumerate(lines):
            for idiom in _INLINE_IDIOMS:
                if idiom in ln:
                    found.add((path.name, _enclosing_function(lines, i), idiom))
            m = _HELPER_DEF.search(ln)
            if m:
                found.add((path.name, m.group(1), m.group(1) + "("))
    return found


def _t(name):
    return {"test": f"{GPU_TESTS}::{name}"}


# (file, function, idiom) -> {"test": the GPU test that reaches the site} or {"exempt": why no test of the rounding itself can}.
# A conversion routine that is not listed here turns tests/test_format_edges_cpu.py::test_ledger_is_complete red.
SITES = {
    # (a) the hardware convert behind f2bf: st1t / st4t and every kernel that packs its own store
    ("common.h", "f2bf", "(__bf16)"): _t("test_cast_to_bf16"),
    ("common.h", "f2bf", "f2bf("): _t("test_cast_to_bf16"),
    ("common.h", "bf2f", "bf2f("): _t("test_widen_cast"),
    # (a) the contractions: the store of a bf16 result, the 8-wide pack of f32 operands, the widening of a bf16 residual
    ("gemm.hip", "f32_to_bf16", "(__bf16)"): _t("test_gemm_store_to_bf16"),
    ("gemm.hip", "f32_to_bf16", "f32_to_bf16("): _t("test_gemm_store_to_bf16"),
    ("gemm.hip", "pack8", "(__bf16)"): _t("test_gemm_operand_pack"),
    ("gemm.hip", "bf16_to_f32", "bf16_to_f32("): _t("test_gemm_residual_widen"),
    # (b) the bit routine of the interpolating gather
    ("graph_ops.hip", "bf16_rne_bits", "0x7fffu"): _t("test_lerp_gather_rounds_on_the_bits"),
    ("graph_ops.hip", "bf16_rne_bits", "(bf16_t)("): _t("test_lerp_gather_rounds_on_the_bits"),
    # (c) only the residual ratios of the window search use it, and no output carries the rounded value: the two neighbours of a
    # tie have EQUAL residuals, so the ratio cannot see the tie rule; every other property moves the ratio, which is compared
    ("graph_ops.hip", "bf16_rne_f32", "0x7fffu"): {
        "exempt": "a residual ratio cannot see the tie rule (equal residuals on either side); test_residual_ratios pins the rest",
        "test": f"{GPU_TESTS}::test_residual_ratios"},
    ("graph_ops.hip", "f16_rne_f32", "(_Float16)"): {
        "exempt": "a residual ratio cannot see the tie rule (equal residuals on either side); test_residual_ratios pins the rest",
        "test": f"{GPU_TESTS}::test_residual_ratios"},
    # (d) the IEEE-half casts
    ("graph_ops.hip", "row_inv_norm_cast_kernel", "(_Float16)"): _t("test_search_prep_casts"),
    ("graph_ops.hip", "cast_f16_kernel", "(_Float16)"): _t("test_search_prep_casts"),
    # (e) its nearest mode is f2bf (above); the stochastic branch adds 16 random bits under the dropped ones
    ("optim_rules.hip", "round_state", "(bf16_t)("): {
        "exempt": "stochastic rounding: tests/test_gpu_optim_state.py holds it against its own Philox host model"},
}


def ledger_problems(sites=None, scanned=None):
    """What is wrong with the ledger, as a list of lines (empty: complete)."""
    sites = SITES if sites is None else sites
    scanned = scan_sites() if scanned is None else scanned
    out = [f"conversion site {k} is not in SITES (tests/format_edges_common.py)" for k in sorted(scanned - set(sites))]
    out += [f"SITES lists {k}, which the sources no longer hold" for k in sorted(set(sites) - scanned)]
    text = (Path(__file__).resolve().parent / "test_gpu_format_edges.py").read_text()
    for k, v in sorted(sites.items()):
        if "test" not in v and not v.get("exempt", "").strip():
            out.append(f"{k}: neither a test nor a reason")
        if "test" in v:
            mod, _, fn = v["test"].partition("::")
            if mod != GPU_TESTS or not re.search(rf"^def {re.escape(fn)}\(", text, re.M):
                out.append(f"{k}: {v['test']} does not exist")
    return out
