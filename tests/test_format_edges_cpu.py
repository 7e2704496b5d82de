"""The host side of the format-edge suite (tests/format_edges_common.py): the integer models against torch's CPU casts over the
whole input set, the comparison helper against wrong roundings, the double-rounding cases of the interpolating gather, and the
ledger of conversion sites.  No GPU."""
import numpy as np
import pytest
import torch

from tests import format_edges_common as FE


@pytest.fixture(scope="module")
def S():
    return FE.input_bits()


def _torch_bits16(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_input_set(S):
    """Every high half with each of the six low halves, then the seeded random patterns; what the set holds of each edge class."""
    assert S.dtype == np.uint32 and S.size == 1_441_792 == FE.N_GRID + FE.N_RANDOM
    grid = S[:FE.N_GRID].reshape(65536, len(FE.LOW_HALVES))
    assert np.array_equal(grid >> 16, np.broadcast_to(np.arange(65536, dtype=np.uint32)[:, None], grid.shape))
    assert np.array_equal(grid & 0xFFFF, np.broadcast_to(np.array(FE.LOW_HALVES, dtype=np.uint32)[None, :], grid.shape))
    assert np.array_equal(S, FE.input_bits())  # (seeded)
    cls = FE.classify(S, "bf16")
    count = {name: int((cls == i).sum()) for i, name in enumerate(FE.CLASSES)}
    print("input set by class:", count)
    assert (count["nan"], count["subnormal"], count["overflow"], count["zero"]) == (5548, 5664, 30, 2)
    # the grid alone: 65 536 ties less the 256 NaN ones, the 256 subnormal ones and the two that overflow; 256 x 6 - 2 subnormals
    # and as many NaNs; 7f7f8000, 7f7f8001 and 7f7fffff of either sign round to inf; +-0
    gcls = FE.classify(grid.ravel(), "bf16")
    gcount = {name: int((gcls == i).sum()) for i, name in enumerate(FE.CLASSES)}
    assert gcount["tie"] == 65536 - 512 - 2 and gcount["subnormal"] == 1534 and gcount["nan"] == 1534
    assert gcount["overflow"] == 6 and gcount["zero"] == 2
    finite_to_inf = (~FE.is_nan32(S)) & ((S & 0x7FFFFFFF) < 0x7F800000) & ((FE.bf16_rne(S) & 0x7FFF) == 0x7F80)
    assert int(finite_to_inf.sum()) == count["overflow"]


def test_bf16_model_against_torch_cpu(S):
    t = torch.from_numpy(FE.f32_of(S).copy())
    got = _torch_bits16(t.to(torch.bfloat16))
    counts = FE.same_bits(got, FE.bf16_rne(S), FE.is_nan32(S), S, "bf16", "torch's CPU bfloat16 cast against the integer model")
    assert sum(counts.values()) == 0
    assert bool(FE.is_nan_bf16(got[FE.is_nan32(S)]).all())  # (torch keeps a NaN a NaN as well)


def test_f16_model_against_torch_cpu(S):
    t = torch.from_numpy(FE.f32_of(S).copy())
    got = _torch_bits16(t.to(torch.float16))
    counts = FE.same_bits(got, FE.f16_rne(S), FE.is_nan32(S), S, "f16", "torch's CPU float16 cast against numpy's")
    assert sum(counts.values()) == 0
    # the edges the model must show: inf from 65520 on, the largest half below it, gradual underflow, a tie to even
    probe = FE.bits_of(np.array([65504.0, 65519.996, 65520.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11],
                                dtype=np.float32))
    assert FE.f16_rne(probe).tolist() == [0x7BFF, 0x7BFF, 0x7C00, 0x0001, 0x0000, 0x0001, 0x3C00, 0x3C02]
    # every half tie with its neighbours (S has them only by chance): torch again, and the tie itself goes to the even half
    E = FE.half_edge_bits()
    assert E.size == 190_464 and not FE.is_nan32(E).any()
    model = FE.f16_rne(E)
    FE.same_bits(_torch_bits16(torch.from_numpy(FE.f32_of(E).copy()).to(torch.float16)), model, FE.is_nan32(E), E, "f16", "half ties")
    below, tie, above = (model[:E.size // 2].reshape(-1, 3)[:, k] for k in range(3))
    h = np.arange(0x7C00, dtype=np.uint16)
    assert np.array_equal(below, h) and np.array_equal(above, h + 1) and np.array_equal(tie, h + (h & 1)) and tie[-1] == 0x7C00


def test_widening_model_against_torch_cpu():
    h = FE.all_bf16_bits()
    t = torch.from_numpy(h.view(np.int16).copy()).view(torch.bfloat16)
    got = t.float().numpy().view(np.uint32)
    counts = FE.same_bits(got, FE.widen(h), FE.is_nan_bf16(h), h, "f32", "torch's CPU bfloat16 -> float against u16 << 16")
    assert sum(counts.values()) == 0


def test_split_model_against_torch_cpu(S):
    """hi / lo of egk_split_bf16 from the integer model against the same two casts and one subtraction in torch."""
    hi, lo, lo_nan = FE.split_model(S)
    x = torch.from_numpy(FE.f32_of(S).copy())
    th = x.to(torch.bfloat16)
    tl = (x - th.float()).to(torch.bfloat16)
    FE.same_bits(_torch_bits16(th), hi, FE.is_nan32(S), S, "bf16", "split hi")
    FE.same_bits(_torch_bits16(tl), lo, lo_nan, S, "bf16", "split lo")
    assert int(lo_nan.sum()) == int(FE.is_nan32(S).sum()) + int(((S & 0x7FFFFFFF) == 0x7F800000).sum())  # (inf - inf)


@pytest.mark.parametrize("name", ["truncation", "round_half_up", "flush_subnormals", "saturate_to_max", "positive_zero_only", "nan_to_inf"])
def test_helper_catches_mutant(S, name):
    """Each wrong rounding changes elements of S, and the helper refuses it and names the class."""
    wrong, cls = FE.mutants(S)[name]
    want, nan_in = FE.bf16_rne(S), FE.is_nan32(S)
    changed = int(FE.mismatches(wrong, want, nan_in, "bf16").sum())
    print(f"mutant {name}: {changed} elements of S change", FE.class_counts(FE.mismatches(wrong, want, nan_in, "bf16"), S, "bf16"))
    assert changed > 0
    assert FE.class_counts(FE.mismatches(wrong, want, nan_in, "bf16"), S, "bf16")[cls] > 0
    with pytest.raises(AssertionError, match=r"elements differ from the bf16 model") as err:
        FE.same_bits(wrong, want, nan_in, S, "bf16", name)
    assert "in " in str(err.value) and " got " in str(err.value) and " want " in str(err.value) and f"'{cls}'" in str(err.value)


def test_helper_on_nan_and_zero():
    """A NaN input accepts any NaN, of either sign and payload, and nothing else; -0 is not +0."""
    src = np.array([0x7FC00000, 0xFF800001, 0x80000000, 0x00000000], dtype=np.uint32)
    nan_in = FE.is_nan32(src)
    want = FE.bf16_rne(src)
    FE.same_bits(np.array([0xFFFF, 0x7F81, 0x8000, 0x0000], dtype=np.uint16), want, nan_in, src)
    for bad in ([0x7F80, 0x7FC0, 0x8000, 0], [0x7FC0, 0x0000, 0x8000, 0], [0x7FC0, 0x7FC0, 0x0000, 0], [0x7FC0, 0x7FC0, 0x8000, 0x8000]):
        with pytest.raises(AssertionError):
            FE.same_bits(np.array(bad, dtype=np.uint16), want, nan_in, src)


def test_lerp_double_rounding_cases():
    """The builder's own assertions (both counts, ties in f32, off the tie in f64), and that ONE f64 -> bf16 rounding differs from the
    documented two on every case."""
    x, y, w, r32, above = FE.lerp_double_rounding_cases()
    assert int(above.sum()) >= 256 and int((~above).sum()) >= 256
    two = FE.bf16_rne(r32)
    one = FE.single_rounding(r32, above)
    assert bool((one != two).all()) and bool((two & 1 == 0).all())
    assert bool(((w > 0) & (w < 1)).all()) and not FE.is_nan32(x).any() and not FE.is_nan32(y).any()
    with pytest.raises(AssertionError):
        FE.same_bits(one, two, np.zeros(two.shape, dtype=bool), r32, "bf16", "one rounding")


def test_ledger_is_complete():
    """Every defining occurrence of a conversion idiom in csrc is in SITES with a GPU test that exists, or a reason."""
    scanned = FE.scan_sites()
    assert len(scanned) >= 14 and all(fn != "<file scope>" for _, fn, _ in scanned), sorted(scanned)
    assert FE.ledger_problems() == []


def test_ledger_notices_a_missing_entry_and_a_new_routine(tmp_path):
    for key in FE.SITES:
        fewer = {k: v for k, v in FE.SITES.items() if k != key}
        assert any(str(key) in line for line in FE.ledger_problems(fewer)), key
    # a sixth rounding routine, in a new file
    (tmp_path / "new_ops.hip").write_text(
        "namespace egk {\n// (a comment that says (__bf16) is no site)\n"
        "__device__ __forceinline__ bf16_t my_round(float x) {\n    const unsigned u = __float_as_uint(x);\n"
        "    return (bf16_t)((u + 0x7fffu) >> 16);\n}\n}\n")
    found = FE.scan_sites(tmp_path)
    assert found == {("new_ops.hip", "my_round", "0x7fffu"), ("new_ops.hip", "my_round", "(bf16_t)(")}
    assert len(FE.ledger_problems(scanned=FE.scan_sites() | found)) == 2
    missing_test = dict(FE.SITES)
    missing_test[("common.h", "f2bf", "f2bf(")] = {"test": FE.GPU_TESTS + "::test_that_is_not_there"}
    assert len(FE.ledger_problems(missing_test)) == 1
