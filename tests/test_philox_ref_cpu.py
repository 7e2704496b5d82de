"""tests/philox_ref.py, the host model the GPU mask tests compare with, checked on its own: the published Philox4x32-10 known
answers, the vectorised path against the scalar one, the mask helpers against an element-by-element loop."""
import numpy as np
import pytest

from tests import philox_ref as P

# Random123 (Salmon et al.) kat_vectors, philox4x32 with 10 rounds: counter, key, result
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_known_answers_scalar(counter, key, want):
    assert P.philox4x32_10_scalar(counter, key) == want


def test_known_answers_vectorised():
    c = np.array([k[0] for k in KNOWN], dtype=np.uint64)
    for i, (counter, key, want) in enumerate(KNOWN):
        got = P.philox4x32_10(*counter, *key)
        assert got.dtype == np.uint32 and got.shape == (4,) and tuple(int(v) for v in got) == want
        # as one lane of an array whose other lanes hold the other counters
        got = P.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], *key)
        assert got.shape == (3, 4) and tuple(int(v) for v in got[i]) == want


def test_two_word_wrapper_is_the_core_with_zero_upper_words():
    rng = np.random.default_rng(5)
    for ctr, seed in [(0, 0), (1, 0), (0, 1), (2 ** 64 - 1, 2 ** 64 - 1), (0x85A308D3243F6A88, 0x299F31D0A4093822),
                      *((int(a), int(b)) for a, b in rng.integers(0, 2 ** 64, (8, 2), dtype=np.uint64))]:
        want = P.philox4x32_10_scalar((ctr & P.MASK32, ctr >> 32, 0, 0), (seed & P.MASK32, seed >> 32))
        assert P.philox_u64_scalar(ctr, seed) == want
        assert tuple(int(v) for v in P.philox_u64(np.uint64(ctr), seed)) == want
    # the first known answer is a wrapper value too (upper words 0)
    assert P.philox_u64_scalar(0, 0) == KNOWN[0][2]
    # low and high counter word are not interchangeable, nor are the key words
    assert P.philox_u64_scalar(1, 0) != P.philox_u64_scalar(1 << 32, 0) and P.philox_u64_scalar(0, 1) != P.philox_u64_scalar(0, 1 << 32)


def test_vectorised_against_scalar_on_both_sides_of_2_32():
    rng = np.random.default_rng(11)
    ctrs = np.concatenate([np.arange(2 ** 32 - 100, 2 ** 32 + 100, dtype=np.uint64), np.arange(0, 50, dtype=np.uint64),
                           np.arange(3 * 2 ** 40 + 5, 3 * 2 ** 40 + 55, dtype=np.uint64),
                           np.arange(2 ** 64 - 20, 2 ** 64, dtype=np.uint64),
                           rng.integers(0, 2 ** 64, 100, dtype=np.uint64)])
    for seed in (0x5EEDE60, 11, 0xDEADBEEF12345678):
        got = P.philox_u64(ctrs, seed)
        assert got.shape == (len(ctrs), 4)
        want = np.array([P.philox_u64_scalar(int(c), seed) for c in ctrs], dtype=np.uint32)
        assert np.array_equal(got, want)
    # shape is kept
    assert np.array_equal(P.philox_u64(ctrs[:12].reshape(3, 4), 7).reshape(12, 4), P.philox_u64(ctrs[:12], 7))


def _keep_scalar(word, p):
    return int(np.float32(word >> 8) * np.float32(2.0 ** -24) >= np.float32(p))


def test_keep_decision_edges():
    # r >> 8 = k: u = k 2^-24 exactly; p = 0.5 keeps from k = 2^23 on
    words = np.array([0, 0xFF, (1 << 31) - 1, 1 << 31, (1 << 31) + 0xFF, 0xFFFFFFFF], dtype=np.uint32)
    assert P.keep_from_words(words, 0.5).tolist() == [0, 0, 0, 1, 1, 1]
    assert P.keep_from_words(words, 0.0).tolist() == [1] * 6
    # p is compared as an f32: 0.1 rounds UP to f32 (0.100000001490116...), so k = ceil(f32(0.1) 2^24) = 1677722 is the first kept
    k = 1677722
    assert np.float32(0.1) * np.float32(2.0 ** 24) > k - 1 and np.float32(0.1) * np.float32(2.0 ** 24) <= k
    assert P.keep_from_words(np.array([(k - 1) << 8, k << 8], dtype=np.uint32), 0.1).tolist() == [0, 1]


@pytest.mark.parametrize("rows,cols", [(3, 5), (2, 8), (4, 250), (2, 257), (2, 1030)])
def test_row_mask_helper_against_a_loop(rows, cols):
    seed, offset, p = 0xABCDEF0123, 2 ** 32 - 70, 0.25
    S = 64 if cols <= 256 else 256 if cols <= 1024 else 1024
    assert P.row_stride(cols) == S
    got = P.keep_mask_rows(seed, offset, rows, cols, p)
    assert got.dtype == np.uint8 and got.shape == (rows, cols)
    for r in range(rows):
        for c in range(cols):
            word = P.philox_u64_scalar(offset + r * S + c // 4, seed)[c % 4]
            assert got[r, c] == _keep_scalar(word, p), (r, c)
    assert P.row_intervals(offset, rows, cols) == [(offset + r * S, offset + r * S + (cols + 3) // 4) for r in range(rows)]
    assert np.array_equal(P.row_counters(offset, rows, cols)[:, 0], np.array([offset + r * S for r in range(rows)], dtype=np.uint64))


def test_row_stride_classes():
    assert [P.row_stride(c) for c in (1, 256, 257, 1024, 1025, 4096)] == [64, 64, 256, 256, 1024, 1024]
    with pytest.raises(ValueError):
        P.row_stride(4097)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021])
def test_flat_mask_helper_against_a_loop(n):
    seed, offset, p = 77, 3 * 2 ** 40 + 5, 0.5
    got = P.keep_mask_flat(seed, offset, n, p)
    assert got.dtype == np.uint8 and got.shape == (n,)
    for i in range(n):
        assert got[i] == _keep_scalar(P.philox_u64_scalar(offset + i // 4, seed)[i % 4], p), i
    assert P.flat_intervals(offset, n) == [(offset, offset + (n + 3) // 4)]


def test_offsets_wrap_like_uint64():
    a = P.keep_mask_flat(9, 2 ** 64 - 2, 16, 0.5)  # counters 2^64 - 2, 2^64 - 1, 0, 1
    b = np.concatenate([P.keep_mask_flat(9, 2 ** 64 - 2, 8, 0.5), P.keep_mask_flat(9, 0, 8, 0.5)])
    assert np.array_equal(a, b)


def test_interval_helpers():
    assert P.disjoint([(0, 4), (4, 8), (10, 11)]) and not P.disjoint([(0, 5), (4, 8)]) and P.disjoint([])
    assert not P.disjoint([(10, 20), (0, 11)])
    assert P.span([(5, 9), (1, 3)]) == (1, 9)
    # rows of one launch never share a counter: the row stride covers a row of the widest width of its class
    for cols in (40, 256, 1024, 4096):
        assert P.disjoint(P.row_intervals(123, 5, cols))


def test_the_model_does_not_import_the_package():
    imports = [ln.strip() for ln in open(P.__file__) if ln.lstrip().startswith(("import ", "from "))]
    assert imports == ["import numpy as np"], imports
