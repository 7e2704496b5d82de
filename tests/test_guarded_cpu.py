"""The guard-band helper (tests/guarded.py) fails when a "kernel" is wrong: plain torch stand-ins on the CPU."""
import re

import pytest
import torch

from tests.guarded import GUARD_ELEMS, GUARD_ROWS, Guarded1D, Guarded2D, pad_cols, sentinel_bits

ROWS, COLS = 5, 7


def _src():
    return torch.arange(ROWS * COLS, dtype=torch.float32).reshape(ROWS, COLS) + 1.0


def _copy_kernel(src, dst_buf, dst_start, ld, rows, cols, row_shift=0, col_shift=0, extra_cols=0, extra_rows=0):
    """dst[r, c] = src[r, c] through raw flat addressing (what a kernel does), with optional defects."""
    flat = dst_buf.view(-1)
    for r in range(rows + extra_rows):
        for c in range(cols + extra_cols):
            v = src[min(r, rows - 1), min(c, cols - 1)]
            flat[dst_start + (r + row_shift) * ld + c + col_shift] = v


def _fails_at(g, what, row, col):
    with pytest.raises(AssertionError) as e:
        g.assert_untouched(what)
    msg = str(e.value)
    assert msg.startswith(what + ":"), msg
    m = re.search(r"first at \(row (-?\d+), col (-?\d+)\)", msg)
    assert m and (int(m.group(1)), int(m.group(2))) == (row, col), msg


def test_guards_are_at_least_what_the_kernels_could_overrun():
    assert GUARD_ROWS >= 256 and GUARD_ELEMS >= 4096
    assert pad_cols(torch.float32) == 4 and pad_cols(torch.bfloat16) == 8


@pytest.mark.parametrize("ld", [COLS, COLS + 4])
def test_a_correct_strided_copy_passes(ld):
    g = Guarded2D(ROWS, COLS, torch.float32, "cpu", ld=ld, guard_rows=3)
    assert g.is_sentinel().all() and torch.isnan(g.view).all()  # an output keeps the sentinel until it is written
    _copy_kernel(_src(), g.buf, g._start, g.ld, ROWS, COLS)
    g.assert_untouched("dst")
    assert torch.equal(g.view, _src()) and g.view.stride() == (ld, 1)
    assert g.ptr == g.buf.data_ptr() + 4 * (3 * ld)


def test_a_forgotten_element_shows_against_the_reference():
    g = Guarded2D(ROWS, COLS, torch.float32, "cpu", guard_rows=2)
    _copy_kernel(_src(), g.buf, g._start, g.ld, ROWS, COLS - 1)
    g.assert_untouched("dst")
    assert not torch.equal(g.view, _src()) and torch.isnan(g.view[:, -1]).all() and int(g.is_sentinel().sum()) == ROWS


def test_one_element_past_the_row_end_is_seen():
    g = Guarded2D(ROWS, COLS, torch.float32, "cpu", ld=COLS + 4, guard_rows=3)
    _copy_kernel(_src(), g.buf, g._start, g.ld, ROWS, COLS, extra_cols=1)
    _fails_at(g, "dst", 0, COLS)


def test_one_element_past_the_row_end_is_seen_without_a_pad():
    # ld == cols: the overrun of rows 0 .. ROWS-2 lands on the next row's first element (later overwritten: not seen), the
    # last row's lands in the guard
    g = Guarded2D(ROWS, COLS, torch.float32, "cpu", guard_rows=3)
    _copy_kernel(_src(), g.buf, g._start, g.ld, ROWS, COLS, extra_cols=1)
    _fails_at(g, "dst", ROWS, 0)


def test_one_row_past_the_last_row_is_seen():
    g = Guarded2D(ROWS, COLS, torch.float32, "cpu", ld=COLS + 4, guard_rows=3)
    _copy_kernel(_src(), g.buf, g._start, g.ld, ROWS, COLS, extra_rows=1)
    _fails_at(g, "dst", ROWS, 0)


def test_one_element_before_the_window_is_seen():
    g = Guarded2D(ROWS, COLS, torch.float32, "cpu", ld=COLS + 4, guard_rows=3, offset_elems=2)
    _copy_kernel(_src(), g.buf, g._start, g.ld, ROWS, COLS)
    g.buf.view(-1)[g._start - 1] = 1.0
    _fails_at(g, "dst", -1, COLS + 3)
    h = Guarded1D(10, torch.float32, "cpu", guard=16)
    h.view.fill_(2.0)
    h.assert_untouched("flat")
    h.buf[h._start - 1] = 2.0
    _fails_at(h, "flat", 0, -1)
    h = Guarded1D(10, torch.float32, "cpu", guard=16)
    h.buf[h._start + 10] = 2.0
    _fails_at(h, "flat", 0, 10)


def test_a_store_into_the_pad_of_a_wider_ld_is_seen():
    g = Guarded2D(ROWS, COLS, torch.float32, "cpu", ld=COLS + 4, guard_rows=3)
    _copy_kernel(_src(), g.buf, g._start, g.ld, ROWS, COLS)
    g.buf.view(-1)[g._start + 2 * g.ld + COLS + 3] = 0.0  # (a kernel that zero-fills up to ld instead of cols)
    _fails_at(g, "dst", 2, COLS + 3)


def test_rewriting_the_same_value_into_a_guard_is_not_a_change_but_any_other_bit_is():
    g = Guarded2D(ROWS, COLS, torch.float32, "cpu", guard_rows=1)
    g.view.zero_()
    g._raw[0] = sentinel_bits(torch.float32) ^ 1  # another NaN: equal under no float comparison, different bits
    _fails_at(g, "dst", -1, 0)


def test_an_input_read_beyond_its_window_poisons_the_result():
    x = Guarded2D(ROWS, COLS, torch.float32, "cpu", ld=COLS + 4, guard_rows=2, init=_src())
    flat = x.buf.view(-1)

    def row_sums(cols, rows):
        return torch.stack([flat[x._start + r * x.ld: x._start + r * x.ld + cols].sum() for r in range(rows)])

    assert torch.equal(row_sums(COLS, ROWS), _src().sum(1))
    assert torch.isnan(row_sums(COLS + 1, ROWS)).all()          # reads one pad column
    assert torch.isnan(row_sums(COLS, ROWS + 1)[-1])            # reads one guard row
    x.assert_untouched("x")


def test_a_gather_through_the_poison_index_returns_the_poison_row():
    n_rows, poison = 6, 6  # the table has one extra row, number 6, that holds NaNs
    table = Guarded2D(n_rows + 1, 4, torch.float32, "cpu", guard_rows=2)
    table.view[:n_rows] = torch.arange(n_rows * 4, dtype=torch.float32).reshape(n_rows, 4)
    for dt in (torch.int64, torch.int32):
        idx = Guarded1D(3, dt, "cpu", guard=8, init=torch.tensor([4, 0, 2]), poison=poison)
        assert idx.buf.tolist() == [poison] * 8 + [4, 0, 2] + [poison] * 8
        got = table.view[idx.buf[idx._start:idx._start + 4].long()]  # one index too many
        assert torch.equal(got[:3], table.view[[4, 0, 2]]) and torch.isnan(got[3]).all()
        idx.assert_untouched("idx")
        idx.buf[0] = 0
        _fails_at(idx, "idx", 0, -8)


@pytest.mark.parametrize("dtype,bits", [(torch.float32, 0x7FC0DEAD), (torch.bfloat16, 0x7FC1), (torch.float16, 0x7FC1),
                                        (torch.int16, 0x7FC1), (torch.float64, 0x7FF80000DEADDEAD), (torch.int32, 77),
                                        (torch.int64, 77), (torch.uint8, 0xA5)])
def test_the_sentinel_survives_a_round_trip(dtype, bits):
    for g in (Guarded2D(3, 5, dtype, "cpu", ld=5 + pad_cols(dtype), guard_rows=2, offset_elems=1, poison=77),
              Guarded1D(9, dtype, "cpu", guard=4, offset_elems=3, poison=77)):
        width = 8 * g._raw.element_size()
        assert all((v & ((1 << width) - 1)) == bits for v in g._raw.tolist())
        if dtype.is_floating_point:
            assert torch.isnan(g.buf).all()
        moved = g.buf.clone().to("cpu").contiguous()  # (a device round trip on a GPU box: bits, not values, are kept)
        assert torch.equal(moved.view(g._raw.dtype), g._raw)
        g.assert_untouched("fresh")
        assert g.is_sentinel().all()
        init = torch.ones(g.view.shape, dtype=dtype)
        g.view.copy_(init)
        g.assert_untouched("written window")
        assert not g.is_sentinel().any()


def test_empty_windows_are_allowed():
    g = Guarded2D(0, 8, torch.float32, "cpu", guard_rows=2)
    g.assert_untouched("no rows")
    assert g.view.shape == (0, 8)
    h = Guarded1D(0, torch.int64, "cpu", guard=4, poison=3)
    h.assert_untouched("no elements")
    assert h.view.numel() == 0 and h.ptr == h.buf.data_ptr() + 4 * 8
