"""The premises of tests/test_gpu_layouts.py, checked without a GPU: which layouts autograd hands to an op's ``backward`` (a
torch upgrade that changes them fails HERE), what the layout helper of the GPU file builds, and what the normalising helpers of
``egopack_amd.ops`` make of every layout (host logic only: no launch happens on CPU tensors)."""
import pytest
import torch

from tests.test_gpu_layouts import BF, F32, FWD_TAGS, GRAD_TAGS, VEC_GRAD_TAGS, bits, expected_layout, lay, lay_values

ROWS, COLS = 6, 8


class _Probe(torch.autograd.Function):
    """Pass-through that records what its backward receives."""
    seen = None

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        _Probe.seen = g
        return g


def _received(downstream):
    x = torch.randn(ROWS, COLS, requires_grad=True)
    y = _Probe.apply(x)
    z = downstream(y)
    (z * torch.randn(z.shape)).sum().backward()  # (a weighted sum: the loss end of an ordinary training graph)
    g = _Probe.seen
    _Probe.seen = None
    return g


OTHER = torch.randn(ROWS, 5)
W = torch.randn(COLS, ROWS)
# downstream expression -> (strides, storage offset) of the [6, 8] gradient the op's backward receives
TABLE = {
    "cat_first": (lambda y: torch.cat([y, OTHER], 1), (13, 1), 0),
    "cat_second": (lambda y: torch.cat([OTHER, y], 1), (13, 1), 5),
    "sum_rows": (lambda y: y.sum(0), (0, 1), 0),
    "sum_all": (lambda y: y.sum(), (0, 0), 0),
    "transposed_elementwise": (lambda y: y.t() * W, (1, 6), 0),
}
PACKED = {
    "column_slice": lambda y: y[:, 2:6],
    "row_step": lambda y: y[::2],
    "cat_rows": lambda y: torch.cat([y, torch.randn(3, COLS)], 0),
    "stack_index": lambda y: torch.stack([y, y])[1],
    "view_permute": lambda y: y.view(2, 3, COLS).permute(1, 0, 2),
    "transposed_matmul": lambda y: y.t() @ torch.randn(ROWS, 4),
}


@pytest.mark.parametrize("how", list(TABLE))
def test_autograd_hands_out_strided_gradients(how):
    fn, strides, offset = TABLE[how]
    g = _received(fn)
    assert tuple(g.shape) == (ROWS, COLS)
    assert g.stride() == strides and g.storage_offset() == offset
    assert not g.is_contiguous()
    if how == "cat_second":
        assert g.data_ptr() % 16 != 0  # 5 floats into an aligned allocation


@pytest.mark.parametrize("how", list(PACKED))
def test_autograd_hands_out_packed_gradients(how):
    g = _received(PACKED[how])
    assert tuple(g.shape) == (ROWS, COLS) and g.is_contiguous()


@pytest.mark.parametrize("dt", [F32, BF])
@pytest.mark.parametrize("tag", GRAD_TAGS)
def test_backward_delivers_the_gradient_view_unchanged(tag, dt):
    view, big = lay(torch.randn(ROWS, COLS).to(dt), tag)
    x = torch.randn(ROWS, COLS).to(dt).requires_grad_(True)
    _Probe.apply(x).backward(gradient=view)
    g = _Probe.seen
    _Probe.seen = None
    assert g.data_ptr() == view.data_ptr() and g.stride() == view.stride() and g.storage_offset() == view.storage_offset()
    assert g.untyped_storage().data_ptr() == big.untyped_storage().data_ptr()


@pytest.mark.parametrize("dt", [F32, BF, torch.int64])
@pytest.mark.parametrize("tag", GRAD_TAGS)
def test_layout_helper(tag, dt):
    rows, cols = 7, 24  # (a width of whole 16-byte groups in every element type: ld_aligned then moves nothing but the stride)
    vals = (torch.randn(rows, cols) * 4).to(dt)
    view, big = lay(vals, tag)
    want = lay_values(vals, tag)
    assert tuple(view.shape) == (rows, cols) and view.dtype == dt
    assert (view.stride(), view.storage_offset()) == expected_layout(tag, rows, cols, dt)
    assert torch.equal(view, want)  # the same values
    assert view.untyped_storage().data_ptr() == big.untyped_storage().data_ptr()
    # everything outside the view is NaN / -1
    seen = torch.zeros(big.numel(), dtype=torch.bool)
    idx = torch.arange(big.numel()).view(big.shape)
    inside = torch.as_strided(idx.view(-1), view.shape, view.stride(), view.storage_offset()).reshape(-1)
    seen[inside] = True
    outside = big.reshape(-1)[~seen]
    assert bool(torch.isnan(outside).all()) if dt.is_floating_point else bool((outside == -1).all())
    if tag != "col_major":  # (a transposed view fills its buffer: a packed misread returns the transposed values)
        assert outside.numel() > 0 or tag == "packed"
    # a launch that reads the view as packed stays inside the allocation
    assert big.numel() - view.storage_offset() >= rows * cols
    # 16-byte alignment: only ld_offset moves the pointer (20 bytes in f32, 10 in bf16)
    if tag == "ld_offset":
        assert (view.data_ptr() - big.data_ptr()) == 5 * view.element_size() and view.data_ptr() % 16 != 0
    else:
        assert view.data_ptr() % 16 == 0
    if tag == "ld_aligned":
        assert (view.stride(0) * view.element_size()) % 16 == 0


@pytest.mark.parametrize("tag", VEC_GRAD_TAGS)
def test_layout_helper_vectors(tag):
    vals = torch.randn(9)
    view, big = lay(vals, tag)
    assert torch.equal(view, lay_values(vals, tag)) and tuple(view.shape) == (9,)
    assert view.stride() == {"packed": (1,), "column": (8,), "bcast": (0,)}[tag]
    assert big.numel() - view.storage_offset() >= 9
    if tag != "packed":
        assert int(torch.isnan(big).sum()) == big.numel() - (9 if tag == "column" else 1)
    assert torch.equal(bits(view), bits(lay_values(vals, tag)))


# ---- the normalising helpers of ops (host logic: no launch on CPU tensors) ------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF])
def test_packed_tensors_pass_every_helper_untouched(dt):
    from egopack_amd import ops
    x = torch.randn(ROWS, COLS).to(dt)
    for helper in (ops._c, ops._rm, lambda t: ops._match(t, dt), lambda t: ops._ld_rows(t, dt), lambda t: ops._operand_rows(t, dt)):
        assert helper(x) is x  # the hot path: the same object, no copy, no launch


@pytest.mark.parametrize("dt", [F32, BF])
@pytest.mark.parametrize("tag", [t for t in GRAD_TAGS if t != "packed"])
def test_helpers_normalise_every_layout(tag, dt):
    from egopack_amd import ops
    rows, cols = 7, 16
    view, _ = lay(torch.randn(rows, cols).to(dt), tag)
    want = lay_values(view, "packed").contiguous()
    # launches without a leading dimension: packed rows
    for helper in (ops._c, lambda t: ops._match(t, dt)):
        out = helper(view)
        assert out.is_contiguous() and torch.equal(out, want)
    # ``_rm``: its callers forward stride(0) to one-element-at-a-time kernels -- unit column stride, row stride >= width
    out = ops._rm(view)
    assert out.stride(1) == 1 and out.stride(0) >= cols and torch.equal(out, want)
    assert (out is view) == (tag in ("ld_aligned", "ld_offset", "row_step"))
    # ``_ld_rows``: a contraction operand -- the same, and whole 16-byte groups; only the aligned views are read where they lie
    out = ops._ld_rows(view, dt)
    assert out.stride(1) == 1 and out.stride(0) >= cols and torch.equal(out, want)
    assert out.data_ptr() % 16 == 0 and (out.stride(0) * out.element_size()) % 16 == 0
    assert (out is view) == (tag in ("ld_aligned", "row_step"))
    # ``_operand_rows`` reads a gradient where it lies under the same rule (everything else goes through its packing launch)
    assert ops._operand_layout_ok(view, view.element_size()) == (tag in ("ld_aligned", "row_step"))
