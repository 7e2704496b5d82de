"""Guard-band buffers: "a launch touches only what its arguments name".

A ``Guarded2D`` / ``Guarded1D`` is ONE allocation in which the logical operand is a window; everything around the window
(guard rows in front and behind, the pad columns of a leading dimension wider than the row, optional elements in front of
the whole thing) holds a sentinel.  ``assert_untouched`` compares every element outside the window bit for bit with that
sentinel, so a store that leaves the window is seen; as an INPUT, the NaN sentinel (or the poison index) makes a read that
leaves the window and reaches the result show up in the result.  Plain torch, works on cpu and cuda tensors alike
(tests/test_guarded_cpu.py runs it without a GPU).

The guards and how they were chosen (a stray access of a defective kernel has to stay INSIDE the allocation):

  GUARD_ROWS = 256   the tallest output tile of the library is 256 rows (egopack_amd/csrc/gemm.hip: variant 7, the
                     256 x 256 tile, ``tiles_m = cdiv(M, 256)``; the others are 64 / 96 / 128 / 192 rows), so a tile
                     that forgets its ragged-row mask stays inside the guard.  The row kernels walk rows one wave (or one
                     workgroup of at most 16 waves) at a time: an overrun of a whole workgroup's rows is 16 rows.
  GUARD_ELEMS = 4096 flat arrays: one full workgroup of the hardware's largest size (1024 threads) storing a 4-element
                     vector each -- more than any flat kernel's tail can overrun by (their vectors are 4 or 8 elements
                     wide, the tail is handled by at most one workgroup).
  PAD_COLS(dtype)    the smallest ``ld - cols`` the cases use: one 16-byte vector (4 f32 / 8 bf16 elements); a vector
                     store that starts at the last logical column ends inside the pad or the next row of the same buffer.

Nothing here hands a kernel a wild index: integer buffers are filled with a caller-chosen ``poison`` that is a VALID value
for the role (the number of a dedicated poison row of the table that holds NaNs).
"""
import torch

GUARD_ROWS = 256
GUARD_ELEMS = 4096

# sentinels, as the bit pattern of the element's own width
_SENTINEL_BITS = {
    torch.float32: 0x7FC0DEAD,            # quiet NaN, payload 0xDEAD
    torch.bfloat16: 0x7FC1,               # quiet NaN
    torch.float16: 0x7FC1,                # NaN (exponent all ones, mantissa 0x3C1)
    torch.int16: 0x7FC1,                  # raw 16-bit words that hold bf16 / IEEE half values
    torch.float64: 0x7FF80000DEADDEAD,    # quiet NaN, payload 0xDEADDEAD
    torch.uint8: 0xA5,
}
_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.int16: torch.int16,
             torch.float64: torch.int64, torch.uint8: torch.uint8, torch.int32: torch.int32, torch.int64: torch.int64}


def pad_cols(dtype) -> int:
    """Elements of one 16-byte vector."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def _signed(bits: int, dtype) -> int:
    if dtype == torch.uint8:
        return bits
    width = torch.empty((), dtype=dtype).element_size() * 8
    return bits - (1 << width) if bits >= 1 << (width - 1) else bits


def sentinel_bits(dtype, poison=None) -> int:
    """The sentinel of ``dtype`` as a (signed) integer of the same width."""
    if dtype in (torch.int32, torch.int64):
        return int(0 if poison is None else poison)
    return _signed(_SENTINEL_BITS[dtype], _INT_VIEW[dtype])


class Guarded2D:
    """``[rows, cols]`` window with strides ``(ld, 1)`` inside one sentinel-filled buffer of
    ``offset_elems + (guard_rows + rows + guard_rows) * ld`` elements."""

    def __init__(self, rows, cols, dtype, device, ld=None, guard_rows=GUARD_ROWS, offset_elems=0, init=None, poison=None):
        ld = cols if ld is None else int(ld)
        if ld < cols or rows < 0 or cols < 0 or guard_rows < 0 or offset_elems < 0:
            raise ValueError("Guarded2D: bad geometry")
        self.rows, self.cols, self.ld, self.dtype = int(rows), int(cols), ld, dtype
        self.guard_rows, self.offset = int(guard_rows), int(offset_elems)
        self._bits = sentinel_bits(dtype, poison)
        self._start = self.offset + self.guard_rows * ld
        total = self.offset + (2 * self.guard_rows + self.rows) * ld
        self._raw = torch.empty(max(total, 1), dtype=_INT_VIEW[dtype], device=device)
        self._raw.fill_(self._bits)
        self.buf = self._raw.view(dtype)
        self.view = self.buf.as_strided((self.rows, self.cols), (ld, 1), self._start)
        if init is not None:
            if tuple(init.shape) != (self.rows, self.cols):
                raise ValueError(f"Guarded2D: init is {tuple(init.shape)}, the window is {(self.rows, self.cols)}")
            self.view.copy_(init.to(dtype) if init.dtype != dtype else init)

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self._start * self.buf.element_size()

    def bits(self) -> torch.Tensor:
        """The window as integers of the element's width (a copy)."""
        return self._raw.as_strided((self.rows, self.cols), (self.ld, 1), self._start).clone()

    def assert_untouched(self, what: str) -> None:
        probe = self._raw.clone()
        probe.as_strided((self.rows, self.cols), (self.ld, 1), self._start).fill_(self._bits)
        bad = (probe != self._bits).nonzero()
        if bad.numel():
            flat = int(bad[0, 0])
            rel = flat - self._start
            row, col = (rel // self.ld, rel % self.ld) if self.ld else (0, rel)
            raise AssertionError(
                f"{what}: {bad.shape[0]} element(s) outside the [{self.rows}, {self.cols}] window (ld {self.ld}) changed; "
                f"first at (row {row}, col {col}) relative to the window "
                f"(bits {int(probe[flat]) & ((1 << 8 * probe.element_size()) - 1):#x}, sentinel "
                f"{self._bits & ((1 << 8 * probe.element_size()) - 1):#x})")

    def is_sentinel(self) -> torch.Tensor:
        """bool [rows, cols]: window elements that still hold the sentinel bits."""
        return self.bits() == self._bits


class Guarded1D(Guarded2D):
    """``n`` elements between two guards of ``guard`` elements (a one-row window: the failure message's column is the
    element offset from the window's first element, negative in front of it)."""

    def __init__(self, n, dtype, device, guard=GUARD_ELEMS, offset_elems=0, init=None, poison=None):
        n = int(n)
        if n < 0 or guard < 0 or offset_elems < 0:
            raise ValueError("Guarded1D: bad geometry")
        self.rows, self.cols, self.ld, self.dtype = 1, n, 0, dtype
        self.n, self.guard_rows, self.offset = n, 0, int(offset_elems)
        self.guard = int(guard)
        self._bits = sentinel_bits(dtype, poison)
        self._start = self.offset + self.guard
        self._raw = torch.empty(self.offset + 2 * self.guard + n + (1 if n + guard + offset_elems == 0 else 0),
                                dtype=_INT_VIEW[dtype], device=device)
        self._raw.fill_(self._bits)
        self.buf = self._raw.view(dtype)
        self.view = self.buf.as_strided((n,), (1,), self._start)
        if init is not None:
            if init.numel() != n:
                raise ValueError(f"Guarded1D: init has {init.numel()} elements, the window {n}")
            self.view.copy_(init.reshape(-1).to(dtype) if init.dtype != dtype else init.reshape(-1))

    def bits(self) -> torch.Tensor:
        return self._raw[self._start:self._start + self.n].clone()

    def assert_untouched(self, what: str) -> None:
        probe = self._raw.clone()
        probe[self._start:self._start + self.n] = self._bits
        bad = (probe != self._bits).nonzero()
        if bad.numel():
            flat = int(bad[0, 0])
            mask = (1 << 8 * probe.element_size()) - 1
            raise AssertionError(
                f"{what}: {bad.shape[0]} element(s) outside the {self.n}-element window changed; first at (row 0, col "
                f"{flat - self._start}) relative to the window (bits {int(probe[flat]) & mask:#x}, sentinel {self._bits & mask:#x})")
