"""Guarded output buffers and poisoned operands for the memory-contract tests (test_kernel_bounds_gpu.py).

``guarded`` lays one flat allocation out as ``front guard | rows * ld payload | back guard`` with EVERY byte set to a sentinel bit
pattern that finite arithmetic cannot produce, hands the kernel the strided ``[rows, cols]`` view of the payload, and afterwards
checks bit for bit that the guards and the pad columns ``cols .. ld - 1`` still hold the sentinel (nothing was stored outside the
result) and that no element of the view still does (everything was stored).  ``poisoned`` is the same idea for operands: the data
inside, a chosen value (NaN where a kernel has no right to read) in the pad columns and in extra rows behind the last one.
"""
import torch

# dtype -> (integer dtype of the same width, sentinel).  Floats: a quiet NaN with a fixed payload (hardware-made NaNs are the
# canonical 0x7E00 / 0x7FC00000 / 0x7FF8000000000000, never these); uint8 / int16: 0xA5 bytes.
_SENTINELS = {
    torch.float16: (torch.int16, 0x7DA5),
    torch.float32: (torch.int32, 0x7FC5A5A5),
    torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
    torch.uint8: (torch.uint8, 0xA5),
    torch.int16: (torch.int16, 0xA5A5 - 0x10000),
}
FRONT = 4096            # elements of the front guard (a multiple of 256 bytes for every dtype)


def _round_up(n, k):
    return (n + k - 1) // k * k


class GuardChecker:
    def __init__(self, bits, sentinel, front, rows, cols, ld):
        self.bits, self.sentinel, self.front, self.rows, self.cols, self.ld = bits, sentinel, front, rows, cols, ld

    def _payload(self):
        return self.bits[self.front:self.front + self.rows * self.ld].view(self.rows, self.ld)

    def _where(self, flat_index):
        """(row, column) of a flat element index relative to the payload (rows < 0: front guard, >= rows: back guard)."""
        rel = int(flat_index) - self.front
        return rel // self.ld, rel % self.ld

    def assert_intact(self, name="buffer"):
        """Both guards and every pad column of every row are bit-identical to the sentinel."""
        bad = self.bits != self.sentinel
        pay = bad[self.front:self.front + self.rows * self.ld].view(self.rows, self.ld)
        inside = pay[:, :self.cols]
        count = int(bad.sum()) - int(inside.sum())
        if count == 0:
            return
        bad = bad.clone()
        bad[self.front:self.front + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        first = int(torch.nonzero(bad.reshape(-1))[0])
        row, col = self._where(first)
        region = "front guard" if row < 0 else ("back guard" if row >= self.rows else "pad columns")
        raise AssertionError(f"{name}: {count} element(s) written outside the [{self.rows}, {self.cols}] result (ld {self.ld}); "
                             f"first at row {row}, column {col} ({region})")

    def assert_untouched(self, name="buffer"):
        """Nothing at all was written (a launcher that refuses a layout must refuse it before any store)."""
        count = int((self.bits != self.sentinel).sum())
        if count:
            row, col = self._where(int(torch.nonzero((self.bits != self.sentinel).reshape(-1))[0]))
            raise AssertionError(f"{name}: {count} element(s) written by a call that was refused; first at row {row}, column {col}")

    def assert_fully_written(self, name="buffer"):
        """No element of the [rows, cols] view still holds the sentinel bit pattern."""
        left = self._payload()[:, :self.cols] == self.sentinel
        count = int(left.sum())
        if count:
            idx = int(torch.nonzero(left.reshape(-1))[0])
            raise AssertionError(f"{name}: {count} element(s) of the [{self.rows}, {self.cols}] result never written; "
                                 f"first at row {idx // self.cols}, column {idx % self.cols}")


def guarded(rows, cols, ld, dtype, device, back_rows=256, sentinel=None):
    """(view [rows, cols] with row stride ld, GuardChecker).  The back guard holds >= back_rows * ld + 4096 elements (a whole
    over-run tile of 256 rows lands in it), the front guard 4096; both are multiples of 256 bytes.  ``sentinel`` overrides the
    fill pattern (uint8 outputs, where 0xA5 is a legal value: run twice with two sentinels and compare the results)."""
    assert rows > 0 and 0 < cols <= ld
    idt, default = _SENTINELS[dtype]
    s = default if sentinel is None else sentinel
    back = _round_up(back_rows * ld + 4096, 256)
    pay = rows * ld
    bits = torch.full((FRONT + _round_up(pay, 256) + back,), s, dtype=idt, device=device)
    view = bits.view(dtype)[FRONT:FRONT + pay].view(rows, ld)[:, :cols]
    return view, GuardChecker(bits, s, FRONT, rows, cols, ld)


def poisoned(t, rows, cols, ld, pad_value, device=None, extra_rows=256):
    """The [rows, cols] view (row stride ld) of a buffer that holds ``t`` with ``pad_value`` in the pad columns cols .. ld - 1 and in
    ``extra_rows`` whole rows behind the last one."""
    assert tuple(t.shape) == (rows, cols) and cols <= ld
    buf = torch.full((rows + extra_rows, ld), pad_value, dtype=t.dtype)
    buf[:rows, :cols] = t
    if device is not None:
        buf = buf.to(device)
    return buf[:rows, :cols]
