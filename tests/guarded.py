"""Guard-banded, padded operands for the kernel tests (plain helpers: no fixtures, nothing collected from here).

Every operand lives in ONE allocation laid out as

    [ front guard | row 0 : width payload + (ld - width) padding | row 1 ... | behind guard ]

with `guard = max(4096, 256 * ld)` elements on each side -- one full row block of the largest GEMM tile -- so that a small
overrun at a tile tail lands in memory the test owns instead of in a neighbour block of the caching allocator:

  * guard_in: guards and padding columns hold `fill` (NaN for floats; for integer operands a value the caller picks so that a
    read of it is HARMFUL: a row number outside the table raises the kernel's out-of-range flag, a live / unmasked marker
    un-masks a NaN row, ...).  An over-read that reaches the result shows up as a NaN, a raised flag or a wrong value
    (compare with assert_values below: it fails on NaN, which `err > tol` does not).
    check() asserts that the kernel wrote nothing into the operand, guards and padding included.
  * guard_out: guards and padding columns hold a canary bit pattern, the payload a pre-fill (a NaN pattern for floats, a
    second canary for ints).  check() asserts that every guard / padding element still holds the canary and that no payload
    element still holds the pre-fill (every output was written), and names the first offender: in front, behind, padding
    column c of row r, or payload element (r, c).  All comparisons go through an int32 view -- never `==` on floats.
  * poison(ws): a workspace filled with NaN, for scratch the contract says is written before it is read.

LIMIT (by design): value detection cannot see an over-read whose value is later discarded by a select (`ok ? t : 0`): the
guard value never reaches an output, so such reads are not detected here.

Memory: the guards are 256 * ld elements per side and the handle keeps a bit snapshot of the whole allocation, so an operand
with a long leading dimension (a transposed A of 24636 columns: 25 MB per guard) costs about four guards of device memory.

`device="cpu"` runs the same harness on host tensors (tests/test_guarded_cpu.py plants defects in numpy stand-ins through
Handle.raw(), the C view of an operand: flat storage + element offset of the payload)."""
import numpy as np
import torch

CANARY = 0x5A5AC3C3          # guards / padding of an output (as a float: 1.54e16, finite)
PREFILL_F32 = 0x7FC0BEEF     # payload pre-fill of a float output: a quiet NaN with a payload no arithmetic produces
PREFILL_I32 = -0x3A3A3A3B    # payload pre-fill of an int output ("second canary")
_DTYPES = (torch.float32, torch.int32)


def assert_values(got, want, rtol=1e-5, atol=1e-6, what=""):
    """|got - want| <= atol + rtol |want| element-wise, written so that a NaN (or inf) in `got` FAILS: the guards, the padding,
    the pre-fills and poisoned scratch are NaN, and a comparison of the form `err > tol` is false for them."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
        tol = atol + rtol * np.abs(want)
        bad = ~(err <= tol)
    if bad.any():
        i = tuple(int(j) for j in np.unravel_index(int(np.argmax(bad)), bad.shape))
        n_nan = int(np.isnan(got).sum())
        finite = err[np.isfinite(err)]
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} elements off ({n_nan} NaN); first at {i}: got {got[i]!r} want {want[i]!r} "
                             f"(tol {tol[i]:.3e}); max finite abs err {finite.max() if finite.size else float('nan'):.3e}")


def guard_len(ld):
    return max(4096, 256 * int(ld))


def _bits(t):
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def _fill_bits(fill, dtype):
    if dtype == torch.int32:
        return int(fill)
    return int(np.array([fill], dtype=np.float32).view(np.int32)[0])


class Handle:
    """One guarded operand: `buf` the whole allocation (1-D), `start` the element offset of payload (0, 0), `rows` rows of
    `width` payload elements at stride `ld`, `guard` elements on each side (+ up to 4 elements of alignment slack in front)."""

    def __init__(self, buf, start, rows, width, ld, shape, is_out):
        self.buf, self.start, self.rows, self.width, self.ld, self.shape, self.is_out = buf, start, rows, width, ld, shape, is_out
        self.prefilled = is_out
        self.view = buf[start:start + rows * ld].view(rows, ld)[:, :width]
        if len(shape) == 1:
            self.view = self.view[0]
        self._snap = _bits(buf).clone()

    # -- what the test hands to the kernel
    @property
    def tensor(self):
        return self.view

    def raw(self):
        """(flat numpy array sharing the allocation, element offset of the payload): the operand as C sees it.  CPU only."""
        return self.buf.numpy(), self.start

    def payload(self):
        """a contiguous copy of the payload in its logical shape"""
        return self.buf[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width].reshape(self.shape).clone()

    def fill_payload(self, values):
        """give an output finite starting values (the beta != 0 cases); the every-output-written check no longer applies"""
        v = torch.as_tensor(np.array(values)).to(self.buf.dtype).reshape(self.rows, self.width)
        self.buf[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width].copy_(v)
        self._snap = _bits(self.buf).clone()
        self.prefilled = False

    def set_guards(self, front, behind):
        """different harmful values in front of and behind an (input) operand; padding columns keep their fill"""
        self.buf[:self.start].fill_(front)
        self.buf[self.start + self.rows * self.ld:].fill_(behind)
        self._snap = _bits(self.buf).clone()

    # -- checks
    def _where(self, i):
        j = i - self.start
        if j < 0:
            return f"in front of the operand ({-j} elements before its first)"
        if j >= self.rows * self.ld:
            return f"behind the operand ({j - self.rows * self.ld} elements past its last row)"
        r, c = divmod(j, self.ld)
        return f"padding column {c} of row {r}" if c >= self.width else f"payload element ({r}, {c})"

    def _payload_mask(self):
        m = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        m[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width] = True
        return m

    def _first(self, bad):
        return int(torch.nonzero(bad)[0].item())

    def check_untouched(self, what="operand"):
        """nothing of the allocation changed since it was set up (inputs; outputs of a call that returned an error code)"""
        bad = _bits(self.buf) != self._snap
        if bool(bad.any()):
            i = self._first(bad)
            raise AssertionError(f"{what}: {int(bad.sum())} elements were written; first at flat index {i}: {self._where(i)}")

    def check(self, what="operand"):
        if not self.is_out:
            return self.check_untouched(what)
        now, pay = _bits(self.buf), self._payload_mask()
        bad = (now != self._snap) & ~pay
        if bool(bad.any()):
            i = self._first(bad)
            raise AssertionError(f"{what}: {int(bad.sum())} canary elements disturbed; first at flat index {i}: {self._where(i)} "
                                 f"holds {int(now[i]) & 0xFFFFFFFF:#010x}")
        if self.prefilled:
            pre = PREFILL_I32 if self.buf.dtype == torch.int32 else PREFILL_F32
            pre = pre - (1 << 32) if pre >= (1 << 31) else pre
            bad = (now == pre) & pay
            if bool(bad.any()):
                i = self._first(bad)
                raise AssertionError(f"{what}: {int(bad.sum())} outputs were never written; first: {self._where(i)}")


def _alloc(rows, width, ld, dtype, device, offset, bits, guard=None):
    assert dtype in _DTYPES, dtype
    assert ld >= width and offset in (0, 1, 2, 3)
    g = guard_len(ld) if guard is None else int(guard)
    assert g >= 4096 and g % 4 == 0, g
    buf = torch.empty(g + 8 + rows * ld + g, dtype=dtype, device=device)
    assert buf.data_ptr() % 4 == 0
    start = g + (-(buf.data_ptr() // 4 + g)) % 4 + offset  # 16-byte aligned, then the deliberate misalignment
    _bits(buf).fill_(bits if bits < (1 << 31) else bits - (1 << 32))
    return buf, start


def guard_in(x, ld=None, fill=float("nan"), device="cuda", offset=0, guard=None):
    """x (numpy / tensor, 1-D or 2-D; more dimensions: the leading ones are flattened into rows) -> (view, handle).  The view has
    x's values at row stride `ld` (default: the width), a 16-byte aligned data_ptr() (+ `offset` floats for the deliberately
    misaligned cases); guards and padding columns hold `fill`.  `guard`: elements per side instead of guard_len(ld), for the long
    flat operands of element-wise kernels (millions of elements in one row: nothing there strides by ld, and 256 * ld is GBs)."""
    x = torch.as_tensor(np.array(x))  # a copy: read-only reference arrays are welcome
    dtype = torch.int32 if not x.dtype.is_floating_point else torch.float32
    shape = tuple(x.shape) if x.dim() <= 2 else (int(np.prod(x.shape[:-1])), x.shape[-1])
    rows, width = (1, shape[0]) if len(shape) == 1 else shape
    ld = width if ld is None else int(ld)
    buf, start = _alloc(rows, width, ld, dtype, device, offset, _fill_bits(fill, dtype) & 0xFFFFFFFF, guard)
    buf[start:start + rows * ld].view(rows, ld)[:, :width].copy_(x.to(dtype).reshape(rows, width))
    h = Handle(buf, start, rows, width, ld, shape, is_out=False)
    assert h.view.data_ptr() % 16 == 4 * offset
    return h.view, h


def guard_out(shape, ld=None, dtype=torch.float32, device="cuda", offset=0, guard=None):
    """-> (view, handle) of an output of `shape` (1-D or 2-D) at row stride `ld`: canaries around and between the rows, the
    payload pre-filled (NaN pattern / second canary) so that handle.check() can tell an output that was never written."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    if len(shape) > 2:
        shape = (int(np.prod(shape[:-1])), shape[-1])
    rows, width = (1, shape[0]) if len(shape) == 1 else shape
    ld = width if ld is None else int(ld)
    buf, start = _alloc(rows, width, ld, dtype, device, offset, CANARY, guard)
    pre = PREFILL_I32 if dtype == torch.int32 else PREFILL_F32
    _bits(buf)[start:start + rows * ld].view(rows, ld)[:, :width].fill_(pre)
    h = Handle(buf, start, rows, width, ld, shape, is_out=True)
    assert h.view.data_ptr() % 16 == 4 * offset
    return h.view, h


def poison(ws):
    """fill a workspace with NaN (every byte 0xFF for byte workspaces: NaN as fp32, -1 as int32).  Not for scratch whose
    contract is "zero before the first call" (ebn_dvn_fwd_train_f32's `stat`)."""
    if ws.dtype.is_floating_point:
        ws.fill_(float("nan"))
    else:
        ws.view(torch.uint8).fill_(0xFF)
    return ws
