"""TEST INFRASTRUCTURE: output buffers that can tell what a launch did to them.

The kernel tests compare what a launch stored with a reference; two things such a comparison cannot see on an exact-size
``torch.empty`` buffer:

  * an element the kernel never wrote.  The caching allocator hands a test the block the previous test (the same case under another
    kernel variant, same seeded inputs) just freed -- it still holds that run's CORRECT result, so a skipped 16-byte store or a
    skipped ragged tile reads as correct (tests/test_guarded_out.py shows it);
  * a store outside the tensor.  It lands in the allocator's neighbouring block and nobody looks there.

``guarded(shape, dtype)`` allocates one flat byte buffer ``[guard | payload | guard]``: GUARD_BYTES bytes of GUARD_BYTE on either
side (the rear guard starts at the payload's last byte + 1), the payload 256-byte aligned like a fresh allocation (pointer
alignment chooses kernel routes: the row-contiguous epilogue, the persistent GEMM, the sub-pixel conv) and filled with POISON: a
quiet-NaN bit pattern no arithmetic produces for the floating-point formats (local_error.check turns a non-finite element into an
infinite error), GUARD_BYTE bytes for the integer ones.  ``init=``: the payload starts as a copy of that tensor instead (in-place
residuals, scatter outputs whose untouched elements a test asserts itself).

``Pool`` keeps the guarded buffers of one test: ``out = pool(M, N, dtype=...)`` hands out the payload view, ``pool.check(name)``
asserts the guards of all of them (and that no poison is left) and lets them go.

Imports torch only; any device (the CPU tests of this module run the same code)."""
import torch

GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
ALIGN = 256
# dtype -> (integer view of the same width, poison pattern).  Quiet NaNs with GUARD_BYTE in the payload bits: never the canonical
# NaN (0x7fc0 / 0x7e00 / 0x7fc00000 / 0x7ff8000000000000) that arithmetic on the device or in torch produces.
POISON = {
    torch.bfloat16: (torch.int16, 0x7FE5),
    torch.float16: (torch.int16, 0x7EA5),
    torch.float32: (torch.int32, 0x7FC0A5A5),
    torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    """the tensor's elements as integers of the same width (floating-point formats; integers pass through)"""
    return t.view(POISON[t.dtype][0]) if t.dtype in POISON else t


class Guarded:
    def __init__(self, shape, dtype, device="cuda", init=None):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        self.dtype, self.shape = dtype, shape
        self.nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.empty(GUARD_BYTES + ALIGN + self.nbytes + GUARD_BYTES, dtype=torch.uint8, device=device)
        self.buf.fill_(GUARD_BYTE)
        # payload offset: the first 256-byte aligned address that leaves room for the front guard (GUARD_BYTES itself on an
        # allocator that aligns its blocks)
        self.off = GUARD_BYTES + (-(self.buf.data_ptr() + GUARD_BYTES)) % ALIGN
        self.t = self.buf[self.off:self.off + self.nbytes].view(dtype).view(shape)
        assert self.t.is_contiguous() and (numel == 0 or self.t.data_ptr() % ALIGN == 0)
        if init is not None:
            if init.dtype != dtype or tuple(init.shape) != shape:
                raise ValueError(f"init must be {dtype} {shape}, got {init.dtype} {tuple(init.shape)}")
            self.t.copy_(init)
        elif dtype in POISON:
            _bits(self.t).fill_(POISON[dtype][1])
        # (integer formats: the payload already holds GUARD_BYTE bytes)

    def _guards(self):
        front = self.buf[self.off - GUARD_BYTES:self.off]
        rear = self.buf[self.off + self.nbytes:self.off + self.nbytes + GUARD_BYTES]
        return front, rear

    def assert_guards(self, name="output"):
        """Both guards bit-unchanged; a failure says how many bytes changed and where the first one lies relative to the payload."""
        front, rear = self._guards()
        bad_f, bad_r = front != GUARD_BYTE, rear != GUARD_BYTE
        n = int(bad_f.sum()) + int(bad_r.sum())
        if n == 0:
            return
        if bool(bad_f.any()):
            first = int(bad_f.nonzero()[0]) - GUARD_BYTES
        else:
            first = self.nbytes + int(bad_r.nonzero()[0])
        raise AssertionError(
            f"{name}: the launch wrote outside its output {self.shape} {self.dtype}: {n} guard bytes changed "
            f"({int(bad_f.sum())} in front, {int(bad_r.sum())} behind), the first at byte {first} relative to the payload's first byte "
            f"(payload: {self.nbytes} bytes; element {first // max(self.t.element_size(), 1)})")

    def poisoned(self):
        """bool tensor: the elements that still hold the poison pattern (bit comparison: a computed NaN does not count)"""
        if self.dtype in POISON:
            return _bits(self.t) == POISON[self.dtype][1]
        width = self.t.element_size()
        pat = int.from_bytes(bytes([GUARD_BYTE] * width), "little", signed=width > 1)
        return self.t.view(_INT_VIEW[width]) == pat

    def assert_written(self, name="output", mask=None):
        """No poison left in the payload (or in ``mask``, a bool tensor of the payload's shape)."""
        left = self.poisoned()
        if mask is not None:
            left = left & mask
        n = int(left.sum())
        if n:
            idx = tuple(int(i) for i in left.nonzero()[0])
            flat = int(left.reshape(-1).nonzero()[0])
            raise AssertionError(f"{name}: {n} of {left.numel()} elements of the output {self.shape} {self.dtype} were never written; "
                                 f"the first at {idx} (flat index {flat}, mod 256: {flat % 256}, mod 8: {flat % 8})")


def guarded(shape, dtype, device="cuda", init=None):
    """-> Guarded: ``.t`` the contiguous payload view, ``.assert_guards(name)``, ``.assert_written(name, mask=None)``."""
    return Guarded(shape, dtype, device, init)


class Pool:
    """The guarded outputs of one test."""

    def __init__(self, device="cuda"):
        self.device, self.live = device, []

    def __call__(self, *shape, dtype, init=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        g = guarded(shape, dtype, self.device, init)
        self.live.append(g)
        return g.t

    def like(self, t, init=None):
        return self(tuple(t.shape), dtype=t.dtype, init=init)

    def check(self, name="output", written=True):
        """assert_guards (and, with ``written``, assert_written) on every buffer handed out since the last check; then let them go.
        Buffers made with ``init=`` hold no poison, so ``written`` says nothing about them: what a partial launch must leave alone
        is the test's own assertion."""
        live, self.live = self.live, []
        for i, g in enumerate(live):
            g.assert_guards(f"{name} [buffer {i}]")
            if written:
                g.assert_written(f"{name} [buffer {i}]")
