"""TEST HELPER for the far-buffer tests (tests/test_gpu_far_strides.py, tests/test_gpu_beyond_4gib.py): buffers whose elements lie
2^32 bytes and more behind the pointer an entry is given, and the comparisons that run where the buffers are.

A truncated offset (a 32-bit product, a narrowed offsets[i]) does not fault in these tests: every buffer is ONE allocation that
covers everything from the pointer handed to the entry to the last element, byte buffers with 2 GiB in front of that pointer as
well (a sign-extended 32-bit offset), all of it filled with a sentinel. The element a wrapped write hits is then the test's own,
and the comparison finds it: the footprint that should hold it still holds the sentinel, and the place it went to does not.

    check_footprints   every footprint (a slot, a row, a clip's channel) equals its expectation; then the footprints are wiped
                       and every byte of the allocation must be the sentinel, checked in chunks of 256 MiB
    check_cycled       a dense [n, row] body whose rows cycle with an odd period equals the period, row by row, in chunks

Both name the rows that differ, so that a row that moved is reported by its index. Nothing here imports torch at module level;
every function takes the module, and all of them work on CPU tensors too: tests/test_far_buffers.py re-places expectations with
offsets truncated at a scaled-down line (2^16 elements) and checks that the moved rows are the ones reported."""
import time

import pytest

LINE = 1 << 32          # bytes
BYTE_LEAD = 1 << 31     # bytes in front of the pointer handed to an entry, in byte buffers
CHUNK = 1 << 28         # bytes compared at a time: temporaries of a comparison stay below 1 GiB
PERIODS = (7, 35, 1031, 4099)


def _need_gb(torch, gb):
    free, _ = torch.cuda.mem_get_info()
    if free < gb * (1 << 30):
        pytest.skip("needs %d GB of device memory, %.1f free" % (gb, free / (1 << 30)))


class Meter:
    """Wall time and peak device memory of a test as the mem_get_info delta (the library's allocations are not torch's): mark()
    at the points where the most is held, report() prints one line."""

    def __init__(self, torch, name):
        self.torch, self.name = torch, name
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        self.t0 = time.time()
        self.free0 = self.low = torch.cuda.mem_get_info()[0]

    def mark(self):
        self.low = min(self.low, self.torch.cuda.mem_get_info()[0])

    def report(self):
        self.torch.cuda.synchronize()
        self.mark()
        print("far-buffer meter: %s: %.1f s, peak %.2f GiB of device memory (%.1f GiB free at its start)" %
              (self.name, time.time() - self.t0, (self.free0 - self.low) / 2.0 ** 30, self.free0 / 2.0 ** 30))


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def slot_stride(line=LINE, slots_below=128):
    """The output stride (a multiple of 16) that makes slot `slots_below` begin 16 * slots_below bytes below the line:
    2^25 - 16 for the line 2^32 and 128 slots below it, so a slot of more than 2 048 bytes straddles the line."""
    return line // slots_below - 16


def sides(offs, lens, itemsize=1, line=LINE):
    """-> (footprints wholly below the line, footprints that straddle it, footprints wholly at or beyond it); offs and lens
    in elements of itemsize bytes, counted from the pointer handed to the entry"""
    below = straddle = beyond = 0
    for o, n in zip(offs, lens):
        if n <= 0:
            continue
        lo, hi = o * itemsize, (o + n) * itemsize
        if hi <= line:
            below += 1
        elif lo >= line:
            beyond += 1
        else:
            straddle += 1
    return below, straddle, beyond


def assert_crosses(offs, lens, itemsize=1, line=LINE, straddle=True, what=""):
    """The run has footprints on both sides of the line and, where asked, one that straddles it."""
    below, on, beyond = sides(offs, lens, itemsize, line)
    assert below > 0 and beyond + on > 0, "%s: nothing on one side of the line (%d below, %d across, %d beyond)" % (what, below, on, beyond)
    assert on > 0 or not straddle, "%s: no footprint straddles the line (%d below, %d beyond)" % (what, below, beyond)
    return below, on, beyond


def truncated(offs, itemsize=1, line=LINE):
    """The element offsets a 32-bit byte offset would give: (o * itemsize mod line) / itemsize"""
    return [((o * itemsize) % line) // itemsize for o in offs]


# ---- buffers ------------------------------------------------------------------------------------------------------------------
class Far:
    """One flat allocation of lead + span elements of dtype filled with `fill`; the entry gets ptr(), element `lead`."""

    def __init__(self, torch, dtype, span, fill, lead=0, device="cuda:0"):
        self.torch, self.fill, self.lead, self.span = torch, fill, lead, span
        self.t = torch.full((lead + span,), fill, dtype=dtype, device=device)
        self.itemsize = self.t.element_size()

    def ptr(self, off=0):
        return self.t.data_ptr() + (self.lead + off) * self.itemsize

    def refill(self):
        self.t.fill_(self.fill)

    def at(self, off, n):
        """the elements [off, off + n) behind the pointer handed to the entry"""
        return self.t[self.lead + off:self.lead + off + n]

    def rows(self, shape, strides, off=0):
        """an as_strided view whose element 0 is `off` elements behind the pointer handed to the entry"""
        return self.t.as_strided(shape, strides, self.lead + off)

    def place(self, off, values):
        self.at(off, values.numel()).copy_(values)


def first_not(torch, t, fill, chunk_bytes=CHUNK):
    """The index of the first element of the flat tensor t that is not `fill`, or -1; compared in chunks"""
    step = max(1, chunk_bytes // t.element_size())
    flags = [(t[a:a + step] != fill).any() for a in range(0, t.numel(), step)]
    if not flags:
        return -1
    flags = torch.stack(flags).cpu().tolist()
    for k, f in enumerate(flags):
        if f:
            c = t[k * step:(k + 1) * step]
            return k * step + int(torch.nonzero(c != fill)[0].item())
    return -1


def check_footprints(torch, far, rows, what, unit="slot"):
    """rows: (name, offset, want, wipe) per footprint, offsets in elements behind the pointer handed to the entry: want (a 1-D
    tensor where far lives, or None for contents that are unspecified) is what [offset, offset + len(want)) must hold; wipe >=
    len(want) elements from offset on are the footprint's. Every footprint is compared, ALL that differ are named; then
    the footprints are wiped and every element of the allocation, the lead included, must be the sentinel. The buffer is left
    filled with the sentinel."""
    bad = []
    for name, off, want, wipe in rows:
        if want is not None and want.numel():
            assert wipe >= want.numel()
            if not torch.equal(far.at(off, want.numel()), want):
                bad.append(name)
    assert not bad, "%s: %d %ss differ from the expectation: %s" % (what, len(bad), unit, bad)
    for name, off, want, wipe in rows:
        if wipe:
            far.at(off, wipe).fill_(far.fill)
    at = first_not(torch, far.t, far.fill)
    if at >= 0:
        rel = at - far.lead
        near = min(rows, key=lambda r: abs(r[1] - rel)) if rows else None
        raise AssertionError("%s: element %d behind the base (byte %d) is written outside every %s (nearest: %s %s at %d)" %
                             (what, rel, rel * far.itemsize, unit, unit, near and near[0], near[1] if near else 0))


def check_strided(torch, far, stride, want, what, unit="slot"):
    """check_footprints for many footprints of one length at one stride: footprint i is [i * stride, i * stride + want.shape[1])
    and must equal want[i] (a 2-D tensor where far lives, holding the sentinel where nothing is to be written); gathered with
    one as_strided view. All rows that differ are named, then the rest of the allocation must be the sentinel."""
    n, length = want.shape
    got = far.rows((n, length), (stride, 1))
    bad = torch.nonzero((got != want).any(dim=1)).flatten().tolist()
    assert not bad, "%s: %d %ss differ from the expectation: %s" % (what, len(bad), unit, bad[:4] + bad[4:][-8:])
    got.fill_(far.fill)
    at = first_not(torch, far.t, far.fill)
    assert at < 0, "%s: element %d behind the base is written outside every %s (%s %d begins at %d)" % (
        what, at - far.lead, unit, unit, (at - far.lead) // stride, (at - far.lead) // stride * stride)


def check_cycled(torch, body, period, what, unit="slot", chunk_bytes=CHUNK):
    """body [n, row] (a view, on the device) must be period [P, row] over and over, the last cycle cut short; compared in
    chunks of whole cycles (at least one) of about chunk_bytes. Names the first rows that differ."""
    n, row = body.shape
    P = period.shape[0]
    assert period.shape[1] == row
    k = max(1, chunk_bytes // (P * row * body.element_size()))
    bad, count = [], 0
    for a in range(0, n, k * P):
        m = min(k * P, n - a)
        full = m // P
        found = []
        if full:
            d = (body[a:a + full * P].view(full, P, row) != period).any(dim=2)
            if bool(d.any()):
                found += (a + torch.nonzero(d.flatten()).flatten()).tolist()
        rest = m - full * P
        if rest:
            d = (body[a + full * P:a + m] != period[:rest]).any(dim=1)
            if bool(d.any()):
                found += (a + full * P + torch.nonzero(d).flatten()).tolist()
        count += len(found)
        bad = (bad + found)[:4] + (bad + found)[4:][-4:]
    assert not bad, "%s: %d %ss differ from the cycle of %d, the first and last of them %s (their classes: %s)" % (
        what, count, unit, P, bad, [b % P for b in bad])


def assert_fill(torch, t, fill, what):
    at = first_not(torch, t, fill)
    assert at < 0, "%s: element %d is not the sentinel" % (what, at)
