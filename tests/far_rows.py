"""Rows past 2^31 elements and 2^32 bytes from their base pointer, for tests/test_far_offsets_gpu.py (the helper's own test: tests/test_far_rows.py).

The kernels form a row's address as base + row * stride in 64 bits.  A [B, n] tensor whose rows lie a few elements apart cannot show a
dropped cast: every offset fits 31 bits.  Far.place() puts a [3, n] view inside ONE flat arena so that those of rows 1 and 2 do not:

    arena element   0 ........ | 2^31 ......... | 2^31 + 2^30 + 4 ... | 2^32 + 8 ........ | end
                    low region   row 0 of every    row 1 of every        row 2 of every
                    (poison)     view (region 0)   view (region 1)       view (region 2)

    FIRST  = 2^31          arena element of the first view's first element
    STRIDE = 2^30 + 4      elements between rows: a multiple of 4, so rows that start 16-byte aligned stay so and the launch layer's
                           vector test (base and stride) picks the same kernel as for dense rows
    row 1 starts 2^32 + 16 bytes, row 2 starts 2^31 + 8 elements = 2^33 + 32 bytes from the view's base
    the arena holds 2^32 + 8 + SLOTS * SLOT + BAND elements (about 16 GiB); torch.empty, NEVER filled as a whole

Several tensors of one call (x, y, per-row positions, ...) are views of the same arena: view k starts SLOT elements after view k - 1, so
the rows r of all views lie side by side in region r, about 2 MiB that is filled with the poison of tests/guarded.py (0x7FC0DEAD, a quiet
NaN with a payload) before the rows are written.  The low region, where wrapped offsets land, is poison too.

What a 32-bit reading of a row's offset does (misreadings(): element offset and byte offset, each truncated to 32 bits and taken as signed
and as unsigned; a reading that equals the true offset is none):

    row 1   the byte offset 2^32 + 16 wraps to 16 bytes: the row is read from 4 elements past the view's base;
    row 2   the element offset 2^31 + 8 read as signed is 8 - 2^31: arena element 8 + k SLOT of view k, in the low region;
            the byte offset 2^33 + 32 wraps to 32 bytes: 8 elements past the view's base.

Every landing point is inside the arena, so a wrong kernel reads wrong data but does not fault.  The signed landing is inside a poison band
and outside every true row.  The byte wraps land INSIDE row 0 of the same view (4 and 8 elements past its first element cannot be anywhere
else): there the misread row [landing, landing + n) runs 4 or 8 elements past the end of row 0 into the poison behind it, and all it holds
before that is row 0's data displaced.  Either way a kernel that reads a misread row whole meets the poison NaN, and one that reads only
part of it returns row 0's values for row 1 or 2 -- the test compares bit for bit with the same call on a dense copy, whose rows differ.

Far.snapshot() copies the four regions (not the arena); Far.assert_unchanged() compares them bit for bit afterwards: the bands hold the
poison and the rows their values -- inputs are const.  The arithmetic lives in Layout, plain integers, so that tests/test_far_rows.py proves
the properties above without a GPU, and exercises Far itself on a layout scaled down to a few KiB.
"""
import collections

import torch

from guarded import POISON

FIRST = 2 ** 31
STRIDE = 2 ** 30 + 4
ROWS = 3
SLOT = 65536          # elements between the bases of two co-located views: the longest row (audio clips) plus its share of poison
SLOTS = 8
BAND = 4096           # elements of poison before the first and after the last slot of a region (16 KiB)
ITEM = 4              # float32 / int32 elements throughout

Misreading = collections.namedtuple("Misreading", "what offset")     # offset: elements relative to the view's base


class Layout:
    """Integer arithmetic of the arena: where views, rows, poison regions and the 32-bit misreadings of row offsets lie (all in elements)."""

    def __init__(self, first=FIRST, stride=STRIDE, rows=ROWS, slot=SLOT, slots=SLOTS, band=BAND, wrap_bits=32):
        self.first, self.stride, self.rows, self.slot, self.slots, self.band, self.wrap_bits = first, stride, rows, slot, slots, band, wrap_bits
        assert band <= first - slots * slot - band, "the low region must end before region 0 begins"
        assert slots * slot + 2 * band <= stride, "regions must not meet"

    @property
    def total(self):
        """elements of the arena"""
        return self.first + (self.rows - 1) * self.stride + self.slots * self.slot + self.band

    def base(self, k):
        """arena element of view k's first element"""
        assert 0 <= k < self.slots
        return self.first + k * self.slot

    def row_start(self, k, r):
        return self.base(k) + r * self.stride

    def regions(self):
        """[(lo, hi)] arena elements that hold poison wherever no row lies: the low region, then one region per row index"""
        width = self.slots * self.slot
        out = [(0, width + self.band)]
        out += [(self.first + r * self.stride - self.band, self.first + r * self.stride + width + self.band) for r in range(self.rows)]
        return out

    def in_region(self, e):
        return any(lo <= e < hi for lo, hi in self.regions())

    def misreadings(self, r):
        """the 32-bit readings of row r's offset that differ from the truth, as element offsets from the view's base"""
        true = r * self.stride
        bits = self.wrap_bits

        def wrap(v, signed):
            v &= (1 << bits) - 1
            return v - (1 << bits) if signed and v >= 1 << (bits - 1) else v
        out = []
        for signed in (True, False):
            sign = "signed" if signed else "unsigned"
            e = wrap(true, signed)
            if e != true:
                out.append(Misreading(f"element offset as {sign} {bits}-bit", e))
            b = wrap(true * ITEM, signed)
            assert b % ITEM == 0
            if b != true * ITEM:
                out.append(Misreading(f"byte offset as {sign} {bits}-bit", b // ITEM))
        return out


class Far:
    """One arena on `device` and the views placed in it.  place(k, t) writes the [rows, n] tensor t as view k and returns the strided view."""

    def __init__(self, device, layout=None, dtype=torch.float32):
        self.layout = layout or Layout()
        assert torch.empty((), dtype=dtype).element_size() == ITEM
        self.arena = torch.empty(self.layout.total, dtype=dtype, device=device)      # never filled as a whole
        self.words = self.arena.view(torch.int32)
        self.live = {}          # k -> n
        self.saved = None
        self.clear()

    @staticmethod
    def bytes_needed(layout=None):
        return (layout or Layout()).total * ITEM

    def clear(self):
        """poison in every region; no view is live"""
        for lo, hi in self.layout.regions():
            self.words[lo:hi].fill_(POISON)
        self.live, self.saved = {}, None

    def place(self, k, t):
        L = self.layout
        assert t.ndim == 2 and t.shape[0] == L.rows and 0 < t.shape[1] <= L.slot - 16, tuple(t.shape)
        assert k not in self.live, f"slot {k} is taken"
        n = t.shape[1]
        src = t.contiguous()
        if src.dtype != self.arena.dtype:
            assert src.element_size() == ITEM
            src = src.view(self.arena.dtype)
        for r in range(L.rows):                                  # plain contiguous copies: no strided copy kernel is trusted with these offsets
            at = L.row_start(k, r)
            self.arena[at:at + n].copy_(src[r])
        self.live[k] = n
        view = self.arena.as_strided((L.rows, n), (L.stride, 1), L.base(k))
        assert view.data_ptr() == self.arena.data_ptr() + L.base(k) * ITEM
        return view if t.dtype == self.arena.dtype else view.view(t.dtype)

    def rows_of(self, k):
        """the rows of view k as a dense copy, read back through contiguous slices"""
        L, n = self.layout, self.live[k]
        return torch.stack([self.arena[L.row_start(k, r):L.row_start(k, r) + n].clone() for r in range(L.rows)])

    def snapshot(self):
        self.saved = [self.words[lo:hi].clone() for lo, hi in self.layout.regions()]
        return self

    def assert_unchanged(self):
        """every region equals its snapshot bit for bit: the poison is untouched and the rows, const inputs, hold their values"""
        assert self.saved is not None, "snapshot() first"
        for (lo, hi), was in zip(self.layout.regions(), self.saved):
            bad = torch.nonzero(self.words[lo:hi] != was).flatten()
            if bad.numel():
                raise AssertionError(f"far arena: {bad.numel()} words changed, arena elements {lo + int(bad[0])} .. {lo + int(bad[-1])}")

    def assert_poison_outside_rows(self):
        """every word of every region that belongs to no live row is the poison"""
        L = self.layout
        for lo, hi in L.regions():
            is_row = torch.zeros(hi - lo, dtype=torch.bool, device=self.arena.device)
            for k, n in self.live.items():
                for r in range(L.rows):
                    at = L.row_start(k, r)
                    if lo <= at < hi:
                        is_row[at - lo:at - lo + n] = True
            bad = torch.nonzero((self.words[lo:hi] != POISON) & ~is_row).flatten()
            if bad.numel():
                raise AssertionError(f"far arena: {bad.numel()} poison words overwritten, arena elements {lo + int(bad[0])} .. {lo + int(bad[-1])}")
