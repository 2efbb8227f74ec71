"""Guard bands for the memory contract of include/sot_hip.h (tests/test_memory_contract_gpu.py; the helper's own test: tests/test_guarded.py).

A tensor from torch.empty cannot show a stray store: the caching allocator rounds every request up and serves it from a larger pool, so a
store one element past an output lands in slack or in another tensor.  guarded() makes ONE flat allocation, fills ALL of it with a fixed
32-bit pattern and hands out a view in its middle:

    | band before | view: row 0 | gap | row 1 | gap | ... | row B-1 | band after |

The bands are at least 64 KiB AND at least 8 rows wide on each side, so a store to "row B", "row B + ROWS - 1" or "one vector past the end"
lands inside them; the gaps (row_stride > row length) hold the pattern too.  The handle remembers which bytes belong to the view:

    assert_untouched()      every byte outside the view still holds the pattern (bands and gaps), compared on the device as integers;
    assert_fully_written()  no 32-bit word of the pattern is left inside the view: an early return cannot pass the guard check by doing nothing;
    assert_unchanged()      the whole allocation, view included, equals the snapshot taken by snapshot(): inputs are const.

The output pattern is a quiet NaN with a payload, 0x7FC0DEAD: no kernel result has these bits (an arithmetic NaN is 0x7FC00000 or 0xFFC00000,
an index of 0x7FC0DEAD or a uint16 pair (0xDEAD, 0x7FC0) is outside every row).  Inputs come in two fills, zeros and the poison NaN
(poisoned_pair): a result that depends on bytes outside its rows differs between the two.
"""
import math

import torch

POISON = 0x7FC0DEAD          # quiet NaN, payload 0xDEAD; as int32 it is positive
MIN_BAND = 64 * 1024         # bytes of guard on each side, at least
MIN_BAND_ROWS = 8            # ... and at least this many rows of the tensor
BASE_ALIGN = 256             # the allocation's first byte; the view sits at BASE_ALIGN * k + offset_bytes
FILLS = {"poison": POISON, "zeros": 0}


class GuardError(AssertionError):
    """region: "before", "gap after row r", "after" or "view"; first / last: offending byte offsets relative to the view's first byte"""

    def __init__(self, what, region, first, last):
        super().__init__(f"{what}: region '{region}', bytes {first} .. {last} relative to the view's first byte")
        self.region, self.first, self.last = region, first, last


def _round_up(v, a):
    return (v + a - 1) // a * a


def _pattern_bytes(pattern, lo, hi, device):
    """the bytes [lo, hi) of an allocation filled with the little-endian 32-bit `pattern` from its first byte"""
    quad = torch.tensor([(pattern >> (8 * k)) & 0xFF for k in range(4)], dtype=torch.uint8, device=device)
    return quad[torch.arange(lo, hi, device=device) & 3]


class Guard:
    def __init__(self, flat, start, rows, row_bytes, stride_bytes, pattern, name):
        self.flat = flat                  # uint8, the whole allocation, first byte on a BASE_ALIGN boundary, a multiple of 4 bytes long
        self.start = start                # byte index of the view's first byte in flat
        self.rows, self.row_bytes, self.stride_bytes = rows, row_bytes, stride_bytes
        self.pattern = pattern
        self.name = name
        self.saved = None

    @property
    def end(self):
        """byte index in flat just past the view's last byte"""
        return self.start + ((self.rows - 1) * self.stride_bytes + self.row_bytes if self.rows > 0 else 0)

    def _check(self, lo, hi, region_of):
        if hi <= lo:
            return
        bad = torch.nonzero(self.flat[lo:hi] != _pattern_bytes(self.pattern, lo, hi, self.flat.device)).flatten()
        if bad.numel():
            first, last = int(bad[0]) + lo, int(bad[-1]) + lo
            raise GuardError(f"{self.name}: bytes outside the view were written", region_of(first), first - self.start, last - self.start)

    def assert_untouched(self):
        self._check(0, self.start, lambda at: "before")
        if self.rows > 1 and self.stride_bytes > self.row_bytes:     # the gaps, as one [rows - 1, gap] comparison
            gap = self.stride_bytes - self.row_bytes
            dev = self.flat.device
            at = (self.start + self.row_bytes + torch.arange(self.rows - 1, device=dev)[:, None] * self.stride_bytes + torch.arange(gap, device=dev)[None, :])
            quad = torch.tensor([(self.pattern >> (8 * k)) & 0xFF for k in range(4)], dtype=torch.uint8, device=dev)
            bad = torch.nonzero((self.flat[at.flatten()] != quad[at.flatten() & 3])).flatten()
            if bad.numel():
                first, last = int(at.flatten()[bad[0]]), int(at.flatten()[bad[-1]])
                row = (first - self.start) // self.stride_bytes
                raise GuardError(f"{self.name}: bytes outside the view were written", f"gap after row {row}", first - self.start, last - self.start)
        self._check(self.end, self.flat.numel(), lambda at: "after")

    def assert_fully_written(self):
        """no aligned 32-bit word that lies wholly inside a row of the view still holds the pattern"""
        hits = torch.nonzero(self.flat.view(torch.int32) == self.pattern).flatten() * 4 - self.start     # byte offsets relative to the view
        if self.rows > 0:
            row = torch.div(hits, self.stride_bytes, rounding_mode="floor")
            col = hits - row * self.stride_bytes
            hits = hits[(hits >= 0) & (row < self.rows) & (col + 4 <= self.row_bytes)]
        else:
            hits = hits[:0]
        if hits.numel():
            raise GuardError(f"{self.name}: {hits.numel()} words of the view were never written", "view", int(hits[0]), int(hits[-1]) + 3)

    def snapshot(self):
        self.saved = self.flat.clone()
        return self

    def assert_unchanged(self):
        assert self.saved is not None, "snapshot() first"
        bad = torch.nonzero(self.flat != self.saved).flatten()
        if bad.numel():
            first, last = int(bad[0]), int(bad[-1])
            region = "before" if first < self.start else "after" if first >= self.end else "view or gap"
            raise GuardError(f"{self.name}: a const input was modified", region, first - self.start, last - self.start)


def guarded(shape, dtype, device, *, row_stride=None, offset_bytes=0, fill="poison", name="buffer"):
    """(view, Guard).  shape: any; the last dimension is the row.  row_stride (elements, 2-D shapes only): rows that far apart, the gaps
    filled like the bands.  offset_bytes: the view's first byte sits that far past a 256-byte boundary (a multiple of the element size)."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    item = torch.empty((), dtype=dtype).element_size()
    assert offset_bytes % item == 0 and 0 <= offset_bytes < BASE_ALIGN, (offset_bytes, item)
    row_len = shape[-1] if shape else 1
    rows = math.prod(shape[:-1]) if shape else 1
    if row_len == 0:
        rows = 0
    stride = row_len if row_stride is None else int(row_stride)
    assert stride >= row_len and (row_stride is None or len(shape) == 2), (shape, row_stride)
    row_bytes, stride_bytes = row_len * item, max(stride * item, item)
    band = _round_up(max(MIN_BAND, MIN_BAND_ROWS * stride_bytes), BASE_ALIGN)
    body = (rows - 1) * stride_bytes + row_bytes if rows > 0 else 0
    total = _round_up(band + offset_bytes + body + band, BASE_ALIGN)
    raw = torch.empty(total + BASE_ALIGN, dtype=torch.uint8, device=device)
    lead = (-raw.data_ptr()) % BASE_ALIGN
    flat = raw[lead:lead + total]
    pattern = FILLS[fill] if isinstance(fill, str) else int(fill)
    flat.view(torch.int32).fill_(pattern)
    start = band + offset_bytes
    if rows > 0:
        typed = flat[start:start + body].view(dtype)
        view = typed.as_strided((rows, row_len), (stride, 1)) if row_stride is not None else typed.view(shape)
    else:
        view = flat[start:start].view(dtype).view(shape)
    g = Guard(flat, start, rows, row_bytes, stride_bytes, pattern, name)
    assert rows == 0 or view.data_ptr() == flat.data_ptr() + start
    assert (flat.data_ptr() + start) % BASE_ALIGN == offset_bytes
    return view, g


def workspace(nbytes, align, device, *, name="workspace"):
    """(uint8 view of exactly `nbytes` bytes, Guard): the first byte at `align` bytes and no better (256: a 256-byte boundary), guard bands
    on both sides -- assert_untouched() proves that a call stayed inside the size its own size function reported."""
    assert align in (1, 2, 4, 8, 16, 32, 64, 128, 256)
    return guarded((int(nbytes),), torch.uint8, device, offset_bytes=align % BASE_ALIGN, name=name)


def ptr(view, guard):
    """the device address of the view's first byte, also for an empty view (where torch's data_ptr() is 0)"""
    return guard.flat.data_ptr() + guard.start


def poisoned_pair(tensor, *, row_stride=None, offset_bytes=0, name="input"):
    """The same values in two layouts that differ only in what the padding holds -- the gaps between rows and the bands before row 0 and
    after row B - 1: ((view, Guard) over zeros, (view, Guard) over the poison NaN), both with a snapshot taken."""
    out = []
    for fill in ("zeros", "poison"):
        view, g = guarded(tensor.shape, tensor.dtype, tensor.device, row_stride=row_stride, offset_bytes=offset_bytes, fill=fill, name=f"{name} ({fill})")
        view.copy_(tensor)
        out.append((view, g.snapshot()))
    return tuple(out)
