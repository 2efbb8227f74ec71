"""tests/far_rows.py without a GPU: the layout in integers, and the Far class itself on a layout scaled down to a few KiB (offsets wrap at 10
bits there as they do at 32 in the real one).

No deliberately wrong kernel is run on a GPU to show that tests/test_far_offsets_gpu.py catches it; this file is that evidence: every 32-bit
reading of every row offset lands where the poison, or another row's data, is.
"""
import pytest
import torch

import far_rows as fr
from guarded import POISON

REAL = fr.Layout()
SMALL = fr.Layout(first=2 ** 9, stride=2 ** 8 + 4, slot=32, slots=4, band=8, wrap_bits=10)     # rows 1, 2 at 2^10 + 16 bytes, 2^9 + 8 elements
LENGTHS = (1, 3, 257, 300, 411, 700, 1025, 1500, 2048, 4173, fr.SLOT - 16)


def true_rows(L, lengths):
    """[(lo, hi)] of every row of every co-located view; lengths: n of view k"""
    return [(L.row_start(k, r), L.row_start(k, r) + n) for k, n in enumerate(lengths) for r in range(L.rows)]


def test_the_sizes_the_layout_promises():
    assert REAL.first == 2 ** 31 and REAL.stride == 2 ** 30 + 4 and REAL.rows == 3
    assert REAL.stride * fr.ITEM == 2 ** 32 + 16 and 2 * REAL.stride == 2 ** 31 + 8
    assert REAL.total == 2 ** 32 + 8 + fr.SLOTS * fr.SLOT + fr.BAND
    assert 16 * 2 ** 30 < fr.Far.bytes_needed() < 16 * 2 ** 30 + 4 * 2 ** 20          # about 16 GiB
    assert sum(hi - lo for lo, hi in REAL.regions()) * fr.ITEM < 16 * 2 ** 20      # what is ever filled or compared: under 16 MiB


def test_stride_and_rows_keep_the_alignment_of_dense_rows():
    assert REAL.stride % 4 == 0 and fr.SLOT % 4 == 0 and REAL.first % 4 == 0
    for k in range(REAL.slots):
        for r in range(REAL.rows):
            assert REAL.row_start(k, r) * fr.ITEM % 16 == 0       # relative to the arena, which the allocator aligns to 256 bytes or better


def test_regions_are_disjoint_ordered_and_inside_the_arena():
    regs = REAL.regions()
    assert len(regs) == 1 + REAL.rows and regs[0][0] == 0 and regs[-1][1] == REAL.total
    for (lo, hi), (lo2, hi2) in zip(regs, regs[1:]):
        assert lo < hi <= lo2 < hi2


@pytest.mark.parametrize("n", LENGTHS)
def test_true_rows_of_co_located_views_do_not_overlap_and_are_banded(n):
    rows = sorted(true_rows(REAL, [n] * REAL.slots))
    for (lo, hi), (lo2, hi2) in zip(rows, rows[1:]):
        assert hi < lo2, "two rows meet"                         # at least one poison word between any two rows ...
    for lo, hi in rows:
        assert hi - lo == n and REAL.in_region(lo - 1) and REAL.in_region(hi) and REAL.in_region(lo) and REAL.in_region(hi - 1)
        assert not any(a <= lo - 1 < b or a <= hi < b for a, b in rows)          # ... and poison just before and just after each


def test_every_far_row_has_a_misreading_and_row_0_has_none():
    assert REAL.misreadings(0) == []
    got = {r: sorted((m.what, m.offset) for m in REAL.misreadings(r)) for r in (1, 2)}
    assert got[1] == [("byte offset as signed 32-bit", 4), ("byte offset as unsigned 32-bit", 4)]
    assert got[2] == [("byte offset as signed 32-bit", 8), ("byte offset as unsigned 32-bit", 8), ("element offset as signed 32-bit", 8 - 2 ** 31)]
    # (rows 1 and 2 as UNSIGNED element offsets, 2^30 + 4 and 2^31 + 8, fit 32 bits: that reading is right, and no layout of three rows in 16 GiB
    # makes it wrong; what it guards against is the signed one)


@pytest.mark.parametrize("n", LENGTHS)
def test_every_misreading_lands_inside_the_arena_on_poison_or_on_another_rows_data(n):
    rows = true_rows(REAL, [n] * REAL.slots)
    for k in range(REAL.slots):
        for r in range(REAL.rows):
            for m in REAL.misreadings(r):
                land = REAL.base(k) + m.offset
                assert 0 <= land and land + n <= REAL.total, (k, r, m)                         # the whole misread row: no fault
                assert REAL.in_region(land) and REAL.in_region(land + n - 1), (k, r, m)          # ... and inside what the helper fills
                assert land != REAL.row_start(k, r)
                inside = [(lo, hi) for lo, hi in rows if lo <= land < hi]
                if "element" in m.what:
                    assert not inside, (k, r, m, "the landing element must be poison")
                    assert all(hi <= land or land + n <= lo for lo, hi in rows), "the whole misread row is poison"
                else:
                    # the byte wraps: 4 and 8 elements past the view's own base, i.e. inside its row 0 unless the row is that short
                    row0 = (REAL.row_start(k, 0), REAL.row_start(k, 0) + n)
                    assert inside == ([row0] if m.offset < n else []), (k, r, m)
                    tail = range(max(land, row0[1]), land + n)      # the part of the misread row behind row 0: poison, at least one word
                    assert len(tail) == min(m.offset, n) and all(not any(lo <= e < hi for lo, hi in rows) for e in (tail[0], tail[-1])), (k, r, m)


def test_small_layout_wraps_like_the_real_one():
    assert SMALL.stride * fr.ITEM == 2 ** 10 + 16 and 2 * SMALL.stride == 2 ** 9 + 8
    for r in range(3):
        assert [(m.what.replace("10-bit", "32-bit"), m.offset if m.offset >= 0 else m.offset + 2 ** 9 - 2 ** 31) for m in SMALL.misreadings(r)] == \
               [(m.what, m.offset) for m in REAL.misreadings(r)]


def test_far_places_views_and_sees_a_stray_store():
    far = fr.Far("cpu", SMALL)
    assert far.arena.numel() == SMALL.total
    x = torch.arange(1, 3 * 11 + 1, dtype=torch.float32).reshape(3, 11)
    y = -torch.arange(1, 3 * 7 + 1, dtype=torch.float32).reshape(3, 7)
    idx = torch.arange(3 * 5, dtype=torch.int32).reshape(3, 5)
    vx, vy, vi = far.place(0, x), far.place(2, y), far.place(3, idx)
    assert vx.stride() == (SMALL.stride, 1) and torch.equal(vx, x) and torch.equal(vy, y) and torch.equal(vi, idx) and vi.dtype == torch.int32
    assert torch.equal(far.rows_of(0), x) and torch.equal(far.rows_of(2), y)
    assert vx.data_ptr() == far.arena.data_ptr() + SMALL.first * 4 and vy.data_ptr() == vx.data_ptr() + 2 * SMALL.slot * 4
    far.assert_poison_outside_rows()
    far.snapshot().assert_unchanged()
    # a row read through each misreading holds the poison NaN, or is the signed landing: all poison
    for r in (1, 2):
        for m in SMALL.misreadings(r):
            land = SMALL.base(0) + m.offset
            got = far.arena[land:land + 11]
            assert torch.isnan(got).any() and not torch.equal(got, x[r]), (r, m)
            assert int((far.words[land:land + 11] == POISON).sum()) == (11 if "element" in m.what else m.offset), (r, m)
    with pytest.raises(AssertionError, match="slot 2 is taken"):
        far.place(2, y)
    far.arena[SMALL.row_start(0, 1) + 11] = 0.0        # one element past a far row
    with pytest.raises(AssertionError, match="poison words overwritten"):
        far.assert_poison_outside_rows()
    with pytest.raises(AssertionError, match="1 words changed"):
        far.assert_unchanged()
    far.clear()
    far.assert_poison_outside_rows()
    far.arena[SMALL.row_start(1, 2)] = 1.0             # a const input row modified (no view is live: it is poison)
    far.snapshot()
    far.words[3] = 7                                   # the low region, where the signed reading lands
    with pytest.raises(AssertionError, match="arena elements 3 .. 3"):
        far.assert_unchanged()
