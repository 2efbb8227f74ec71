"""tests/guarded.py must be able to FAIL: one stray element is planted at each place a kernel could reach, and every assert_* has to raise
and name the right region and offset; with nothing planted it passes.  Torch indexing only, no project kernel.  The cases run here on CPU
tensors and again on the device from tests/test_memory_contract_gpu.py (check_plant(device, case))."""
import collections

import pytest
import torch

import guarded as gd

Plant = collections.namedtuple("Plant", "id shape dtype row_stride offset_bytes where region")

# where: a function of the Guard giving the byte index in the flat allocation that gets one stray byte
LAYOUTS = [
    ("f32_dense", (5, 129), torch.float32, None, 0),
    ("f32_off4", (5, 129), torch.float32, None, 4),
    ("f32_off8_strided", (5, 129), torch.float32, 132, 8),
    ("u16_odd_rows", (3, 2 * 129), torch.uint16, None, 2),
    ("u16_odd_strided", (9, 257), torch.uint16, 260, 6),
    ("i64", (3, 100), torch.int64, None, 8),
    ("f64", (1,), torch.float64, None, 8),
    ("f32_3d", (2, 3, 33), torch.float32, None, 4),
    ("i32_empty", (0, 16), torch.int32, None, 4),
]
PLACES = [
    ("last_byte_before", lambda g: g.start - 1, "before"),
    ("first_byte_after", lambda g: g.end, "after"),
    ("first_byte_of_band", lambda g: 0, "before"),
    ("last_byte_of_band", lambda g: g.flat.numel() - 1, "after"),
    ("first_byte_of_gap", lambda g: g.start + 2 * g.stride_bytes + g.row_bytes, "gap after row 2"),
    ("last_byte_of_gap", lambda g: g.start + 2 * g.stride_bytes - 1, "gap after row 1"),
]
PLANTS = [Plant(f"{lid}-{pid}", shape, dtype, stride, off, where, region)
          for lid, shape, dtype, stride, off in LAYOUTS for pid, where, region in PLACES if "gap" not in pid or stride is not None]


def check_plant(device, plant):
    view, g = gd.guarded(plant.shape, plant.dtype, device, row_stride=plant.row_stride, offset_bytes=plant.offset_bytes)
    assert tuple(view.shape) == tuple(plant.shape) and view.dtype == plant.dtype
    assert g.start >= gd.MIN_BAND and g.flat.numel() - g.end >= gd.MIN_BAND
    assert g.start >= gd.MIN_BAND_ROWS * g.stride_bytes and g.flat.numel() - g.end >= gd.MIN_BAND_ROWS * g.stride_bytes
    g.assert_untouched()                       # nothing planted
    if view.numel():
        view.copy_(torch.ones(plant.shape, dtype=torch.float32, device=device).to(plant.dtype))   # writing the whole view is allowed
        g.assert_untouched()
        g.assert_fully_written()
    at = plant.where(g)
    g.flat[at] ^= 0x01                         # one stray byte
    with pytest.raises(gd.GuardError) as err:
        g.assert_untouched()
    assert err.value.region == plant.region, (err.value.region, plant.region)
    assert err.value.first == err.value.last == at - g.start
    assert plant.region in str(err.value) and str(at - g.start) in str(err.value)


def check_unwritten_word(device):
    """an untouched word inside a "fully written" output: first, last and an interior word of a strided view; a word of the pattern in a GAP is fine"""
    for col in (0, 64, 128):
        view, g = gd.guarded((5, 129), torch.float32, device, row_stride=132, offset_bytes=4)
        with pytest.raises(gd.GuardError):
            g.assert_fully_written()           # nothing written at all: the early return
        view.fill_(1.0)
        g.assert_fully_written()
        g.assert_untouched()
        view[3, col] = torch.tensor(gd.POISON, dtype=torch.int32, device=device).view(torch.float32)
        with pytest.raises(gd.GuardError) as err:
            g.assert_fully_written()
        assert err.value.region == "view" and err.value.first == (3 * 132 + col) * 4 and err.value.last == err.value.first + 3
    # uint16 rows of odd length at a 2-byte offset: the words of the pattern's grid that lie inside a row
    view, g = gd.guarded((3, 259), torch.uint16, device, offset_bytes=2)
    view.copy_(torch.arange(3 * 259, device=device).reshape(3, 259).to(torch.uint16))
    g.assert_fully_written()
    g.flat[g.start + 2:g.start + 6] = gd._pattern_bytes(gd.POISON, g.start + 2, g.start + 6, device)
    with pytest.raises(gd.GuardError) as err:
        g.assert_fully_written()
    assert (err.value.first, err.value.last) == (2, 5)


def check_workspace(device):
    """an exact-size workspace: its last byte may be written, one byte past it may not; alignment as stated and no better"""
    for nbytes, align in ((1000, 8), (4096, 16), (12, 4), (768, 256), (0, 16)):
        ws, g = gd.workspace(nbytes, align, device)
        assert ws.numel() == nbytes and ws.dtype == torch.uint8
        addr = gd.ptr(ws, g)
        assert addr % align == 0 and (align == 256 or addr % (2 * align) != 0)
        ws.fill_(7)
        g.assert_untouched()
        g.flat[g.start + nbytes] = 7           # one byte past the reported size
        with pytest.raises(gd.GuardError) as err:
            g.assert_untouched()
        assert err.value.region == "after" and err.value.first == nbytes


def check_poisoned_pair(device):
    t = torch.rand(5, 129, device=device)
    (zv, zg), (pv, pg) = gd.poisoned_pair(t, row_stride=132, offset_bytes=4)
    assert torch.equal(zv, t) and torch.equal(pv, t) and zv.stride() == pv.stride() == (132, 1)
    assert zv.data_ptr() % 16 == pv.data_ptr() % 16 == 4
    flat = torch.as_strided(zg.flat[zg.start:].view(torch.float32), (5, 132), (132, 1))
    assert torch.all(flat[:4, 129:] == 0)
    flat = torch.as_strided(pg.flat[pg.start:].view(torch.int32), (5, 132), (132, 1))
    assert torch.all(flat[:, 129:] == gd.POISON) and torch.isnan(pg.flat[:pg.start].view(torch.float32)).all()
    for g in (zg, pg):
        g.assert_unchanged()
        g.assert_untouched()
    for g, at, region in ((zg, zg.start + 4, "view or gap"), (pg, pg.start - 1, "before"), (zg, zg.end, "after")):
        g.flat[at] ^= 0x80
        with pytest.raises(gd.GuardError) as err:
            g.assert_unchanged()
        assert err.value.region == region and err.value.first == at - g.start
        g.flat[at] ^= 0x80
        g.assert_unchanged()


@pytest.mark.parametrize("plant", PLANTS, ids=[p.id for p in PLANTS])
def test_planted_stray_byte_is_reported(plant):
    check_plant(torch.device("cpu"), plant)


def test_unwritten_word_is_reported():
    check_unwritten_word(torch.device("cpu"))


def test_workspace_is_exact():
    check_workspace(torch.device("cpu"))


def test_poisoned_pair():
    check_poisoned_pair(torch.device("cpu"))


def test_pattern_is_a_quiet_nan_no_result_has():
    v = torch.tensor([gd.POISON], dtype=torch.int32).view(torch.float32)
    assert torch.isnan(v).all()
    for made in (torch.tensor(float("nan")), torch.tensor(0.0) / torch.tensor(0.0), torch.tensor(float("inf")) - torch.tensor(float("inf"))):
        assert int(made.view(torch.int32)) != gd.POISON
    assert (gd.POISON & 0xFFFF) > 16384 and (gd.POISON >> 16) > 16384      # no uint16 permutation entry (n, m <= 16384)
