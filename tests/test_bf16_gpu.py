"""-m gpu: bfloat16 weight rows (include/sot_hip.h, ABI 19; csrc/sot_bf16.hip).

Two identities define the feature, so no tolerance appears below:
  forward   every output for bfloat16 x, y equals, bit for bit, the float32 route's output for x.float(), y.float() (widening is exact);
  backward  the gradient of a bfloat16 operand is bfloat16 and equals g32.to(torch.bfloat16) of the float32 route's gradient.
NaN is compared as NaN, not by payload.

1. the conversion kernels against torch's own conversions, inside guard bands (tests/guarded.py);
2. the native kernels (16-bit row loads) on batches that force a workgroup's second and third row: R(G) = CUs * 2048 / G rows are resident
   at most (a workgroup holds at least four waves, a CU at most 32), B = 3 R(G) + 3 -- the rule of tests/test_row_loop_gpu.py -- with
   exactly the float32 problem's workspace, which proves that no widened copy was made;
3. the widening route through the typed entry points, workspace of exactly the reported size, one byte less refused;
4. the module: loss, gradient dtype and bits, per-row positions, the quantile tensors, no_grad / inference_mode, the refusals;
5. torch.compile(fullgraph=True)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bf16_model as bm
import guarded as gd
import row_kinds as rk
from gpu_util import device, native

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
RS, NS, SAME = 8, 32, 64        # SOT_FLAG_REQUIRE_SORT, SOT_FLAG_NO_SPECIALIZE, SOT_FLAG_SAME_GRID
PAPER = 1 | 2 | 4 | 8           # square_dist, dont_normalize, limit_quantile_range, require_sort
SOT_ERR_WORKSPACE = -5
# (name, p, flags): p = 1 on one grid (the merge-free kernel; 2048 bins take its plain row loop), paper mode, general p with dont_normalize
MODES = (("p1_area", 1.0, RS | SAME), ("paper", 2.0, PAPER), ("p3_dn", 3.0, 2 | RS))


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def stream(nat):
    return nat.stream_ptr(device())


def same_bits16(got, want):
    """two bfloat16 tensors: equal bits, NaN compared as NaN"""
    assert got.dtype is BF16 and want.dtype is BF16 and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(got.view(torch.int16)[~gn], want.view(torch.int16)[~wn]))


def same_bits32(got, want):
    assert got.dtype is F32 and want.dtype is F32 and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(got.view(torch.int32)[~gn], want.view(torch.int32)[~wn]))


# ------------------------------------------------------------------------------------------------------------- 1. conversion kernels
@functools.lru_cache(maxsize=2)
def _f32_rows(B, n, seed):
    """[B, n] float32 on the device: the model's adversarial values first, random bit patterns and ordinary values behind them"""
    adv = bm.adversarial_values()
    flat = np.concatenate([adv, bm.random_values(max(B * n - adv.size, 0), seed)])[:B * n]
    if B * n > adv.size:
        flat = np.roll(flat, seed % 5)      # the adversarial values land in other columns (and lanes) from case to case
    return torch.from_numpy(flat.reshape(B, n).copy()).to(device())


# (B, n): every length of the issue on a small batch; then batches of more than three times the row groups of the capped grid (8 workgroups
# per CU; 300 >= the CUs of the chip, asserted), so that workgroups walk a second and a third group: 256 one-element rows per group, one
# 2048-element row per group (16-byte accesses), 1025 elements element-wise
CONV_SHAPES = [(37, 1), (37, 3), (37, 8), (37, 1025), (37, 2048), (37, 24), (3 * 8 * 256 * 300 + 5, 1), (3 * 8 * 300 + 5, 2048), (3 * 8 * 300 + 5, 1025)]
# (source row stride - n, destination row stride - n, source offset in elements, destination offset in elements): dense and aligned; rows
# n + 3 apart; row starts 2 bytes (one bfloat16) off a 16-byte boundary
CONV_LAYOUTS = [(0, 0, 0, 0), (3, 0, 0, 0), (0, 3, 0, 0), (3, 3, 1, 1), (0, 0, 1, 0), (0, 0, 0, 1), (8, 8, 0, 0)]


def _conv_cases():
    """every layout on the small batches; the aligned and the 2-bytes-off layout on the large ones"""
    return [(B, n, lay) for B, n in CONV_SHAPES for lay in CONV_LAYOUTS if B < 1000 or lay in ((0, 0, 0, 0), (3, 3, 1, 1))]


def _conv_ids():
    return [f"B{B}n{n}-{CONV_LAYOUTS.index(lay)}" for B, n, lay in _conv_cases()]


@pytest.mark.parametrize("B,n,layout", _conv_cases(), ids=_conv_ids())
def test_conversion_kernels_equal_torch_inside_guard_bands(B, n, layout):
    nat = native()
    lib = nat.load()
    ds, dd, so, do = layout
    if B > 1000:      # rows per group as csrc/sot_bf16.hip forms them: a chunk is 8 elements where 16-byte accesses apply, 1 otherwise
        chunks = n // 8 if (n % 8 == 0 and layout == (0, 0, 0, 0)) else n
        assert cus() <= 300 and -(-B // max(1, 256 // chunks)) > 3 * 8 * cus()
    src32 = _f32_rows(B, n, 11 + n)
    # ---- f32 -> bf16
    (src, gs) = gd.guarded((B, n), F32, device(), row_stride=n + ds, offset_bytes=4 * so, fill="poison", name="f32 source")
    src.copy_(src32)
    gs.snapshot()
    dst, gdst = gd.guarded((B, n), BF16, device(), row_stride=n + dd, offset_bytes=2 * do, name="bf16 destination")
    rc = lib.sot_rows_f32_to_bf16(gd.ptr(src, gs), B, n, n + ds, gd.ptr(dst, gdst), n + dd, stream(nat))
    assert rc == 0
    gs.assert_unchanged()
    gdst.assert_untouched()
    want16 = src32.to(BF16)
    assert same_bits16(dst.contiguous(), want16), (B, n, layout)
    # ---- bf16 -> f32 (every bit pattern the narrowing produced, NaNs included; plus all 65536 patterns when the tensor holds them)
    src16 = want16.clone()
    if B * n >= 65536:
        src16.view(-1).view(torch.int16)[:65536] = torch.arange(-32768, 32768, device=device()).to(torch.int16)
    (s16, g16) = gd.guarded((B, n), BF16, device(), row_stride=n + ds, offset_bytes=2 * so, fill="poison", name="bf16 source")
    s16.copy_(src16)
    g16.snapshot()
    d32, gd32 = gd.guarded((B, n), F32, device(), row_stride=n + dd, offset_bytes=4 * do, name="f32 destination")
    rc = lib.sot_rows_bf16_to_f32(gd.ptr(s16, g16), B, n, n + ds, gd.ptr(d32, gd32), n + dd, stream(nat))
    assert rc == 0
    g16.assert_unchanged()
    gd32.assert_untouched()
    got32 = d32.contiguous()
    # exact: every bit of the result is the source's bits shifted up, NaN payloads included
    assert torch.equal(got32.view(torch.int32), src16.view(torch.int16).to(torch.int32) << 16), (B, n, layout)
    assert same_bits32(got32, src16.float())


def test_conversion_refusals_and_empty_batch():
    nat = native()
    lib = nat.load()
    dst, g = gd.guarded((4, 8), F32, device(), name="untouched destination")
    src = torch.zeros(4, 8, dtype=BF16, device=device())
    for args in ((src.data_ptr(), -1, 8, 8, gd.ptr(dst, g), 8), (src.data_ptr(), 4, 0, 8, gd.ptr(dst, g), 8), (src.data_ptr(), 4, 8, 7, gd.ptr(dst, g), 8),
                 (src.data_ptr(), 4, 8, 8, gd.ptr(dst, g), 7)):
        assert lib.sot_rows_bf16_to_f32(*args, stream(nat)) == nat.SOT_ERR_BAD_SHAPE, args
        assert lib.sot_rows_f32_to_bf16(*args, stream(nat)) == nat.SOT_ERR_BAD_SHAPE, args
    assert lib.sot_rows_bf16_to_f32(None, 4, 8, 8, gd.ptr(dst, g), 8, stream(nat)) == nat.SOT_ERR_NULL_POINTER
    assert lib.sot_rows_f32_to_bf16(src.data_ptr(), 4, 8, 8, None, 8, stream(nat)) == nat.SOT_ERR_NULL_POINTER
    assert lib.sot_rows_bf16_to_f32(None, 0, 8, 8, None, 8, stream(nat)) == 0          # the empty batch is a defined call
    assert lib.sot_rows_f32_to_bf16(None, 0, 8, 8, None, 8, stream(nat)) == 0
    torch.cuda.synchronize()
    g.assert_untouched()
    assert not torch.isfinite(dst).any()       # the poison is intact inside the view as well


# ------------------------------------------------------------------------------------------------------------- 2. native forward
def _typed_call(nat, x16, y16, xpos, ypos, p, flags, want_mean=False, workspace_bytes=None, ws_align=256):
    """sot_w1d_forward_bf16 / sot_w1d_loss_bf16 with every buffer inside guard bands and a workspace of exactly the reported size.
    Returns (status, rows, mean or None, reported workspace bytes, the float32 problem's workspace bytes, guards)."""
    lib = nat.load()
    B = x16.shape[0]
    pr = nat.make_problem(x16, y16, xpos, ypos, p, flags)
    reported = int(lib.sot_w1d_bf16_workspace_bytes(ctypes.byref(pr)))
    inner = int(lib.sot_workspace_bytes(ctypes.byref(pr)))
    nbytes = reported if workspace_bytes is None else workspace_bytes
    ws, gws = gd.workspace(nbytes, ws_align, device())
    rows, grows = gd.guarded((B,), F32, device(), name="row losses")
    mean, gmean = gd.guarded((1,), F32, device(), name="mean")
    if want_mean:
        rc = lib.sot_w1d_loss_bf16(ctypes.byref(pr), gd.ptr(rows, grows), float(B), 0, 0.0, gd.ptr(mean, gmean), None, None, gd.ptr(ws, gws), nbytes, stream(nat))
    else:
        rc = lib.sot_w1d_forward_bf16(ctypes.byref(pr), gd.ptr(rows, grows), gd.ptr(ws, gws), nbytes, stream(nat))
    torch.cuda.synchronize()
    return rc, rows, (mean if want_mean else None), reported, inner, (gws, grows, gmean)


@functools.lru_cache(maxsize=None)
def _native_batch(n, G):
    B = 3 * (cus() * 2048 // G) + 3
    x, y, _ = rk.make_weights(B, n, n, 1000 + n, device())
    x16, y16 = x.to(BF16), y.to(BF16)
    pos = torch.linspace(0, 1, n, device=device())
    return B, x16, y16, pos, pos.clone()


@functools.lru_cache(maxsize=None)
def _native_reference(n, G, mode):
    """the float32 route on the upcast, computed once per (length, mode) and left unchanged"""
    nat = native()
    _, x16, y16, pos, pos2 = _native_batch(n, G)
    _, p, flags = MODES[mode]
    return nat.forward_rows(x16.float(), y16.float(), pos, pos2, p, flags)


# n, G = threads per row, ROWS per workgroup: the geometries of csrc/sot_full_fwd.hpp (dispatch_area_full_pow2 / dispatch_forward_full_pow2)
NATIVE = [(512, 64, 4), (1024, 128, 2), (2048, 256, 1), (4096, 512, 1)]


@pytest.mark.parametrize("mode", range(3), ids=[m[0] for m in MODES])
@pytest.mark.parametrize("n,G,rows_per_wg", NATIVE, ids=[f"n{n}" for n, _, _ in NATIVE])
def test_native_forward_equals_float32_route_on_the_upcast(n, G, rows_per_wg, mode):
    nat = native()
    B, x16, y16, pos, pos2 = _native_batch(n, G)
    assert B > 3 * (cus() * 2048 // G) and (rows_per_wg == 1 or B % rows_per_wg != 0)     # second and third rows; a partial last row group
    _, p, flags = MODES[mode]
    want = _native_reference(n, G, mode)
    rc, rows, _, reported, inner, guards = _typed_call(nat, x16, y16, pos, pos2, p, flags)
    assert rc == 0
    assert reported == inner, "a native problem needs the float32 problem's workspace: no widened copy"
    for g in guards:
        g.assert_untouched()
    guards[1].assert_fully_written()
    assert torch.equal(rows, want)
    for shift in (1, B // 2 + 1):       # roll invariance, bit for bit: rows change their workgroup, iteration, slot and neighbours
        rc, rolled, *_ = _typed_call(nat, torch.roll(x16, shift, 0), torch.roll(y16, shift, 0), pos, pos2, p, flags)
        assert rc == 0
        assert torch.equal(torch.roll(rolled, -shift, 0), want), shift


def test_native_loss_entry_and_strided_rows():
    """sot_w1d_loss_bf16 on the native route: rows and mean; rows 2048 + 8 elements apart stay native (16-byte aligned rows)"""
    nat = native()
    B, n = 1031, 2048
    x, y, _ = rk.make_weights(B, n, n, 77, device())
    pos = torch.linspace(0, 1, n, device=device())
    wide = torch.empty(B, n + 8, dtype=BF16, device=device()).fill_(float("nan"))
    wide2 = wide.clone()
    x16, y16 = wide[:, :n], wide2[:, :n]
    x16.copy_(x)
    y16.copy_(y)
    for _, p, flags in MODES:
        mean32, rows32, _ = nat.loss_fused(x16.float(), y16.float(), pos, pos.clone(), p, flags)
        rc, rows, mean, reported, inner, guards = _typed_call(nat, x16, y16, pos, pos.clone(), p, flags, want_mean=True)
        assert rc == 0 and reported == inner
        for g in guards:
            g.assert_untouched()
        assert torch.equal(rows, rows32) and torch.equal(mean.reshape(()), mean32)


# ------------------------------------------------------------------------------------------------------------- 3. widening routes
WIDE_B = 67


def _wide_case(name):
    """(x16, y16, xpos, ypos, extra flags) of one widening case; rows are views where the case is about strides"""
    dev = device()
    n, m, rowpos, stride, extra = {"bins1025": (1025, 1025, False, None, 0), "bins257": (257, 257, False, None, 0), "bins1000": (1000, 1000, False, None, 0),
                                   "stride2049": (2048, 2048, False, 2049, 0), "no_specialize": (2048, 2048, False, None, NS),
                                   "rowpos512": (512, 512, True, None, 0), "n700_m300": (700, 300, False, None, 0)}[name]
    x, y, _ = rk.make_weights(WIDE_B, n, m, 31 + n, dev)
    if stride is None:
        x16, y16 = x.to(BF16), y.to(BF16)
    else:       # rows `stride` elements apart: alternately 2 bytes off a 4-byte boundary; the gaps hold NaN
        bx = torch.full((WIDE_B, stride), float("nan"), dtype=BF16, device=dev)
        by = bx.clone()
        x16, y16 = bx[:, :n], by[:, :m]
        x16.copy_(x)
        y16.copy_(y)
    if rowpos:
        xpos, _ = rk.make_positions(WIDE_B, n, 5, dev)
        ypos, _ = rk.make_positions(WIDE_B, m, 6, dev)
    else:
        xpos, ypos = torch.linspace(0, 1, n, device=dev), torch.linspace(0, 1, m, device=dev)
    return x16, y16, xpos, ypos, extra, n == m and not rowpos


WIDE = ["bins1025", "bins257", "bins1000", "stride2049", "no_specialize", "rowpos512", "n700_m300"]


@pytest.mark.parametrize("name", WIDE)
def test_widening_route_equals_float32_call_on_the_upcast(name):
    nat = native()
    x16, y16, xpos, ypos, extra, one_grid = _wide_case(name)
    for mode, p, flags in MODES:
        if mode == "p1_area" and not one_grid:
            flags = RS                      # two grids: p = 1 on the merge kernel
        flags |= extra
        mean32, rows32, _ = nat.loss_fused(x16.float(), y16.float(), xpos, ypos, p, flags)
        for align in (256, 4):              # any alignment of the workspace will do
            rc, rows, mean, reported, inner, guards = _typed_call(nat, x16, y16, xpos, ypos, p, flags, want_mean=True, ws_align=align)
            assert rc == 0, (name, mode)
            assert reported >= inner + 4 * WIDE_B * (x16.shape[1] + y16.shape[1])
            for g in guards:
                g.assert_untouched()
            guards[1].assert_fully_written()
            assert torch.equal(rows, rows32), (name, mode)
            assert torch.equal(mean.reshape(()), mean32), (name, mode)
        rc, rows_only, *_ = _typed_call(nat, x16, y16, xpos, ypos, p, flags)
        assert rc == 0 and torch.equal(rows_only, rows32)
        # one byte less: refused before anything is enqueued, the outputs keep their poison
        rc, rows, mean, reported, _, guards = _typed_call(nat, x16, y16, xpos, ypos, p, flags, want_mean=True, workspace_bytes=reported - 1)
        assert rc == SOT_ERR_WORKSPACE, (name, mode)
        for g in guards:
            g.assert_untouched()
        assert bool((rows.view(torch.int32) == gd.POISON).all()) and bool((mean.view(torch.int32) == gd.POISON).all())


def test_typed_refusals_match_the_float32_entry_points():
    nat = native()
    lib = nat.load()
    x16, y16, xpos, ypos, _, _ = _wide_case("bins257")
    rows = torch.empty(WIDE_B, device=device())
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=device())

    def both(change, want):
        pr = nat.make_problem(x16, y16, xpos, ypos, 2.0, PAPER)
        pf = nat.make_problem(x16.float(), y16.float(), xpos, ypos, 2.0, PAPER)
        for q in (pr, pf):
            change(q)
        got16 = lib.sot_w1d_forward_bf16(ctypes.byref(pr), rows.data_ptr(), ws.data_ptr(), ws.numel(), stream(nat))
        got32 = lib.sot_w1d_forward(ctypes.byref(pf), rows.data_ptr(), ws.data_ptr(), ws.numel(), stream(nat))
        assert got16 == got32 == want, (got16, got32, want)

    both(lambda q: setattr(q, "p", 0.5), nat.SOT_ERR_INVALID_P)
    both(lambda q: setattr(q, "B", -1), nat.SOT_ERR_BAD_SHAPE)
    both(lambda q: setattr(q, "x_row_stride", 256), nat.SOT_ERR_BAD_SHAPE)
    both(lambda q: setattr(q, "y", None), nat.SOT_ERR_NULL_POINTER)
    both(lambda q: (setattr(q, "n", 20000), setattr(q, "m", 20000), setattr(q, "x_row_stride", 20000), setattr(q, "y_row_stride", 20000)),
         nat.SOT_ERR_UNSUPPORTED_SIZE)
    assert lib.sot_w1d_forward_bf16(None, rows.data_ptr(), ws.data_ptr(), ws.numel(), stream(nat)) == nat.SOT_ERR_NULL_POINTER
    pr = nat.make_problem(x16, y16, xpos, ypos, 2.0, PAPER)
    assert lib.sot_w1d_forward_bf16(ctypes.byref(pr), None, ws.data_ptr(), ws.numel(), stream(nat)) == nat.SOT_ERR_NULL_POINTER
    assert lib.sot_w1d_forward_bf16(ctypes.byref(pr), rows.data_ptr(), None, 0, stream(nat)) == nat.SOT_ERR_NULL_POINTER     # the widened copies need a place
    assert lib.sot_w1d_loss_bf16(ctypes.byref(pr), rows.data_ptr(), 67.0, 0, 0.0, None, None, None, ws.data_ptr(), ws.numel(), stream(nat)) == nat.SOT_ERR_NULL_POINTER
    pr.B = 0
    assert lib.sot_w1d_forward_bf16(ctypes.byref(pr), None, None, 0, stream(nat)) == 0                                        # an empty batch: nothing to do
    assert lib.sot_w1d_loss_bf16(ctypes.byref(pr), rows.data_ptr(), 1.0, 0, 0.0, rows.data_ptr(), None, None, None, 0, stream(nat)) == nat.SOT_ERR_BAD_SHAPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 4. module and gradient
def _paper_module():
    from sot_amd.losses import Wasserstein1D
    native()
    return Wasserstein1D(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True).to(device())


def _weights16(B, n, seed, m=None):
    x, y, _ = rk.make_weights(B, n, n if m is None else m, seed, device())
    return x.to(BF16), y.to(BF16)


def _loss_and_grad(mod, x, y, **kw):
    y = y.detach().clone().requires_grad_(True)
    loss = mod(x, y, **kw)
    loss.backward()
    return loss.detach(), y.grad


@pytest.mark.parametrize("config", ["p1_fixed_x_2048", "paper_1025"])
def test_module_loss_and_gradient(config):
    from sot_amd.losses import Wasserstein1D
    native()
    if config == "p1_fixed_x_2048":
        mod, n, kw = Wasserstein1D(p=1, fixed_x=2048).to(device()), 2048, {}
    else:
        pos = torch.fft.rfftfreq(2048, 1 / 16000.0).to(device())
        pos = pos / pos.max()
        mod, n, kw = _paper_module(), 1025, dict(x_pos=pos, y_pos=pos.clone())
    x16, y16 = _weights16(131, n, 3)
    loss16, g16 = _loss_and_grad(mod, x16, y16, **kw)
    loss32, g32 = _loss_and_grad(mod, x16.float(), y16.float(), **kw)
    assert loss16.dtype is F32 and same_bits32(loss16, loss32)
    assert g16.dtype is BF16 and g32.dtype is F32
    assert same_bits16(g16, g32.to(BF16))
    assert bool((g16 != 0).any())
    # both operands differentiated, 3-D input, a reduction over one axis (the row-loss route)
    x3 = x16[:128].reshape(4, 32, n).clone().requires_grad_(True)
    y3 = y16[:128].reshape(4, 32, n).clone().requires_grad_(True)
    xf, yf = x3.detach().float().requires_grad_(True), y3.detach().float().requires_grad_(True)
    out16, out32 = mod(x3, y3, dims=1, **kw), mod(xf, yf, dims=1, **kw)
    assert out16.dtype is F32 and same_bits32(out16.detach(), out32.detach())
    cot = torch.rand(out16.shape, device=device())
    out16.backward(cot)
    out32.backward(cot)
    assert x3.grad.dtype is BF16 and same_bits16(x3.grad, xf.grad.to(BF16)) and same_bits16(y3.grad, yf.grad.to(BF16))


def test_module_per_row_positions_and_position_gradient():
    mod = _paper_module()
    B, n = 67, 512
    x16, y16 = _weights16(B, n, 9)
    xp, _ = rk.make_positions(B, n, 5, device())
    yp, _ = rk.make_positions(B, n, 6, device())
    out = []
    for wide in (False, True):
        x = x16.float() if wide else x16
        y = (y16.float() if wide else y16).clone().requires_grad_(True)
        xpos, ypos = xp.clone().requires_grad_(True), yp.clone().requires_grad_(True)
        loss = mod(x, y, x_pos=xpos, y_pos=ypos)
        loss.backward()
        out.append((loss.detach(), y.grad, xpos.grad, ypos.grad))
    (l16, gy16, gxp16, gyp16), (l32, gy32, gxp32, gyp32) = out
    assert l16.dtype is F32 and same_bits32(l16, l32)
    assert gy16.dtype is BF16 and same_bits16(gy16, gy32.to(BF16))
    assert gxp16.dtype is F32 and gyp16.dtype is F32 and same_bits32(gxp16, gxp32) and same_bits32(gyp16, gyp32)


def test_module_return_quantiles_under_a_random_cotangent():
    mod = _paper_module()
    B, n = 33, 257
    x16, y16 = _weights16(B, n, 13)
    pos = torch.linspace(0, 1, n, device=device())
    g = torch.Generator(device=device()).manual_seed(5)
    cots = None
    res = []
    for wide in (False, True):
        x = (x16.float() if wide else x16).clone().requires_grad_(True)
        y = (y16.float() if wide else y16).clone().requires_grad_(True)
        outs = mod(x, y, x_pos=pos, y_pos=pos.clone(), return_quantiles=True)
        assert len(outs) == 5 and all(o.dtype is F32 for o in outs)
        if cots is None:
            cots = [torch.rand(o.shape, generator=g, device=device()) - 0.5 for o in outs]
        sum((o * c).sum() for o, c in zip(outs, cots)).backward()
        res.append(([o.detach() for o in outs], x.grad, y.grad))
    (o16, gx16, gy16), (o32, gx32, gy32) = res
    for a, b in zip(o16, o32):
        assert same_bits32(a, b)
    assert gx16.dtype is BF16 and gy16.dtype is BF16
    assert same_bits16(gx16, gx32.to(BF16)) and same_bits16(gy16, gy32.to(BF16))


def test_calls_without_a_gradient_take_the_typed_forward(monkeypatch):
    from sot_amd import losses
    from sot_amd.losses import Wasserstein1D, wasserstein_1d
    nat = native()
    taken = []
    for name in ("loss_fused_bf16", "forward_rows_bf16"):
        real = getattr(nat, name)
        monkeypatch.setattr(nat, name, (lambda real, name: lambda *a, **k: (taken.append(name), real(*a, **k))[1])(real, name))
    monkeypatch.setattr(nat, "rows_to_f32", lambda *a, **k: pytest.fail("a call without a gradient widened its rows in Python"))
    assert losses.nat is nat
    mod = Wasserstein1D(p=1, fixed_x=2048).to(device())
    x16, y16 = _weights16(259, 2048, 21)
    with torch.no_grad():
        loss32 = mod(x16.float(), y16.float())
        loss16 = mod(x16, y16)
    assert taken == ["loss_fused_bf16"] and loss16.dtype is F32 and same_bits32(loss16, loss32)
    with torch.inference_mode():
        assert same_bits32(mod(x16, y16), loss32)
    assert same_bits32(mod(x16, y16), loss32)                       # grad mode on, but nothing requires a gradient
    assert taken == ["loss_fused_bf16"] * 3
    rows16, rows32 = mod.row_losses(x16, y16), mod.row_losses(x16.float(), y16.float())
    assert taken[-1] == "forward_rows_bf16" and rows16.dtype is F32 and same_bits32(rows16, rows32)
    # the paper's configuration on 1025 bins (widened inside the call) and the functional form (weights as given)
    paper = _paper_module()
    a16, b16 = _weights16(67, 1025, 22)
    pos = torch.linspace(0, 1, 1025, device=device())
    assert same_bits32(paper(a16, b16, x_pos=pos, y_pos=pos.clone()), paper(a16.float(), b16.float(), x_pos=pos, y_pos=pos.clone()))
    u, v = pos.expand(67, 1025), pos.clone().expand(67, 1025)      # stride-0 rows: one shared grid per side
    assert same_bits32(wasserstein_1d(u, v, a16, b16, p=2), wasserstein_1d(u, v, a16.float(), b16.float(), p=2))
    assert taken[-2:] == ["loss_fused_bf16", "forward_rows_bf16"]


def test_float16_and_mixed_operands_are_refused():
    from sot_amd.losses import Wasserstein1D, wasserstein_1d
    native()
    mod = Wasserstein1D(p=1, fixed_x=512).to(device())
    x16, y16 = _weights16(5, 512, 1)
    for x, y in ((x16.half(), y16.half()), (x16, y16.float()), (x16.float(), y16), (x16, y16.half())):
        with pytest.raises(TypeError, match="sot_amd computes in float32"):
            mod(x, y)
        with pytest.raises(TypeError, match="sot_amd computes in float32"):
            mod.row_losses(x, y)
    pos = torch.linspace(0, 1, 512, device=device()).expand(5, 512)
    with pytest.raises(TypeError, match="sot_amd computes in float32"):
        wasserstein_1d(pos, pos, x16, y16.float())
    with pytest.raises(TypeError, match="sot_amd computes in float32"):       # positions stay float32
        mod(x16, y16, x_pos=pos[0].to(BF16), y_pos=pos[0].to(BF16))


# ------------------------------------------------------------------------------------------------------------- 5. torch.compile
def test_compiled_module_equals_eager_on_bfloat16_inputs():
    from sot_amd import ops
    from sot_amd.losses import Wasserstein1D
    native()
    torch._dynamo.reset()
    mod = Wasserstein1D(p=1, fixed_x=2048).to(device())
    x16, y16 = _weights16(64, 2048, 41)
    eager_loss, eager_grad = _loss_and_grad(mod, x16, y16)
    with torch.no_grad():
        eager_plain = mod(x16, y16)
    before = dict(ops.CALLS)
    compiled = torch.compile(mod, fullgraph=True)
    loss, grad = _loss_and_grad(compiled, x16, y16)
    assert loss.dtype is F32 and torch.equal(loss, eager_loss)
    assert grad.dtype is BF16 and torch.equal(grad, eager_grad)
    assert ops.CALLS["rows_to_f32"] > before.get("rows_to_f32", 0) and ops.CALLS["rows_to_bf16"] > before.get("rows_to_bf16", 0)
    with torch.no_grad():
        plain = compiled(x16, y16)
    assert torch.equal(plain, eager_plain) and ops.CALLS["w1d_mean_bf16"] > before.get("w1d_mean_bf16", 0)
    torch._dynamo.reset()


def test_bf16_ops_pass_opcheck():
    from sot_amd import ops
    native()
    x16, y16 = _weights16(5, 33, 51)
    pos = torch.rand(33, device=device())
    rp = torch.rand(5, 33, device=device())
    R = lambda t: t.clone().requires_grad_(True)               # noqa: E731
    samples = {
        "rows_to_f32": [(R(x16),), (x16[:, :17],)],
        "rows_to_bf16": [(R(x16.float()),)],
        "w1d_rows_bf16": [(R(x16), R(y16), R(pos), R(pos), 2.0, PAPER), (R(x16), R(y16), R(rp), R(rp), 2.0, PAPER)],
        "w1d_mean_bf16": [(R(x16), R(y16), R(pos), R(pos), 2.0, PAPER), (x16, y16, pos, pos, 1.0, RS)],
    }
    assert sorted(samples) == sorted(ops.BF16_NAMES)
    for name, argsets in samples.items():
        op = getattr(torch.ops.sot_amd, name).default
        for args in argsets:
            torch.library.opcheck(op, args)
