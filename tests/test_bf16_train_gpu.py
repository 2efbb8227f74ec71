"""-m gpu: bfloat16 training (include/sot_hip.h, ABI 20; csrc/sot_bf16_bwd.hip) -- 16-bit row loads and 16-bit gradient stores inside the
full-row backward kernels, the typed entry points sot_w1d_backward_bf16 / sot_w1d_loss_and_grad_bf16 and the module's typed training route.

The result is defined bit for bit, so no tolerance appears below: each gradient element equals rne(v) -- v the float32 call's element on
x16.float(), y16.float(), rne torch's .to(torch.bfloat16) -- or rne(v * g) in fix-up mode (g = *rescale, one float32 multiply); row losses
and the mean equal the float32 call's bits.  NaN is compared as NaN.

1. the native kernels on batches sized by the rule of tests/test_row_loop_gpu.py (R(G) = CUs * 2048 / G rows are resident at most,
   B = 3 R(G) + 3: every workgroup walks a second row and most a third, and the last row group is partial where a workgroup holds 2 or 4
   rows), per-row random cotangents, every buffer inside guard bands (tests/guarded.py), a workspace of exactly the reported size -- the
   float32 problem's, which proves that no float32 image was made -- and roll invariance;
2. the training form, also on rows 2048 + 8 elements apart; 3. the fix-up mode; 4. the widening routes; 5. refusals and B == 0;
6. the module: loss bits, gradient bits, a second backward through a retained graph, and no row conversion from Python."""
import ctypes
import functools

import pytest
import torch

import guarded as gd
import row_kinds as rk
from gpu_util import device, native

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
RS, NS, SAME, TIE_FREE = 8, 32, 64, 256     # SOT_FLAG_REQUIRE_SORT, _NO_SPECIALIZE, _SAME_GRID, _TIE_FREE_GRADIENT
PAPER = 1 | 2 | 4 | 8                        # square_dist, dont_normalize, limit_quantile_range, require_sort
SOT_ERR_WORKSPACE = -5
MODES = (("p1_area", 1.0, RS | SAME), ("paper", 2.0, PAPER), ("p3_dn", 3.0, 2 | RS))     # those of tests/test_bf16_gpu.py


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def stream(nat):
    return nat.stream_ptr(device())


def same_bits16(got, want):
    assert got.dtype is BF16 and want.dtype is BF16 and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(got.view(torch.int16)[~gn], want.view(torch.int16)[~wn]))


def same_bits32(got, want):
    assert got.dtype is F32 and want.dtype is F32 and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(got.view(torch.int32)[~gn], want.view(torch.int32)[~wn]))


def untouched16(t):
    """a guarded buffer (typed_backward / typed_loss_and_grad attach the guard) that still holds the poison in every 32-bit word, view included"""
    return bool((t.guard.flat.view(torch.int32) == gd.POISON).all())


class Out:
    pass


def typed_backward(nat, x16, y16, xpos, ypos, p, flags, grad_row, want_x, grad_scale=1.0, rescale=None, workspace_bytes=None, ws_align=256,
                   gy_into=None):
    """sot_w1d_backward_bf16 with every buffer inside guard bands and a workspace of exactly the reported size (or workspace_bytes)"""
    lib = nat.load()
    B, n = x16.shape
    m = y16.shape[1]
    o = Out()
    pr = nat.make_problem(x16, y16, xpos, ypos, p, flags)
    o.reported = int(lib.sot_w1d_bf16_backward_workspace_bytes(ctypes.byref(pr), int(want_x), 1))
    o.inner = int(lib.sot_workspace_bytes(ctypes.byref(pr)))
    o.native = bool(lib.sot_w1d_bf16_native(ctypes.byref(pr)))
    nbytes = o.reported if workspace_bytes is None else workspace_bytes
    ws, gws = gd.workspace(nbytes, ws_align, device())
    o.gx, ggx = gd.guarded((B, n), BF16, device(), name="grad_x") if want_x else (None, None)
    o.gy, ggy = gd.guarded((B, m), BF16, device(), name="grad_y") if gy_into is None else gy_into
    stride = 0 if (grad_row is None or grad_row.numel() == 1) else 1
    o.rc = lib.sot_w1d_backward_bf16(ctypes.byref(pr), None if grad_row is None else grad_row.data_ptr(), stride, float(grad_scale),
                                     gd.ptr(o.gx, ggx) if want_x else None, gd.ptr(o.gy, ggy), None if rescale is None else rescale.data_ptr(),
                                     gd.ptr(ws, gws), nbytes, stream(nat))
    torch.cuda.synchronize()
    o.gy.guard = ggy
    if want_x:
        o.gx.guard = ggx
    o.guards = [g for g in (gws, ggx, ggy) if g is not None]
    o.grad_guards = [g for g in (ggx, ggy) if g is not None]
    return o


def typed_loss_and_grad(nat, x16, y16, xpos, ypos, p, flags, workspace_bytes=None, ws_align=256):
    lib = nat.load()
    B, m = x16.shape[0], y16.shape[1]
    o = Out()
    pr = nat.make_problem(x16, y16, xpos, ypos, p, flags)
    o.reported = int(lib.sot_w1d_bf16_backward_workspace_bytes(ctypes.byref(pr), 0, 1))
    o.inner = int(lib.sot_workspace_bytes(ctypes.byref(pr)))
    nbytes = o.reported if workspace_bytes is None else workspace_bytes
    ws, gws = gd.workspace(nbytes, ws_align, device())
    o.rows, grows = gd.guarded((B,), F32, device(), name="row losses")
    o.mean, gmean = gd.guarded((1,), F32, device(), name="mean")
    o.gy, ggy = gd.guarded((B, m), BF16, device(), name="grad_y")
    o.rc = lib.sot_w1d_loss_and_grad_bf16(ctypes.byref(pr), gd.ptr(o.rows, grows), float(B), gd.ptr(o.mean, gmean), None, 1.0 / B, gd.ptr(o.gy, ggy),
                                          None, gd.ptr(ws, gws), nbytes, stream(nat))
    torch.cuda.synchronize()
    o.gy.guard = ggy
    o.guards = [gws, grows, gmean, ggy]
    o.written = [grows, ggy]
    return o


# ------------------------------------------------------------------------------------------------------------- 1. native backward
# n, G = threads per row, rows per workgroup of the both-gradient / of the y-only kernel (csrc/sot_full_bwd.hpp: dispatch_backward_full_pow2)
NATIVE = [(512, 64, 4, 4), (1024, 128, 2, 2), (2048, 256, 1, 2), (4096, 512, 1, 1)]


@functools.lru_cache(maxsize=None)
def _native_batch(n, G):
    B = 3 * (cus() * 2048 // G) + 3
    x, y, _ = rk.make_weights(B, n, n, 2000 + n, device())
    pos = torch.linspace(0, 1, n, device=device())
    cot = torch.rand(B, generator=torch.Generator(device=device()).manual_seed(n), device=device()) + 0.25
    return B, x.to(BF16), y.to(BF16), pos, pos.clone(), cot


@functools.lru_cache(maxsize=None)
def _native_reference(n, G, mode, want_x):
    """the float32 route on the upcast, narrowed by torch: computed once per case and left unchanged"""
    nat = native()
    _, x16, y16, pos, pos2, cot = _native_batch(n, G)
    _, p, flags = MODES[mode]
    gx, gy = nat.backward_rows(x16.float(), y16.float(), pos, pos2, p, flags, cot, need_gx=want_x, need_gy=True)
    return (gx.to(BF16) if want_x else None), gy.to(BF16)


@pytest.mark.parametrize("want_x", [False, True], ids=["y_only", "both"])
@pytest.mark.parametrize("mode", range(3), ids=[m[0] for m in MODES])
@pytest.mark.parametrize("n,G,rows_both,rows_y", NATIVE, ids=[f"n{n}" for n, *_ in NATIVE])
def test_native_backward_equals_float32_route_on_the_upcast(n, G, rows_both, rows_y, mode, want_x):
    nat = native()
    B, x16, y16, pos, pos2, cot = _native_batch(n, G)
    rows_per_wg = rows_both if want_x else rows_y
    assert B > 3 * (cus() * 2048 // G) and (rows_per_wg == 1 or B % rows_per_wg != 0)     # second and third rows; a partial last row group
    _, p, flags = MODES[mode]
    want_gx, want_gy = _native_reference(n, G, mode, want_x)
    o = typed_backward(nat, x16, y16, pos, pos2, p, flags, cot, want_x)
    assert o.rc == 0 and o.native
    assert o.reported == o.inner, "a native problem needs the float32 problem's workspace: no float32 image of a spectrum or a gradient"
    for g in o.guards:
        g.assert_untouched()
    for g in o.grad_guards:
        g.assert_fully_written()
    assert same_bits16(o.gy, want_gy)
    assert not want_x or same_bits16(o.gx, want_gx)
    assert bool((o.gy.float() != 0).any())
    for shift in (1, B // 2 + 1):       # roll invariance, bit for bit: rows change their workgroup, iteration, slot and neighbours
        r = typed_backward(nat, torch.roll(x16, shift, 0), torch.roll(y16, shift, 0), pos, pos2, p, flags, torch.roll(cot, shift, 0), want_x)
        assert r.rc == 0
        assert same_bits16(torch.roll(r.gy, -shift, 0), want_gy), shift
        assert not want_x or same_bits16(torch.roll(r.gx, -shift, 0), want_gx), shift


def test_native_backward_through_a_permuted_grid():
    """positions that are not sorted: the gradients leave through the plan's permutation as single 16-bit elements"""
    nat = native()
    B, n = 67, 512
    x, y, _ = rk.make_weights(B, n, n, 5, device())
    x16, y16 = x.to(BF16), y.to(BF16)
    gen = torch.Generator(device=device()).manual_seed(3)
    xpos, ypos = torch.rand(n, generator=gen, device=device()), torch.rand(n, generator=gen, device=device())
    cot = torch.rand(B, generator=gen, device=device())
    for _, p, flags in MODES[1:]:
        for want_x in (False, True):
            gx, gy = nat.backward_rows(x16.float(), y16.float(), xpos, ypos, p, flags, cot, need_gx=want_x, need_gy=True)
            o = typed_backward(nat, x16, y16, xpos, ypos, p, flags, cot, want_x)
            assert o.rc == 0 and o.native and o.reported == o.inner
            for g in o.guards:
                g.assert_untouched()
            for g in o.grad_guards:
                g.assert_fully_written()
            assert same_bits16(o.gy, gy.to(BF16)) and (not want_x or same_bits16(o.gx, gx.to(BF16)))


# ------------------------------------------------------------------------------------------------------------- 2. training form
def _strided(B, n, seed, pad):
    x, y, _ = rk.make_weights(B, n, n, seed, device())
    bx = torch.full((B, n + pad), float("nan"), dtype=BF16, device=device())
    by = bx.clone()
    x16, y16 = bx[:, :n], by[:, :n]
    x16.copy_(x)
    y16.copy_(y)
    return x16, y16


@pytest.mark.parametrize("n,pad", [(2048, 8), (2048, 0), (512, 0), (1024, 0), (4096, 0)], ids=["n2048_stride2056", "n2048", "n512", "n1024", "n4096"])
def test_training_form_equals_float32_call_on_the_upcast(n, pad):
    """row losses, mean and grad_y; rows 2048 + 8 elements apart stay native (16-byte aligned rows)"""
    nat = native()
    B = 1031 if n >= 2048 else 2051
    x16, y16 = _strided(B, n, 70 + n + pad, pad)
    pos = torch.linspace(0, 1, n, device=device())
    for _, p, flags in MODES:
        mean32, rows32, gy32 = nat.loss_and_grad(x16.float(), y16.float(), pos, pos.clone(), p, flags)
        o = typed_loss_and_grad(nat, x16, y16, pos, pos.clone(), p, flags)
        assert o.rc == 0 and o.reported == o.inner
        for g in o.guards:
            g.assert_untouched()
        for g in o.written:
            g.assert_fully_written()
        assert same_bits32(o.rows, rows32) and same_bits32(o.mean.reshape(()), mean32)
        assert same_bits16(o.gy, gy32.to(BF16))


# ------------------------------------------------------------------------------------------------------------- 3. fix-up mode
@pytest.mark.parametrize("n", [2048, 512])
def test_fix_up_mode(n):
    nat = native()
    B = 1031
    x16, y16 = _strided(B, n, 90 + n, 0)
    pos = torch.linspace(0, 1, n, device=device())
    for _, p, flags in MODES:
        _, _, v32 = nat.loss_and_grad(x16.float(), y16.float(), pos, pos.clone(), p, flags)
        # *rescale == 1: every workgroup leaves at once, the buffer keeps its sentinel
        one = torch.ones(1, device=device())
        o = typed_backward(nat, x16, y16, pos, pos.clone(), p, flags, None, False, grad_scale=1.0 / B, rescale=one)
        assert o.rc == 0 and o.native
        for g in o.guards:
            g.assert_untouched()
        assert untouched16(o.gy)
        for g in (0.37, -2.5):
            scal = torch.full((1,), g, device=device())
            o = typed_backward(nat, x16, y16, pos, pos.clone(), p, flags, None, False, grad_scale=1.0 / B, rescale=scal)
            assert o.rc == 0 and o.reported == o.inner
            for gg in o.guards:
                gg.assert_untouched()
            o.grad_guards[0].assert_fully_written()
            assert same_bits16(o.gy, (v32 * scal).to(BF16)), (p, g)
    # the scalar belongs to the y-only call
    o = typed_backward(nat, x16, y16, pos, pos.clone(), 2.0, PAPER, None, True, rescale=torch.ones(1, device=device()))
    assert o.rc == nat.SOT_ERR_BAD_SHAPE and untouched16(o.gx) and untouched16(o.gy)


# ------------------------------------------------------------------------------------------------------------- 4. widening routes
WIDE_B = 67
WIDE = {"bins1025": (1025, 1025, False, None, 0), "bins257": (257, 257, False, None, 0), "bins1000": (1000, 1000, False, None, 0),
        "stride2049": (2048, 2048, False, 2049, 0), "no_specialize": (2048, 2048, False, None, NS), "rowpos512": (512, 512, True, None, 0),
        "n700_m300": (700, 300, False, None, 0), "tie_free": (2048, 2048, False, None, TIE_FREE)}


def _wide_case(name):
    dev = device()
    n, m, rowpos, stride, extra = WIDE[name]
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


@pytest.mark.parametrize("name", list(WIDE))
def test_widening_routes_equal_float32_calls_on_the_upcast(name):
    nat = native()
    x16, y16, xpos, ypos, extra, one_grid = _wide_case(name)
    n, m = x16.shape[1], y16.shape[1]
    cot = torch.rand(WIDE_B, generator=torch.Generator(device=device()).manual_seed(17), device=device()) + 0.25
    scal = torch.full((1,), 0.37, device=device())
    for mode, p, flags in MODES:
        if mode == "p1_area" and not one_grid:
            flags = RS                      # two grids
        flags |= extra
        x32, y32 = x16.float(), y16.float()
        for want_x in (False, True):
            gx32, gy32 = nat.backward_rows(x32, y32, xpos, ypos, p, flags, cot, need_gx=want_x, need_gy=True)
            for align in (256, 2):          # any alignment of the workspace will do
                o = typed_backward(nat, x16, y16, xpos, ypos, p, flags, cot, want_x, ws_align=align)
                assert o.rc == 0 and not o.native, (name, mode)
                assert o.reported >= o.inner + 4 * WIDE_B * (n + m) + 4 * WIDE_B * (m + (n if want_x else 0))
                for g in o.guards:
                    g.assert_untouched()
                for g in o.grad_guards:
                    g.assert_fully_written()
                assert same_bits16(o.gy, gy32.to(BF16)), (name, mode, want_x)
                assert not want_x or same_bits16(o.gx, gx32.to(BF16)), (name, mode)
            # one byte less: refused before anything is enqueued, the outputs keep their poison
            o = typed_backward(nat, x16, y16, xpos, ypos, p, flags, cot, want_x, workspace_bytes=o.reported - 1)
            assert o.rc == SOT_ERR_WORKSPACE, (name, mode)
            for g in o.guards:
                g.assert_untouched()
            assert untouched16(o.gy) and (not want_x or untouched16(o.gx))
        # the training form, and its gradient fixed up by 0.37
        mean32, rows32, v32 = nat.loss_and_grad(x32, y32, xpos, ypos, p, flags)
        t = typed_loss_and_grad(nat, x16, y16, xpos, ypos, p, flags)
        assert t.rc == 0 and t.reported >= t.inner + 4 * WIDE_B * (n + 2 * m), (name, mode)
        for g in t.guards:
            g.assert_untouched()
        for g in t.written:
            g.assert_fully_written()
        assert same_bits32(t.rows, rows32) and same_bits32(t.mean.reshape(()), mean32), (name, mode)
        assert same_bits16(t.gy, v32.to(BF16)), (name, mode)
        o = typed_backward(nat, x16, y16, xpos, ypos, p, flags, None, False, grad_scale=1.0 / WIDE_B, rescale=scal)
        assert o.rc == 0 and same_bits16(o.gy, (v32 * scal).to(BF16)), (name, mode)
        for g in o.guards:
            g.assert_untouched()
        t = typed_loss_and_grad(nat, x16, y16, xpos, ypos, p, flags, workspace_bytes=t.reported - 1)
        assert t.rc == SOT_ERR_WORKSPACE
        for g in t.guards:
            g.assert_untouched()
        assert untouched16(t.gy) and bool((t.rows.view(torch.int32) == gd.POISON).all())


def test_gradient_rows_off_a_16_byte_boundary_take_the_widening_route():
    """a native problem whose gradient buffer starts 2 bytes off: widened inside the call, with the workspace the size function reports for
    the same problem under SOT_FLAG_NO_SPECIALIZE (include/sot_hip.h); the native-sized workspace is refused"""
    nat = native()
    lib = nat.load()
    B, n = 67, 512
    x16, y16 = _strided(B, n, 3, 0)
    pos = torch.linspace(0, 1, n, device=device())
    cot = torch.rand(B, device=device())
    _, gy32 = nat.backward_rows(x16.float(), y16.float(), pos, pos.clone(), 2.0, PAPER, cot, need_gx=False, need_gy=True)
    pr = nat.make_problem(x16, y16, pos, pos.clone(), 2.0, PAPER | NS)
    widened = int(lib.sot_w1d_bf16_backward_workspace_bytes(ctypes.byref(pr), 0, 1))
    off = gd.guarded((B, n), BF16, device(), offset_bytes=2, name="grad_y, 2 bytes off")
    o = typed_backward(nat, x16, y16, pos, pos.clone(), 2.0, PAPER, cot, False, workspace_bytes=widened, gy_into=off)
    assert o.rc == 0 and o.native and widened > o.reported
    for g in o.guards:
        g.assert_untouched()
    o.grad_guards[0].assert_fully_written()
    assert same_bits16(o.gy.contiguous(), gy32.to(BF16))
    off = gd.guarded((B, n), BF16, device(), offset_bytes=2, name="grad_y, 2 bytes off")
    o = typed_backward(nat, x16, y16, pos, pos.clone(), 2.0, PAPER, cot, False, gy_into=off)
    assert o.rc == SOT_ERR_WORKSPACE and untouched16(o.gy)


# ------------------------------------------------------------------------------------------------------------- 5. refusals and B == 0
@pytest.mark.parametrize("name", ["bins257", "native2048"])
def test_typed_refusals_and_empty_batch_match_the_float32_entry_points(name):
    nat = native()
    lib = nat.load()
    if name == "native2048":
        x16, y16 = _strided(WIDE_B, 2048, 4, 0)
        xpos = torch.linspace(0, 1, 2048, device=device())
        ypos = xpos.clone()
    else:
        x16, y16, xpos, ypos, _, _ = _wide_case(name)
    B, n = x16.shape
    rows = torch.empty(B, device=device())
    mean = torch.empty(1, device=device())
    cot = torch.rand(B, device=device())
    g16 = torch.empty(B, n, dtype=BF16, device=device())
    g32 = torch.empty(B, n, device=device())
    ws = torch.empty(1 << 21, dtype=torch.uint8, device=device())
    s = stream(nat)

    def both(change, want, stride=1):
        pr = nat.make_problem(x16, y16, xpos, ypos, 2.0, PAPER)
        pf = nat.make_problem(x16.float(), y16.float(), xpos, ypos, 2.0, PAPER)
        for q in (pr, pf):
            change(q)
        got16 = lib.sot_w1d_backward_bf16(ctypes.byref(pr), cot.data_ptr(), stride, 1.0, None, g16.data_ptr(), None, ws.data_ptr(), ws.numel(), s)
        got32 = lib.sot_w1d_backward(ctypes.byref(pf), cot.data_ptr(), stride, 1.0, None, g32.data_ptr(), ws.data_ptr(), ws.numel(), s)
        assert got16 == got32 == want, (got16, got32, want)
        got16 = lib.sot_w1d_loss_and_grad_bf16(ctypes.byref(pr), rows.data_ptr(), float(B), mean.data_ptr(), None, 1.0 / B, g16.data_ptr(), None,
                                               ws.data_ptr(), ws.numel(), s)
        got32 = lib.sot_w1d_loss_and_grad(ctypes.byref(pf), rows.data_ptr(), float(B), mean.data_ptr(), None, 1.0 / B, g32.data_ptr(), None,
                                          ws.data_ptr(), ws.numel(), s)
        assert got16 == got32 == want, (got16, got32, want)

    both(lambda q: setattr(q, "p", 0.5), nat.SOT_ERR_INVALID_P)
    both(lambda q: setattr(q, "B", -1), nat.SOT_ERR_BAD_SHAPE)
    both(lambda q: setattr(q, "x_row_stride", 16), nat.SOT_ERR_BAD_SHAPE)
    both(lambda q: setattr(q, "y", None), nat.SOT_ERR_NULL_POINTER)
    both(lambda q: (setattr(q, "n", 20000), setattr(q, "m", 20000), setattr(q, "x_row_stride", 20000), setattr(q, "y_row_stride", 20000)),
         nat.SOT_ERR_UNSUPPORTED_SIZE)
    pr = nat.make_problem(x16, y16, xpos, ypos, 2.0, PAPER)
    pf = nat.make_problem(x16.float(), y16.float(), xpos, ypos, 2.0, PAPER)
    assert lib.sot_w1d_backward_bf16(ctypes.byref(pr), cot.data_ptr(), 2, 1.0, None, g16.data_ptr(), None, ws.data_ptr(), ws.numel(), s) == \
        lib.sot_w1d_backward(ctypes.byref(pf), cot.data_ptr(), 2, 1.0, None, g32.data_ptr(), ws.data_ptr(), ws.numel(), s) == nat.SOT_ERR_BAD_SHAPE
    assert lib.sot_w1d_backward_bf16(None, cot.data_ptr(), 1, 1.0, None, g16.data_ptr(), None, ws.data_ptr(), ws.numel(), s) == nat.SOT_ERR_NULL_POINTER
    assert lib.sot_w1d_loss_and_grad_bf16(None, rows.data_ptr(), 1.0, mean.data_ptr(), None, 1.0, g16.data_ptr(), None, ws.data_ptr(), ws.numel(), s) == nat.SOT_ERR_NULL_POINTER
    for args in ((None, mean.data_ptr(), g16.data_ptr()), (rows.data_ptr(), None, g16.data_ptr()), (rows.data_ptr(), mean.data_ptr(), None)):
        assert lib.sot_w1d_loss_and_grad_bf16(ctypes.byref(pr), args[0], float(B), args[1], None, 1.0 / B, args[2], None, ws.data_ptr(), ws.numel(), s) == nat.SOT_ERR_NULL_POINTER
    # no workspace where one is needed: the float32 call's answer (the position plan, or the float32 images, need a place)
    assert lib.sot_w1d_backward_bf16(ctypes.byref(pr), cot.data_ptr(), 1, 1.0, None, g16.data_ptr(), None, None, 0, s) == \
        lib.sot_w1d_backward(ctypes.byref(pf), cot.data_ptr(), 1, 1.0, None, g32.data_ptr(), None, 0, s) == nat.SOT_ERR_NULL_POINTER
    for q in (pr, pf):
        q.B = 0
    assert lib.sot_w1d_backward_bf16(ctypes.byref(pr), None, 0, 1.0, None, None, None, None, 0, s) == \
        lib.sot_w1d_backward(ctypes.byref(pf), None, 0, 1.0, None, None, None, 0, s) == 0                      # an empty batch: nothing to do
    assert lib.sot_w1d_loss_and_grad_bf16(ctypes.byref(pr), rows.data_ptr(), 1.0, mean.data_ptr(), None, 1.0, g16.data_ptr(), None, None, 0, s) == \
        lib.sot_w1d_loss_and_grad(ctypes.byref(pf), rows.data_ptr(), 1.0, mean.data_ptr(), None, 1.0, g32.data_ptr(), None, None, 0, s) == nat.SOT_ERR_BAD_SHAPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 6. the module
def _paper_module():
    from sot_amd.losses import Wasserstein1D
    native()
    return Wasserstein1D(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True).to(device())


def _weights16(B, n, seed):
    x, y, _ = rk.make_weights(B, n, n, seed, device())
    return x.to(BF16), y.to(BF16)


def _module_identities(mod, n, kw):
    """the calls of the issue on `mod`: bfloat16 operands against the same calls on their upcast"""
    x16, y16 = _weights16(131, n, 3)
    for weight in (None, 0.37):
        res = []
        for wide in (False, True):
            y = (y16.float() if wide else y16).clone().requires_grad_(True)
            loss = mod(x16.float() if wide else x16, y, **kw)
            (loss if weight is None else weight * loss).backward(retain_graph=True)
            first = y.grad.clone()
            y.grad = None
            (loss if weight is None else weight * loss).backward()       # a second backward through the retained graph
            res.append((loss.detach(), first, y.grad))
        (l16, g16, again16), (l32, g32, again32) = res
        assert l16.dtype is F32 and same_bits32(l16, l32)
        assert g16.dtype is BF16 and same_bits16(g16, g32.to(BF16)), weight
        assert same_bits16(again16, again32.to(BF16)), weight
        assert bool((g16.float() != 0).any())
    # both operands differentiated
    x = x16.clone().requires_grad_(True)
    y = y16.clone().requires_grad_(True)
    xf, yf = x16.float().requires_grad_(True), y16.float().requires_grad_(True)
    l16, l32 = mod(x, y, **kw), mod(xf, yf, **kw)
    (0.37 * l16).backward()
    (0.37 * l32).backward()
    assert same_bits32(l16.detach(), l32.detach())
    assert x.grad.dtype is BF16 and same_bits16(x.grad, xf.grad.to(BF16)) and same_bits16(y.grad, yf.grad.to(BF16))
    # 3-D input, a reduction over one axis under a random cotangent (the row-loss route)
    x3 = x16[:128].reshape(4, 32, n).clone().requires_grad_(True)
    y3 = y16[:128].reshape(4, 32, n).clone().requires_grad_(True)
    xf, yf = x3.detach().float().requires_grad_(True), y3.detach().float().requires_grad_(True)
    out16, out32 = mod(x3, y3, dims=1, **kw), mod(xf, yf, dims=1, **kw)
    assert out16.dtype is F32 and same_bits32(out16.detach(), out32.detach())
    cot = torch.rand(out16.shape, device=device())
    out16.backward(cot)
    out32.backward(cot)
    assert x3.grad.dtype is BF16 and same_bits16(x3.grad, xf.grad.to(BF16)) and same_bits16(y3.grad, yf.grad.to(BF16))
    # row_losses, only y differentiated
    y = y16.clone().requires_grad_(True)
    yf = y16.float().requires_grad_(True)
    r16, r32 = mod.row_losses(x16, y, **kw), mod.row_losses(x16.float(), yf, **kw)
    cot = torch.rand(r16.shape, device=device())
    r16.backward(cot)
    r32.backward(cot)
    assert same_bits32(r16.detach(), r32.detach()) and same_bits16(y.grad, yf.grad.to(BF16))


def _configs():
    from sot_amd.losses import Wasserstein1D
    native()
    pos = torch.linspace(0, 1, 2048, device=device())
    return {"p1_fixed_x_2048": (Wasserstein1D(p=1, fixed_x=2048).to(device()), {}),
            "paper_2048": (_paper_module(), dict(x_pos=pos, y_pos=pos.clone()))}


@pytest.mark.parametrize("config", ["p1_fixed_x_2048", "paper_2048"])
def test_module_training_on_2048_bins_converts_no_row_in_python(config, monkeypatch):
    """Fails on the parent commit, whose bfloat16 calls with a gradient widen their rows and narrow the gradient in Python."""
    from sot_amd import losses
    nat = native()
    mod, kw = _configs()[config]
    x16, y16 = _weights16(8, 2048, 1)
    with torch.no_grad():
        mod(x16.float(), y16.float(), **kw)      # (the float32 module's own warm-up is not what this test is about)
    calls = []
    real_w, real_n = nat.rows_to_f32, nat.rows_to_bf16
    monkeypatch.setattr(nat, "rows_to_f32", lambda *a, **k: (calls.append("rows_to_f32"), real_w(*a, **k))[1])
    monkeypatch.setattr(nat, "rows_to_bf16", lambda *a, **k: (calls.append("rows_to_bf16"), real_n(*a, **k))[1])
    assert losses.nat is nat
    _module_identities(mod, 2048, kw)
    assert calls == [], "a native training call converted rows in Python"
    monkeypatch.setattr(nat, "rows_to_f32", lambda *a, **k: pytest.fail("a native training call widened its rows in Python"))
    monkeypatch.setattr(nat, "rows_to_bf16", lambda *a, **k: pytest.fail("a native training call narrowed its gradient in Python"))
    y = y16.clone().requires_grad_(True)
    mod(x16, y, **kw).backward()
    assert y.grad.dtype is BF16


def test_module_training_takes_the_typed_calls(monkeypatch):
    from sot_amd.losses import Wasserstein1D
    nat = native()
    taken = []
    for name in ("loss_and_grad_bf16", "backward_rows_bf16", "loss_fused_bf16", "forward_rows_bf16", "rows_to_f32", "rows_to_bf16"):
        real = getattr(nat, name)
        monkeypatch.setattr(nat, name, (lambda real, name: lambda *a, **k: (taken.append(name), real(*a, **k))[1])(real, name))
    mod = Wasserstein1D(p=1, fixed_x=2048).to(device())
    x16, y16 = _weights16(67, 2048, 2)
    y = y16.clone().requires_grad_(True)
    mod(x16, y).backward()
    assert taken == ["loss_and_grad_bf16", "backward_rows_bf16"]          # the training step: one node, its backward the fix-up launch
    del taken[:]
    x = x16.clone().requires_grad_(True)
    mod(x, y).backward()
    assert taken == ["loss_fused_bf16", "backward_rows_bf16"]
    del taken[:]
    mod.row_losses(x16, y).sum().backward()
    assert taken == ["forward_rows_bf16", "backward_rows_bf16"]
    # what still widens: 1025 bins, a position that requires a gradient, the tie-free form
    del taken[:]
    paper = _paper_module()
    a16, b16 = _weights16(67, 1025, 22)
    pos = torch.linspace(0, 1, 1025, device=device())
    b = b16.clone().requires_grad_(True)
    paper(a16, b, x_pos=pos, y_pos=pos.clone()).backward()
    assert taken.count("rows_to_f32") == 2 and taken.count("rows_to_bf16") == 1 and "backward_rows_bf16" not in taken
    del taken[:]
    pos = torch.linspace(0, 1, 2048, device=device())
    xp = pos.clone().requires_grad_(True)
    y.grad = None
    paper(x16, y, x_pos=xp, y_pos=pos.clone()).backward()
    assert taken.count("rows_to_f32") == 2 and taken.count("rows_to_bf16") == 1 and "backward_rows_bf16" not in taken
    assert xp.grad is not None and y.grad.dtype is BF16
    del taken[:]
    tie = Wasserstein1D(p=1, fixed_x=2048).to(device())
    tie.tie_free_gradient = True
    mod32 = Wasserstein1D(p=1, fixed_x=2048).to(device())
    mod32.tie_free_gradient = True
    y.grad = None
    yf = y16.float().requires_grad_(True)
    tie(x16, y).backward()
    mod32(x16.float(), yf).backward()
    assert taken.count("rows_to_f32") == 2 and "backward_rows_bf16" not in taken and same_bits16(y.grad, yf.grad.to(BF16))


def test_module_late_gradient_form_matches_too(monkeypatch):
    """EARLY_GRADIENT off: the typed forward + mean, then the typed backward with the float32 late route's arguments"""
    from sot_amd import losses
    native()
    monkeypatch.setattr(losses, "EARLY_GRADIENT", False)
    mod = _paper_module()
    pos = torch.linspace(0, 1, 1024, device=device())
    x16, y16 = _weights16(67, 1024, 8)
    y, yf = y16.clone().requires_grad_(True), y16.float().requires_grad_(True)
    l16, l32 = mod(x16, y, x_pos=pos, y_pos=pos.clone()), mod(x16.float(), yf, x_pos=pos, y_pos=pos.clone())
    (0.37 * l16).backward()
    (0.37 * l32).backward()
    assert same_bits32(l16.detach(), l32.detach()) and same_bits16(y.grad, yf.grad.to(BF16))
