"""-m gpu: ROW OFFSETS PAST 2^31 ELEMENTS AND 2^32 BYTES, on every entry point of include/sot_hip.h that takes a row stride.

The kernels form row addresses in 64 bits (a.x + r * a.xs with int64 strides, a 64-bit row pointer under every buffer descriptor); no other
test holds that in place, because no other test has a row further than a few MiB from its base.  Here every strided input of a call is a
[3, n] view of ONE 16 GiB arena (tests/far_rows.py: first element at arena element 2^31, row stride 2^30 + 4 elements, so row 1 starts
2^32 + 16 bytes and row 2 starts 2^31 + 8 elements from the view's base; x, y and per-row positions side by side in the stride gap).  Every
32-bit reading of such an offset lands inside the arena, on the poison NaN of tests/guarded.py or on row 0's data (tests/test_far_rows.py
proves it in integers), so a kernel that drops a cast reads wrong data without leaving the allocation.

Per line of W1D / STFT_FAR and per test of the other entry points, for each mode:
    1. every output of the call on the far views equals BIT FOR BIT the same call on dense copies of the same three rows -- the layout-S rule
       of tests/test_memory_contract_gpu.py with the same kernel on both sides: the stride is a multiple of 4 and the rows start on 16-byte
       boundaries, so the launch layer's vector test answers as for dense rows, and three rows are three rows (no batch threshold moves);
    2. after the call every word of the arena's poison regions outside the rows is the poison, and the rows hold what was written: inputs are const.

Three rows cannot reach a route behind a batch threshold: at 257 bins the half-wave kernel serves batches from 40960 rows, which at this
stride would be 160 TiB, so the 257-bin line runs the full kernel and the half-wave family is represented by the merge-free 129-bin kernel,
which has no threshold (csrc/sot_full_fwd.hip: dispatch_area_full).  The one-wave-per-frame STFT kernels (from 3072 frames / 1024 frame groups) are out of a
three-clip batch's reach for the same reason; test_dense_* below takes them across 2^31 elements of their outputs instead.

test_dense_*: DENSE buffers that themselves cross 2^31 elements need their real size: the smallest batch with B * n > 2^31.  The ABI refuses
row strides below the row length, so rows cannot overlap inside one tensor; instead x and y are two dense views of ONE buffer of (B + 1) n
values, y[r] = x[r + 1], which halves the inputs and lets them cross 2^31 elements too.  Checked: the last min(CUs, 64) rows or clips equal
the same rows run as a call of their own (bit for bit where the same kernel serves them), and about 40 rows spread over the batch (the
first, the last, those on either side of element 2^31, and a hash-drawn rest) are held to the oracle / torch in float64 at the project's
bounds.

Every test asks torch.cuda.mem_get_info() first and skips, with the bytes in the reason, only if less than its need plus 2 GiB is free.
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

import far_rows as fr
import row_kinds as rk
import test_memory_contract_gpu as mc
import test_row_loop_gpu as rl
from gpu_util import device, native

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
HEADROOM = 2 * 2 ** 30
ROWS = fr.ROWS
P, ok, stream, same_bits = mc.P, mc.ok, mc.stream, mc.same_bits


def need_memory(nbytes, what):
    free, _ = torch.cuda.mem_get_info()
    print(f"{what}: needs {nbytes} bytes + {HEADROOM} headroom, {free} free")
    if free < nbytes + HEADROOM:
        pytest.skip(f"{what} needs {nbytes} + {HEADROOM} bytes of device memory, {free} are free")


@pytest.fixture(scope="module")
def far():
    native()
    torch.cuda.empty_cache()
    need_memory(fr.Far.bytes_needed(), "the far arena")
    arena = fr.Far(device())
    yield arena
    del arena
    torch.cuda.empty_cache()


class Bufs:
    """The buffers of one call, with the interface of tests/test_memory_contract_gpu.py's Run: `far` given -- every input the ABI takes a row
    stride for is a view of the arena, in the next free slot; far None -- dense copies.  Everything else is a plain tensor."""

    def __init__(self, far=None):
        self.far, self.dev = far, device()
        self.inputs, self.outputs, self.placed, self.keep = {}, {}, {}, []
        if far is not None:
            far.clear()

    def inp(self, name, t, strided=False, align=None):
        if name in self.inputs:
            return self.inputs[name]
        if self.far is not None and strided and t.ndim == 2:
            k = len(self.placed)
            view = self.far.place(k, t)
            assert view.stride() == (fr.STRIDE, 1) and view.data_ptr() % 16 == 0
            self.placed[k] = t
        else:
            view = t.contiguous().clone()
        self.inputs[name] = view
        return view

    def out(self, name, shape, dtype=F32, init=None, **_):
        view = torch.empty(shape, dtype=dtype, device=self.dev) if init is None else init.contiguous().clone()
        self.outputs[name] = view
        return view

    def ws(self, nbytes, align=4, claim=None):
        nbytes = int(nbytes)
        if nbytes == 0:
            return None, 0
        view = torch.empty(nbytes, dtype=U8, device=self.dev)
        self.keep.append(view)
        return view.data_ptr(), int(claim or nbytes)

    def finish(self):
        torch.cuda.synchronize()
        if self.far is not None:
            self.far.assert_poison_outside_rows()
            for k, t in self.placed.items():
                assert same_bits(self.far.rows_of(k).view(t.dtype), t), f"far view {k}: a const input was modified"
        return {k: v.clone() for k, v in self.outputs.items()}


def far_equals_dense(far, what, call, strided_inputs, finite=True):
    """conditions 1 and 2 for one call"""
    a = Bufs(far)
    call(a)
    got = a.finish()
    assert len(a.placed) == strided_inputs, (what, "inputs on the far view", len(a.placed), strided_inputs)
    b = Bufs(None)
    call(b)
    want = b.finish()
    assert set(got) == set(want) and got
    for name in want:
        if finite and want[name].dtype in (F32, F64):
            assert bool(torch.isfinite(want[name]).all()), (what, name, "the dense call is not finite")
        if not same_bits(got[name], want[name]):
            g, w = got[name].double().flatten(), want[name].double().flatten()
            at = torch.nonzero((g != w) & ~(g.isnan() & w.isnan())).flatten()
            raise AssertionError(f"{what}: output {name} on far rows differs from the dense call at {at.numel()} of {g.numel()} elements, first {at[:4].tolist()}, "
                                 f"largest difference {float((g - w).abs().nan_to_num(0.0).max()):.3e}; NaN in the far result: {bool(g.isnan().any())}")


# ---- the SOT row kernels ------------------------------------------------------------------------------------------------------------------
FWD, RT, BWD, HIP, PICK = rl.FWD, rl.RT, rl.BWD, rl.HIP, rl.PICK
Line = collections.namedtuple("Line", "id n m rowpos flags area cite")
# id, n, m, per-row positions, extra flags, merge-free?, the dispatch lines three aligned rows take: forward; backward (both gradients); training form
W1D = [
    Line("merge2048", 2048, 2048, False, 0, False, FWD + ": dispatch_forward_full_pow2 (sot_full_fwd.hpp), <256, 8, 1>; " + BWD + ": dispatch_backward_full_pow2 (sot_full_bwd.hpp), <256, 8, 1, 0, 1>; " + HIP + ": run_backward -> the y-only kernel of the same table"),
    Line("merge1025", 1025, 1025, False, 0, False, FWD + ": dispatch_forward_full, <128, 9, 2, 1025> (3 rows < 6144: two waves per row); " + BWD + ": dispatch_backward_full; " + HIP + ": run_backward -> its y-only kernel"),
    Line("merge_free2048", 2048, 2048, False, 0, True, FWD + ": dispatch_area_full_pow2 (sot_full_fwd.hpp), dispatch_area_full_g<256, 8, 1>; " + BWD + ": dispatch_backward_full_pow2 (sot_full_bwd.hpp); " + HIP + ": run_backward, area -> " + BWD + ": dispatch_area_train, dispatch_area_train_g<256, 8, 1> "
         "(SOT_FLAG_TIE_FREE_GRADIENT; the far rows are 16-byte aligned, so `full` holds as for the dense ones)"),
    Line("half_wave129", 129, 129, False, 0, True, FWD + ": dispatch_area_full, dispatch_area_half<5, 8, 129> (every batch size); " + BWD + ": dispatch_backward_full, <64, 3, 4, 129>"),
    Line("full257", 257, 257, False, 0, False, FWD + ": dispatch_forward_full, <64, 5, 4, 257> (3 rows < 40960: not the half-wave kernel); " + BWD + ": dispatch_backward_full"),
    Line("rt1500", 1500, 1500, False, 0, False, RT + ":15 <192, 8, 1, -1>; csrc/sot_full_rt_bwd.hip:20 <192, 8, 1, -1>"),
    Line("gen300x411", 300, 411, False, rl.NS, False, PICK + " (64, 8), n != m, forward and backward"),
    Line("rp2048", 2048, 2048, True, 0, False, HIP + ": launch_rowpos_sort; " + HIP + ": run_forward -> dispatch_forward_full_rowpos_g<256>; " + HIP + ": run_backward -> dispatch_backward_full_rowpos_g<256>"),
    Line("rp700", 700, 700, True, 0, False, HIP + ": launch_rowpos_sort; " + HIP + ": run_forward, dispatch_forward<true>, " + HIP + ": run_backward, dispatch_backward<true>, " + PICK + " (128, 12)"),
]
W1D_BY_ID = {ln.id: ln for ln in W1D}


def modes(line):
    if line.area:
        return (("p1_area", 1.0, 8 | line.flags),)
    label, p, flags = rk.MODES[1]
    return (("p1", 1.0, 8 | line.flags | mc.NO_AREA), (label, p, flags | line.flags))


def as_case(line):
    return rl.C(line.id, "fwd", line.n, 0, 0, line.cite, m=line.m, rowpos=line.rowpos)


@pytest.mark.parametrize("name", [ln.id for ln in W1D])
def test_w1d_forward_backward_loss_and_training_form(far, name):
    """sot_w1d_forward, sot_w1d_backward, sot_w1d_loss_and_grad, sot_w1d_loss"""
    nat, line = native(), W1D_BY_ID[name]
    lib, case = nat.load(), as_case(line)
    inp = mc.sot_batch(ROWS, line.n, line.m, line.rowpos)
    B, n, m = ROWS, line.n, line.m
    strided = 4 if line.rowpos else 2
    for label, p, flags in modes(line):
        def forward(run):
            pr, ws, ws_n = mc.sot_problem(run, nat, case, inp, p, flags)
            if line.area:
                assert pr.flags & mc.SAME_GRID
            rows = run.out("row_loss", (B,))
            ok(nat, lib.sot_w1d_forward(ctypes.byref(pr), rows.data_ptr(), ws, ws_n, stream(nat)))

        def backward(run):
            pr, ws, ws_n = mc.sot_problem(run, nat, case, inp, p, flags)
            g = run.inp("g", inp["g"])
            gx, gy = run.out("gx", (B, n)), run.out("gy", (B, m))
            ok(nat, lib.sot_w1d_backward(ctypes.byref(pr), g.data_ptr(), 1, 0.25, gx.data_ptr(), gy.data_ptr(), ws, ws_n, stream(nat)))

        def train(run, extra=0):
            pr, ws, ws_n = mc.sot_problem(run, nat, case, inp, p, flags | extra)
            rows, mean, total, gy = run.out("row_loss", (B,)), run.out("mean", (1,)), run.out("sum", (1,), F64), run.out("gy", (B, m))
            ok(nat, lib.sot_w1d_loss_and_grad(ctypes.byref(pr), rows.data_ptr(), float(B), mean.data_ptr(), total.data_ptr(), 1.0 / B, gy.data_ptr(), None, ws, ws_n,
                                              stream(nat)))

        def loss(run):
            pr, ws, ws_n = mc.sot_problem(run, nat, case, inp, p, flags)
            rows, mean, total = run.out("row_loss", (B,)), run.out("mean", (1,)), run.out("sum", (1,), F64)
            ok(nat, lib.sot_w1d_loss(ctypes.byref(pr), rows.data_ptr(), float(B), 0, 0.0, mean.data_ptr(), total.data_ptr(), None, ws, ws_n, stream(nat)))

        calls = [("sot_w1d_forward", forward), ("sot_w1d_backward", backward), ("sot_w1d_loss_and_grad", train), ("sot_w1d_loss", loss)]
        if line.area:
            calls.append(("sot_w1d_loss_and_grad, tie-free", lambda run: train(run, mc.TIE_FREE)))
        for entry, call in calls:
            far_equals_dense(far, f"{line.id} {label} {entry}", call, strided)


@pytest.mark.parametrize("rowpos", [False, True], ids=["shared", "rowpos"])
def test_quantiles_and_their_backward(far, rowpos):
    """sot_w1d_quantiles, sot_w1d_quantiles_backward at 300 points: csrc/sot_hip.hip: sot_w1d_quantiles, run_forward(quant) and csrc/sot_quantgrad.hip:239, pick_cfg (64, 8)"""
    nat = native()
    lib, B, n, m = nat.load(), ROWS, 300, 300
    case = rl.C("quant300", "quant", n, 0, 0, "", rowpos=rowpos)
    inp = mc.sot_batch(B, n, m, rowpos)
    strided = 4 if rowpos else 2
    for label, p, flags in (("p1", 1.0, 8), rk.MODES[1]):
        def quant(run):
            pr, ws, ws_n = mc.sot_problem(run, nat, case, inp, p, flags)
            outs = [run.out(k, (B, w)) for k, w in zip(("uq", "vq", "Q", "U", "V"), (n + m, n + m, n + m, n, m))]
            ok(nat, lib.sot_w1d_quantiles(ctypes.byref(pr), *[o.data_ptr() for o in outs], ws, ws_n, stream(nat)))

        def quant_bwd(run):
            pr, ws, ws_n = mc.sot_problem(run, nat, case, inp, p, flags)
            ups = [run.inp(f"up{k}", u) for k, u in enumerate(inp["ups"])]
            outs = [run.out(k, (B, w)) for k, w in zip(("gx", "gy", "gxp", "gyp"), (n, m, n, m))]
            ok(nat, lib.sot_w1d_quantiles_backward(ctypes.byref(pr), *[u.data_ptr() for u in ups], *[o.data_ptr() for o in outs], ws, ws_n, stream(nat)))
        far_equals_dense(far, f"quantiles {label}", quant, strided)
        far_equals_dense(far, f"quantiles_backward {label}", quant_bwd, strided)


@pytest.mark.parametrize("rowpos", [False, True], ids=["shared", "rowpos"])
def test_position_grad(far, rowpos):
    """sot_w1d_position_grad at 300 points: csrc/sot_posgrad.hip:202 setup_launch, pick_cfg (64, 8)"""
    nat = native()
    lib, B, n, m = nat.load(), ROWS, 300, 300
    case = rl.C("posgrad300", "posgrad", n, 0, 0, "", rowpos=rowpos)
    inp = mc.sot_batch(B, n, m, rowpos)
    for label, p, flags in (("p1", 1.0, 8), rk.MODES[1]):
        def call(run):
            pr, ws, ws_n = mc.sot_problem(run, nat, case, inp, p, flags)
            g = run.inp("g", inp["g"])
            gxp, gyp = run.out("gxp", (B, n)), run.out("gyp", (B, m))
            ok(nat, lib.sot_w1d_position_grad(ctypes.byref(pr), g.data_ptr(), 1, 0.25, gxp.data_ptr(), gyp.data_ptr(), ws, ws_n, stream(nat)))
        far_equals_dense(far, f"position_grad {label}", call, 4 if rowpos else 2)


@pytest.mark.parametrize("rows_on_x", [False, True], ids=["rows_on_y", "rows_on_x"])
def test_mixed_supports(far, rows_on_x):
    """sot_w1d_mixed_forward / _backward / _position_grad: csrc/sot_mixed.hip:508 dispatch_mixed_g<., 64, 8> (257 x 37) and :509 <., 128, 12> (37 x 1025);
    x, y and the per-row side's positions are far views, the shared grid has no stride"""
    nat = native()
    lib, B = nat.load(), ROWS
    n, m = (37, 1025) if rows_on_x else (257, 37)
    K = n if rows_on_x else m
    inp = mc.mixed_batch(B, n, m, rows_on_x)
    for label, p, flags in (("p1", 1.0, 8), rk.MODES[1]):
        def fwd(run):
            pr, ws, ws_n = mc.mixed_call(run, nat, inp, p, flags)
            assert (pr.xpos_row_stride == 0) != (pr.ypos_row_stride == 0)
            rows = run.out("row_loss", (B,))
            ok(nat, lib.sot_w1d_mixed_forward(ctypes.byref(pr), rows.data_ptr(), ws, ws_n, stream(nat)))

        def bwd(run):
            pr, ws, ws_n = mc.mixed_call(run, nat, inp, p, flags)
            g = run.inp("g", inp["g"])
            gx, gy = run.out("gx", (B, n)), run.out("gy", (B, m))
            ok(nat, lib.sot_w1d_mixed_backward(ctypes.byref(pr), g.data_ptr(), 1, 0.25, gx.data_ptr(), gy.data_ptr(), ws, ws_n, stream(nat)))

        def posgrad(run):
            pr, ws, ws_n = mc.mixed_call(run, nat, inp, p, flags)
            g = run.inp("g", inp["g"])
            gpos = run.out("gpos", (B, K))
            ok(nat, lib.sot_w1d_mixed_position_grad(ctypes.byref(pr), g.data_ptr(), 1, 0.25, gpos.data_ptr(), ws, ws_n, stream(nat)))
        for entry, call in (("sot_w1d_mixed_forward", fwd), ("sot_w1d_mixed_backward", bwd), ("sot_w1d_mixed_position_grad", posgrad)):
            far_equals_dense(far, f"{entry} {label}", call, 3)


def test_forward_csr_with_offsets_past_2_31(far):
    """sot_w1d_forward_csr (csrc/sot_csr.hip:39 pick_cfg (64, 8) of (max_n, max_m) = (300, 411)): the CSR arrays ARE the far views' memory -- the
    base pointers are the views' first elements, x_offsets / y_offsets name rows 0, 1, 2 at 0, 2^30 + 4 and 2^31 + 8.  CSR rows are adjacent by
    definition, so the stretch between two true rows is a row of its own, far longer than max_n: the header gives it NaN ("every row needs
    1 <= length <= max_n, otherwise its loss is NaN") and the kernel reads one element of it (csrc/sot_rows.hpp:656 bad_row: lengths 1), the
    poison word behind the true row.  Five CSR rows, of which 0, 2, 4 are compared; the dense call has junk rows of max_n + 1 entries."""
    nat = native()
    lib, n, m = nat.load(), 300, 411
    inp = mc.sot_batch(ROWS, n, m, True)
    lens_x, lens_y = [n, 217, 1], [m - 5, m, 64]

    def offsets(lens, stride):
        off = [0]
        for r, k in enumerate(lens):
            off += [r * stride + k] + ([(r + 1) * stride] if r + 1 < len(lens) else [])
        return torch.tensor(off, dtype=I64, device=device())

    for label, p, flags in (("p1", 1.0, 8), rk.MODES[1]):
        def call(run):
            views = [run.inp(k, inp[k], strided=True) for k in ("x", "xpos", "y", "ypos")]
            if run.far is not None:
                stride_x = stride_y = fr.STRIDE
                ptrs = [v.data_ptr() for v in views]
            else:       # dense: rows max_n + 1 apart, the last entry of each stretch is the junk row's
                stride_x, stride_y = 2 * n + 1, 2 * m + 1
                packed = []
                for v, stride in zip(views, (stride_x, stride_x, stride_y, stride_y)):
                    flat = torch.zeros(3 * stride, device=device())
                    flat.view(I32).fill_(fr.POISON)
                    for r in range(ROWS):
                        flat[r * stride:r * stride + v.shape[1]] = v[r]
                    packed.append(flat)
                run.keep += packed
                ptrs = [t.data_ptr() for t in packed]
            xoff, yoff = offsets(lens_x, stride_x), offsets(lens_y, stride_y)
            run.keep += [xoff, yoff]
            assert run.far is None or (int(xoff[4]) == 2 ** 31 + 8 and int(xoff[2]) * 4 == 2 ** 32 + 16)
            rows = run.out("row_loss", (5,))
            ok(nat, lib.sot_w1d_forward_csr(ptrs[0], ptrs[1], xoff.data_ptr(), int(xoff[-1]), ptrs[2], ptrs[3], yoff.data_ptr(), int(yoff[-1]), 5, n, m, float(p), int(flags),
                                            rows.data_ptr(), stream(nat)))
        a, b = Bufs(far), Bufs(None)
        call(a)
        call(b)
        got, want = a.finish()["row_loss"], b.finish()["row_loss"]
        assert bool(torch.isnan(got[1::2]).all()) and bool(torch.isnan(want[1::2]).all()), "over-long rows give NaN"
        assert bool(torch.isfinite(want[0::2]).all()) and same_bits(got[0::2], want[0::2]), (label, got, want)
        dense = nat.forward_rows_csr(*rl.csr_of(dict(inp, xlen=torch.tensor(lens_x, device=device()), ylen=torch.tensor(lens_y, device=device()))), n, m, p, flags)
        assert same_bits(want[0::2], dense), "the five-row dense call differs from the three true rows alone"


@pytest.mark.parametrize("n,cite", [(100, HIP + ": sot_segmented_sort, launch_segmented_sort_wave<2>"), (2048, HIP + ": sot_segmented_sort, launch_segmented_sort_wave<32>"),
                                    (3000, HIP + ": sot_segmented_sort, sot_segmented_sort_kernel")], ids=["100", "2048", "3000"])
def test_segmented_sort(far, n, cite):
    nat = native()
    keys, _ = rk.make_positions(ROWS, n, 100 + n, device())

    def call(run):
        k = run.inp("keys", keys, strided=True)
        vals, idx = run.out("sorted_keys", (ROWS, n)), run.out("indices", (ROWS, n), I64)
        ok(nat, nat.load().sot_segmented_sort(k.data_ptr(), ROWS, n, k.stride(0), vals.data_ptr(), idx.data_ptr(), stream(nat)))
    far_equals_dense(far, f"sot_segmented_sort {n}", call, 1)
    want_v, want_i = torch.sort(keys, dim=1, stable=True)
    run = Bufs(far)
    call(run)
    got = run.finish()
    assert torch.equal(got["sorted_keys"], want_v) and torch.equal(got["indices"], want_i)


def test_column_sum(far):
    """sot_column_sum: csrc/sot_posgrad.hip:237 run_column_sum"""
    nat = native()
    rows = torch.randn(ROWS, 300, generator=torch.Generator(device=device()).manual_seed(300), device=device())

    def call(run):
        r = run.inp("rows", rows, strided=True)
        out = run.out("out", (300,))
        ok(nat, nat.load().sot_column_sum(r.data_ptr(), ROWS, 300, r.stride(0), out.data_ptr(), stream(nat)))
    far_equals_dense(far, "sot_column_sum", call, 1)


# ---- the signal objects -------------------------------------------------------------------------------------------------------------------
STFT = mc.STFT
STFT_FAR = {   # name: (n_fft, hop, samples, forward dispatch, backward dispatch) for three clips
    "slot512": (512, 128, 3001, STFT + " pick_forward_route -> slot: stft_mag_forward_kernel<8>", STFT + " pick_backward_route -> recomputing slot: partial_kernel<8> + overlap-add / slot from spectrum: spec_kernel<8>"),
    "persistent2048": (2048, 512, 5000, STFT + " pick_forward_route: 30 frames < 512 -> persistent slot", STFT + " pick_backward_route -> recomputing slot: partial_kernel<10> / slot from spectrum: spec_kernel<10>"),
    "wavew2048": (2048, 256, 256 * 172 - 17, STFT + " pick_forward_route: 512 <= 516 frames < 3072 -> wavew", STFT + " pick_backward_route -> the slot routes (258 groups < 1024: not wave2)"),
}


@pytest.mark.parametrize("geo", list(STFT_FAR))
def test_stft_forward_and_backward(far, geo):
    """sot_stft_mag_forward[_pair][_spec], sot_stft_mag_backward[_spec] on audio_row_stride"""
    nat = native()
    lib, dev = nat.load(), device()
    n_fft, hop, samples, _, _ = STFT_FAR[geo]
    a_t, b_t = mc.audio_batch(ROWS, samples, n_fft + hop)
    window = torch.hann_window(n_fft, device=dev)
    frames, bins = int(lib.sot_stft_frames(samples, hop)), n_fft // 2 + 1
    if geo == "wavew2048":
        assert 512 <= ROWS * frames < 3072
    gm_t = torch.randn(ROWS, frames, bins, generator=torch.Generator(device=dev).manual_seed(frames), device=dev)
    scale, base = torch.tensor([0.75], device=dev), b_t
    spec_t = nat.stft_mag_forward(a_t, window, n_fft, hop, want_spec=True)[1]
    nbytes = int(lib.sot_stft_backward_workspace_bytes(ROWS, samples, n_fft, hop))

    def forward(pair, want_spec):
        def call(run):
            a, w = run.inp("audio_a", a_t, strided=True), run.inp("window", window)
            mag = run.out("mag", ((2 if pair else 1) * ROWS, frames, bins))
            spec = run.out("spec", (ROWS, frames, bins, 2)) if want_spec else None
            if pair:
                b = run.inp("audio_b", b_t, strided=True)
                if want_spec:
                    rc = lib.sot_stft_mag_forward_pair_spec(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), ROWS, samples, w.data_ptr(), n_fft, hop, mag.data_ptr(), spec.data_ptr(), stream(nat))
                else:
                    rc = lib.sot_stft_mag_forward_pair(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), ROWS, samples, w.data_ptr(), n_fft, hop, mag.data_ptr(), stream(nat))
            elif want_spec:
                rc = lib.sot_stft_mag_forward_spec(a.data_ptr(), ROWS, samples, a.stride(0), w.data_ptr(), n_fft, hop, mag.data_ptr(), spec.data_ptr(), stream(nat))
            else:
                rc = lib.sot_stft_mag_forward(a.data_ptr(), ROWS, samples, a.stride(0), w.data_ptr(), n_fft, hop, mag.data_ptr(), stream(nat))
            ok(nat, rc)
        return call

    def backward(from_spec, acc):
        def call(run):
            a, w = run.inp("audio", a_t, strided=True), run.inp("window", window)
            gm, sc = run.inp("grad_mag", gm_t), run.inp("grad_scale", scale)
            sp = run.inp("spec", spec_t) if from_spec else None
            ga = run.out("grad_audio", (ROWS, samples), init=base if acc else None)
            ws, ws_n = run.ws(nbytes)
            if from_spec:
                rc = lib.sot_stft_mag_backward_spec(a.data_ptr(), sp.data_ptr(), ROWS, samples, a.stride(0), w.data_ptr(), n_fft, hop, gm.data_ptr(), sc.data_ptr(), ga.data_ptr(), acc, ws, ws_n, stream(nat))
            else:
                rc = lib.sot_stft_mag_backward(a.data_ptr(), ROWS, samples, a.stride(0), w.data_ptr(), n_fft, hop, gm.data_ptr(), sc.data_ptr(), ga.data_ptr(), acc, ws, ws_n, stream(nat))
            ok(nat, rc)
        return call

    for pair in (False, True):
        for want_spec in (False, True):
            far_equals_dense(far, f"stft forward {geo} pair={pair} spec={want_spec}", forward(pair, want_spec), 2 if pair else 1)
    for from_spec in (False, True):
        for acc in (0, 1):
            far_equals_dense(far, f"stft backward {geo} spec={from_spec} accumulate={acc}", backward(from_spec, acc), 1)


MSS_SIZES = mc.MSS_SIZES


def _mss_inputs(run, samples):
    t_t, v_t = mc.audio_batch(ROWS, samples, samples)
    t, v = run.inp("target", t_t, strided=True), run.inp("value", v_t, strided=True)
    wins = [run.inp(f"window{s}", torch.hann_window(s, device=device())) for s in MSS_SIZES]
    csizes = (ctypes.c_int * len(MSS_SIZES))(*MSS_SIZES)
    wptr = (ctypes.c_void_p * len(MSS_SIZES))(*[w.data_ptr() for w in wins])
    run.keep += [csizes, wptr]
    return t, v, csizes, wptr


@pytest.mark.parametrize("per_clip", [0, 1])
@pytest.mark.parametrize("samples", [3000, 5000], ids=["one_chunk", "two_chunks"])
def test_mss_loss_and_grad(far, samples, per_clip):
    """sot_mss_loss_and_grad on target_row_stride and value_row_stride (csrc/sot_mss.hip: 4096-sample chunks per (scale, clip))"""
    nat = native()
    lib = nat.load()

    def call(run):
        t, v, csizes, wptr = _mss_inputs(run, samples)
        nbytes = lib.sot_mss_workspace_bytes(ROWS, samples, ctypes.cast(csizes, ctypes.c_void_p), 3)
        loss, grad = run.out("loss", (ROWS,) if per_clip else (1,)), run.out("grad", (ROWS, samples))
        ws, ws_n = run.ws(nbytes)
        ok(nat, lib.sot_mss_loss_and_grad(t.data_ptr(), t.stride(0), v.data_ptr(), v.stride(0), ROWS, samples, ctypes.cast(csizes, ctypes.c_void_p),
                                          ctypes.cast(wptr, ctypes.c_void_p), 3, 1.0, 1.0, 1e-5, 0, per_clip, 0.5, loss.data_ptr(), grad.data_ptr(), ws, ws_n, stream(nat)))
    far_equals_dense(far, f"sot_mss_loss_and_grad {samples} per_clip={per_clip}", call, 2)


@pytest.mark.parametrize("per_clip", [0, 1])
def test_spec_metrics(far, per_clip):
    """sot_spec_metrics on both strides (csrc/sot_mss.hip: metric mode, two groups on a union of three sizes)"""
    nat = native()
    lib, samples = nat.load(), 5000
    groups = [((64, 512), 1.0, 1.0, 0.0, False), ((2048, 512), 0.0, 0.0, 1.0, True)]

    def call(run):
        t, v, csizes, wptr = _mss_inputs(run, samples)
        grp = (nat.SotMetricGroup * 2)()
        for i, (gs, mag_w, log_w, lsd_w, l2) in enumerate(groups):
            grp[i].n_sizes = len(gs)
            for j, s in enumerate(gs):
                grp[i].fft_sizes[j] = s
            grp[i].mag_weight, grp[i].logmag_weight, grp[i].lsd_weight, grp[i].l2 = mag_w, log_w, lsd_w, int(l2)
        run.keep.append(grp)
        nbytes = lib.sot_spec_metrics_workspace_bytes(ROWS, samples, ctypes.cast(csizes, ctypes.c_void_p), 3, 2)
        out = run.out("out", (ROWS, 2) if per_clip else (2,))
        ws, ws_n = run.ws(nbytes)
        ok(nat, lib.sot_spec_metrics(t.data_ptr(), t.stride(0), v.data_ptr(), v.stride(0), ROWS, samples, ctypes.cast(csizes, ctypes.c_void_p),
                                     ctypes.cast(wptr, ctypes.c_void_p), 3, ctypes.cast(grp, ctypes.c_void_p), 2, 1e-5, per_clip, out.data_ptr(), ws, ws_n, stream(nat)))
    far_equals_dense(far, f"sot_spec_metrics per_clip={per_clip}", call, 2)


@pytest.mark.parametrize("samples", [1024, 1025])
def test_fir(far, samples):
    """sot_fir_same_forward / _backward on audio_row_stride and taps_row_stride (csrc/sot_fir.hip: one full tile; SOT_FIR_TILE + 1), taps per clip"""
    nat = native()
    lib, dev, n_taps, start = nat.load(), device(), 128, 62
    gen = torch.Generator(device=dev).manual_seed(samples)
    audio_t, grad_t = torch.randn(ROWS, samples, generator=gen, device=dev), torch.randn(ROWS, samples, generator=gen, device=dev)
    taps_t = torch.randn(ROWS, n_taps, generator=gen, device=dev)
    nbytes = int(lib.sot_fir_workspace_bytes(ROWS, samples, n_taps))

    def fwd(run):
        a, t = run.inp("audio", audio_t, strided=True), run.inp("taps", taps_t, strided=True)
        out = run.out("out", (ROWS, samples))
        ok(nat, lib.sot_fir_same_forward(a.data_ptr(), a.stride(0), t.data_ptr(), t.stride(0), ROWS, samples, n_taps, start, out.data_ptr(), stream(nat)))

    def bwd(run):
        a, t = run.inp("audio", audio_t, strided=True), run.inp("taps", taps_t, strided=True)
        g = run.inp("grad_out", grad_t)
        ga, gt = run.out("grad_audio", (ROWS, samples)), run.out("grad_taps", (ROWS, n_taps))
        ws, ws_n = run.ws(nbytes)
        ok(nat, lib.sot_fir_same_backward(g.data_ptr(), a.data_ptr(), a.stride(0), t.data_ptr(), t.stride(0), ROWS, samples, n_taps, start, ga.data_ptr(), gt.data_ptr(),
                                          ws, ws_n, stream(nat)))
    far_equals_dense(far, f"sot_fir_same_forward {samples}", fwd, 2)
    far_equals_dense(far, f"sot_fir_same_backward {samples}", bwd, 2)


# ---- dense buffers that themselves cross 2^31 elements -------------------------------------------------------------------------------------
def rows_past_2_31(n):
    """the smallest batch whose dense [B, n] float32 buffer has more than 2^31 elements"""
    B = 2 ** 31 // n + 1
    assert B * n > 2 ** 31 >= (B - 1) * n
    return B


def sample_rows(B, n):
    """about 40 rows: the first, the last, the rows around element 2^31 of a dense [B, n] buffer, and a hash-drawn rest"""
    edge = 2 ** 31 // n
    picks = torch.cat([torch.tensor([0, 1, B - 2, B - 1, edge - 2, edge - 1, edge]), rk.row_hash(torch.arange(33, dtype=I64), 0xFA5) % B])
    return torch.unique(picks.clamp(0, B - 1))


def shifted_pair(B, n, seed):
    """x [B, n] and y [B, n] with y[r] = x[r + 1]: two dense views (row stride n, which is what the ABI accepts) of ONE buffer of (B + 1) n
    values, so the inputs cost one allocation -- and cross 2^31 elements themselves"""
    flat = torch.rand((B + 1) * n, generator=torch.Generator(device=device()).manual_seed(seed), device=device())
    return flat[:B * n].view(B, n), flat[n:].view(B, n)


def ends_count():
    return min(rl.cus(), 64)


def free_memory():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("tie_free", [False, True], ids=["merge_walk", "merge_free"])
def test_dense_loss_and_grad_2048(tie_free):
    """sot_w1d_loss_and_grad, p = 1 on one grid, n = m = 2048, B = 2^20 + 1: grad_y has 2^31 + 2048 elements (csrc/sot_hip.hip: run_backward ->
    csrc/sot_full_bwd.hpp: dispatch_backward_full_pow2, and with SOT_FLAG_TIE_FREE_GRADIENT `area` -> csrc/sot_full_bwd.hip: dispatch_area_train).  Both kernels are chosen by the row length
    alone, so the last rows as a call of their own are held bit for bit."""
    from oracle import sot_oracle as so
    nat = native()
    n, B = 2048, rows_past_2_31(2048)
    assert B == 2 ** 20 + 1
    need_memory(((B + 1) * n + B * n) * 4, "2048-bin training form past 2^31 elements")
    case = rl.BY_ID["tiefree2048" if tie_free else "train2048"]
    x, y = shifted_pair(B, n, 2048)
    pos = torch.linspace(0, 1, n, device=device())
    inp = dict(x=x, y=y, xpos=pos, ypos=pos, plan=nat.PositionPlan(pos, pos))
    flags = 8 | (nat.FLAG_TIE_FREE_GRADIENT if tie_free else nat.FLAG_NO_AREA)
    rows, gy = rl.call_loss_and_grad(nat, inp, 1.0, flags)
    assert gy.numel() > 2 ** 31 and bool(torch.isfinite(rows).all()) and bool(torch.isfinite(gy[-4096:]).all())
    c = ends_count()
    rows_c, gy_c = rl.call_loss_and_grad(nat, dict(inp, x=x[B - c:], y=y[B - c:]), 1.0, flags)
    assert torch.equal(rows[B - c:], rows_c) and torch.equal(gy[B - c:], gy_c), "the last rows alone differ"
    s = sample_rows(B, n).to(device())
    xc, yc, pc = x[s].cpu().numpy(), y[s].cpu().numpy(), pos.cpu().numpy()
    want, dbg = so.forward(xc, yc, pc, pc, p=1.0, flags=8, debug=True)
    rl.assert_forward(case, "p1", rows[s].cpu().numpy(), want)
    _, wy = so.backward(xc, yc, pc, pc, np.full(len(s), rl.TRAIN_GRAD_SCALE, np.float32), p=1.0, flags=8)
    got = gy[s].cpu().numpy()
    if tie_free:     # the oracle is the yardstick on rows without exactly tied levels (tests/test_row_loop_gpu.py: test_training_form)
        keep = ~(dbg["Q"][:, 1:] == dbg["Q"][:, :-1]).any(1)
        print(f"{int(keep.sum())} of {len(keep)} sample rows tie-free")
        assert 4 * int(keep.sum()) >= len(keep)
        got, wy = got[keep], wy[keep]
    rl.assert_gradient(case, "p1 gy", got, wy, 1e-5)
    del x, y, rows, gy, inp
    free_memory()


def test_dense_backward_generic_300():
    """sot_w1d_backward on the generic kernel (SOT_FLAG_NO_SPECIALIZE, csrc/sot_launch.hpp: pick_cfg (64, 8)), n = m = 300, grad_y only: the
    smallest batch with B * 300 > 2^31.  The geometry depends on the lengths alone: the last rows alone bit for bit."""
    from oracle import sot_oracle as so
    nat = native()
    n = 300
    B = rows_past_2_31(n)
    need_memory(((B + 1) * n + B * n + B) * 4, "generic backward past 2^31 elements")
    case = rl.BY_ID["bwd_gen300x411"]
    x, y = shifted_pair(B, n, 300)
    pos = torch.linspace(0, 1, n, device=device())
    plan = nat.PositionPlan(pos, pos)
    g = 0.5 + torch.rand(B, generator=torch.Generator(device=device()).manual_seed(B), device=device())
    c = ends_count()
    s = sample_rows(B, n).to(device())
    xc, yc, pc = x[s].cpu().numpy(), y[s].cpu().numpy(), pos.cpu().numpy()
    for label, p, oflags in (rk.MODES[0], rk.MODES[1]):
        flags = oflags | rl.NS | (nat.FLAG_NO_AREA if p == 1.0 else 0)
        gx, gy = nat.backward_rows(x, y, pos, pos, p, flags, g, need_gx=False, plan=plan, grad_scale=0.25)
        assert gx is None and gy.numel() > 2 ** 31
        _, gy_c = nat.backward_rows(x[B - c:], y[B - c:], pos, pos, p, flags, g[B - c:], need_gx=False, plan=plan, grad_scale=0.25)
        assert torch.equal(gy[B - c:], gy_c), (label, "the last rows alone differ")
        _, wy = so.backward(xc, yc, pc, pc, (0.25 * g[s]).cpu().numpy(), p=p, flags=oflags)
        rl.assert_gradient(case, f"{label} gy", gy[s].cpu().numpy(), wy, 1e-5)
        del gy
    del x, y
    free_memory()


def test_dense_segmented_sort_2048():
    """sot_segmented_sort, n = 2048, keys only (indices = NULL, which the entry point allows), B = 2^20 + 1 (csrc/sot_hip.hip: sot_segmented_sort,
    launch_segmented_sort_wave<32>, chosen by n alone)"""
    nat = native()
    n, B = 2048, rows_past_2_31(2048)
    need_memory(2 * B * n * 4, "segmented sort past 2^31 elements")
    keys = torch.rand(B, n, generator=torch.Generator(device=device()).manual_seed(5), device=device())
    vals = torch.empty_like(keys)
    lib = nat.load()
    ok(nat, lib.sot_segmented_sort(keys.data_ptr(), B, n, n, vals.data_ptr(), None, stream(nat)))
    c = ends_count()
    alone = torch.empty(c, n, device=device())
    ok(nat, lib.sot_segmented_sort(keys[B - c:].data_ptr(), c, n, n, alone.data_ptr(), None, stream(nat)))
    assert torch.equal(vals[B - c:], alone), "the last rows alone differ"
    s = sample_rows(B, n).to(device())
    assert torch.equal(vals[s], torch.sort(keys[s], dim=1, stable=True).values)
    del keys, vals
    free_memory()


def test_dense_stft_wave2_forward_and_backward():
    """sot_stft_mag_forward, n_fft 2048 / hop 256 on stft_mag_forward_wave2_kernel (csrc/sot_stft.hip pick_forward_route -> wave2), mag only: 17 frames per clip and the
    smallest batch for which mag [clips, 17, 1025] has more than 2^31 elements; then the backward that reads a grad_mag of that size, from the
    stored spectrum on stft_mag_backward_spec_wave2_kernel (pick_backward_route -> wave2 from spectrum: 17 > 16 frames, so not the clip kernel) with the overlap-add behind it.
    The last min(CUs, 64) clips alone run other kernels (pick_forward_route -> wavew, below 3072 frames; pick_backward_route -> slot from spectrum, below 1024 groups):
    1e-6 of the peak forward, 2e-5 of the gradient's peak backward, the bounds of test_one_wave_per_frame_kernels_of_large_batches, which
    also supplies the bounds of the sample: torch.stft -- here in float64 -- within 2e-6 of the peak, the recomputing slot kernel on batches
    of 8 clips within 2e-5 of the gradient's peak."""
    from sot_amd import spectra
    nat = native()
    dev = device()
    n_fft, hop, samples, frames, bins = 2048, 256, 4096 + 77, 17, 1025
    clips = rows_past_2_31(frames * bins)
    groups = (frames + 1) // 2
    need_memory((clips * frames * bins * 4 + 2 * clips * samples + clips * groups * (n_fft + hop)) * 4, "n_fft 2048 STFT past 2^31 elements")
    gen = torch.Generator(device=dev).manual_seed(17)
    a = torch.rand(clips, samples, generator=gen, device=dev) - 0.5
    a[3] = 0.0
    a[5] *= 1e-21
    win = torch.hann_window(n_fft, device=dev)
    mag = nat.stft_mag_forward(a, win, n_fft, hop)
    assert mag.shape == (clips, frames, bins) and mag.numel() > 2 ** 31 and clips * frames >= 3072
    c = ends_count()
    s = sample_rows(clips, frames * bins).to(dev)
    s = torch.unique(torch.cat([s, torch.tensor([3, 5], device=dev)]))
    ref = torch.stft(spectra.end_padded(a[s].double(), n_fft, hop), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=win.double(), center=False,
                     normalized=True, return_complex=True).abs().permute(0, 2, 1)
    peak = float(ref.max())
    assert c * frames < 3072
    alone = nat.stft_mag_forward(a[clips - c:], win, n_fft, hop)
    worst = float((mag[clips - c:] - alone).abs().max()) / peak
    print(f"forward: the last {c} clips alone (wavew kernel) {worst:.2e} of the peak")
    assert worst <= 1e-6
    worst = float((mag[s].double() - ref).abs().max()) / peak
    print(f"forward: {len(s)} sample clips against torch.stft in float64 {worst:.2e} of the peak")
    assert worst <= 2e-6 and float(mag[3].abs().max()) == 0.0
    del mag
    free_memory()
    mag, spec = nat.stft_mag_forward(a, win, n_fft, hop, want_spec=True)
    gm = mag                                            # the upstream gradient: the magnitudes themselves (dL/d mag of sum mag^2 / 2)
    assert clips * groups >= 1024 and frames > 16
    got = nat.stft_mag_backward(a, win, n_fft, hop, gm, spec=spec)
    assert bool(torch.isfinite(got).all()) and float(got[3].abs().max()) == 0.0
    gpeak = float(got.abs().max())
    alone = nat.stft_mag_backward(a[clips - c:], win, n_fft, hop, gm[clips - c:], spec=spec[clips - c:])
    worst = float((got[clips - c:] - alone).abs().max()) / gpeak
    print(f"backward: the last {c} clips alone (slot kernel from the spectrum) {worst:.2e} of the gradient's peak")
    assert worst <= 2e-5
    worst = 0.0
    for i in range(0, len(s), 8):
        at = s[i:i + 8]
        want = nat.stft_mag_backward(a[at], win, n_fft, hop, gm[at])       # the recomputing slot kernel
        worst = max(worst, float((got[at] - want).abs().max()) / gpeak)
    print(f"backward: {len(s)} sample clips against the recomputing slot kernel {worst:.2e} of the gradient's peak")
    assert worst <= 2e-5
    del mag, spec, gm, got, a
    free_memory()
