"""-m gpu: the MEMORY CONTRACT of include/sot_hip.h, straight through the C ABI, with guard bands around every buffer (tests/guarded.py).

The header says: the caller owns every buffer; outputs are dense; a workspace holds *_workspace_bytes() bytes; input rows may sit
row_stride >= n apart; inputs are const; a call that returns an error, or is given an empty batch, touches nothing.  The value tests cannot
see a violation: torch.empty rounds every request up and serves it from a pool, so a store past an output lands in slack.  Here every input,
output and workspace of a call is a view in the middle of an allocation filled with a poison pattern, and the workspace has exactly the bytes
its size function reports.

Every case of CASES runs in the layouts
    A   dense, every base on a 256-byte boundary;
    O   dense, every base 4 bytes off the 16-byte grid (2 for uint16, 8 for int64 / double); a buffer whose alignment the header fixes
        (windows, spec: 8; FIR, metrics workspace: 8; MSS workspace: 16) sits at exactly that alignment and no better;
    S   as O, and every input the ABI takes a stride for has row stride = length + 3 (per-row positions too);
    S4  (per-row-position cases only) bases as A, row stride = length + 4: the packed-word pre-sort on strided rows;
each with the inputs' padding -- bands and row gaps -- once zero and once the poison NaN.  Asserted (exact but for the named exceptions of 6):
    1. after the call every output's and every workspace's guard is untouched;
    2. every output the header defines for every element holds no word of the poison (an early return cannot pass by doing nothing);
    3. every input allocation, padding included, is bit-identical to its copy from before the call;
    4. the zero-padded and the poison-padded run give bit-identical outputs (the calls are documented as deterministic: a result that
       depends on bytes outside its rows differs);
    5. layout A equals the binding's wrapper (nat.forward_rows, ...) on contiguous tensors bit for bit -- where the wrapper returns another
       shape (batch sums of position gradients), the same call on plain torch.empty tensors stands in;
    6. layouts O, S, S4 against A: BIT FOR BIT on every output of every line -- the layouts run the same instantiation, or the scalar-access
       variant of it, which forms the same terms in the same order -- except where the line's `close` column names a layout and the dispatch
       line that sends it to ANOTHER kernel (NOT_BITWISE below: the wave2 STFT backward on a scratch buffer 4 bytes off, the 2048-bin
       merge-free training form on rows 4 bytes off).  Only there: forward values within rtol 2e-6, atol 1e-12 (tests/test_row_loop_gpu.py:
       CLOSE), gradients within 1e-5 of the row's largest entry, sort outputs and permutations still bit for bit;
    7. REFUSALS: per entry point one refused call and one call on an empty batch, outputs and workspace full of the pattern: the documented
       status, and nothing written.

Batches are small: B = 2 ROWS + 1 rows (two row groups, the last one partial); a route that exists only from a batch threshold takes the
threshold + 1 (+ 2 where that leaves no partial group).  A new row kernel or entry point adds a line to CASES (tests/test_workspace_sizes.py
fails when an exported function that enqueues work has none).
"""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded as gd
import row_kinds as rk
import test_guarded as tg
import test_row_loop_gpu as rl
from gpu_util import device, native

pytestmark = pytest.mark.gpu

kFwd1025OneWaveRows = rl.kFwd1025OneWaveRows
CLOSE = rl.CLOSE
GRAD_TOL = 1e-5                # of the row's largest entry ("Tolerances")
NS, SAME_GRID, NO_AREA, TIE_FREE = 32, 64, 128, 256
F32, F64, I32, I64, U16, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint16, torch.uint8

Case = collections.namedtuple("Case", "id entries family n m rows cite lo hi rowpos layouts close extra")

ENTRY_OF = {"fwd": "sot_w1d_forward", "area": "sot_w1d_forward", "fwd_perm": "sot_w1d_forward", "bwd": "sot_w1d_backward",
            "train": "sot_w1d_loss_and_grad", "tiefree": "sot_w1d_loss_and_grad", "posgrad": "sot_w1d_position_grad",
            "quant": "sot_w1d_quantiles", "quantgrad": "sot_w1d_quantiles_backward", "csr": "sot_w1d_forward_csr",
            "sort": "sot_segmented_sort", "fused": "sot_w1d_loss"}
ALL, DENSE = ("A", "O", "S"), ("A", "O")


# The `close` column: layout -> the dispatch line that sends this layout to ANOTHER kernel than layout A's, so that condition 6 is a tolerance there.
# Every layout a line does not name here is held to A bit for bit.
WAVE2_SCRATCH = ("csrc/sot_stft.hip pick_backward_route: wave2 from spectrum needs the scratch rows on 8-byte boundaries: with the workspace 4 bytes off the grid "
                 "stft_mag_backward_spec_kernel<10>, the slot kernel (slot from spectrum), serves the call (another FFT, another association)")
TIE_FREE_2048 = ("csrc/sot_hip.hip: run_backward, `full` needs backward_full_supports(2048, aligned16) and `area` needs `full`: with rows 4 bytes off the grid "
                 ":555 dispatch_backward_full_rt, the merge walk, serves the call -- SOT_FLAG_TIE_FREE_GRADIENT is a permission (include/sot_hip.h)")
NOT_BITWISE = {"tiefree2048": {"O": TIE_FREE_2048, "S": TIE_FREE_2048}}     # for the lines taken over from tests/test_row_loop_gpu.py


def C(id, entries, family, n=None, m=None, rows=None, cite="", lo=0, hi=None, rowpos=False, layouts=None, close=None, **extra):
    entries = (entries,) if isinstance(entries, str) else tuple(entries)
    if layouts is None:
        layouts = ALL + (("S4",) if rowpos else ())
    close = dict(close or NOT_BITWISE.get(id, {}))
    assert set(close) <= set(layouts[1:])
    return Case(id, entries, family, n, n if m is None else m, rows, cite, lo, hi, rowpos, layouts, close, extra)


# ---- the SOT row-kernel routes: the lines of tests/test_row_loop_gpu.py, same lengths, same citations ----
LEFT_OUT = {}      # route id of tests/test_row_loop_gpu.py -> why this file has no line for it (none today)
CASES = [C(c.id, ENTRY_OF[c.family], c.family, c.n, c.m, c.rows, c.cite, c.lo, c.hi, c.rowpos,
           DENSE if c.family == "csr" else None, **c.extra) for c in rl.CASES]
FWD, HIP, PICK = rl.FWD, rl.HIP, rl.PICK
CASES += [
    # the 129-bin full kernel below 8192 rows: tests/test_row_loop_gpu.py cannot force its second row; no second row is needed here
    C("fwd129_full", "sot_w1d_forward", "fwd", 129, rows=4, cite=FWD + ": dispatch_forward_full, <64, 3, 4, 129>, below the 8192-row threshold", hi=rl.kHalf129Rows - 1),
    # odd row lengths in the uint16 image: the y half of a row starts on an odd element, rows are 386 elements
    C("rp129x257_odd_image", "sot_w1d_forward", "fwd_perm", 129, 257, rows=4, cite=HIP + ": setup_launch, row_perm_out / row_perm_in, " + PICK + " (64, 8)", rowpos=True),
    C("rp129x257", "sot_w1d_forward", "fwd", 129, 257, rows=4, cite=HIP + ": launch_rowpos_sort, element-wise stores (n & 3 != 0)", rowpos=True),
    # beyond the pre-sort's domain: sot_workspace_bytes is 0 (csrc/sot_launch.hpp: rowpos_presort_runs), the call takes workspace = NULL, 0
    C("rp2049_no_workspace", "sot_w1d_forward", "fwd", 2049, rows=1, cite=HIP + ": setup_launch, rowpos_presort_runs is false; " + PICK + " (1024, 8)", rowpos=True, no_workspace=True),
    C("bwd_rp2049_no_workspace", "sot_w1d_backward", "bwd", 2049, rows=1, cite=HIP + ": setup_launch; " + PICK + " (1024, 8)", rowpos=True, no_workspace=True),
    # shared positions planned inside the call: the workspace of ws_layout (csrc/sot_launch.hpp), exact
    C("fwd_gen100_plan_in_workspace", "sot_w1d_forward", "fwd", 100, rows=4, cite=HIP + ": setup_launch, launch_prepare into the workspace", flags=NS, plan_in_workspace=True),
    C("bwd513_plan_in_workspace", "sot_w1d_backward", "bwd", 513, rows=4, cite=HIP + ": setup_launch; " + rl.BWD + ": dispatch_backward_full", plan_in_workspace=True),
    C("sort3000", "sot_segmented_sort", "sort", 3000, rows=1, cite=HIP + ": sot_segmented_sort, sot_segmented_sort_kernel (n > 2048: up to 1024 threads per row)"),
    C("loss2048_two_kernels", ("sot_w1d_loss", "sot_w1d_reduce_mean"), "loss", 2048, rows=1, cite=HIP + ": loss_call, forward, then sot_reduce_mean_kernel"),
    C("loss513_hinge", ("sot_w1d_loss", "sot_w1d_reduce_mean"), "loss", 513, rows=4, cite=HIP + ": loss_call, apply_hinge", hinge=0.01),
    C("mixed_fwd_rows_on_y", "sot_w1d_mixed_forward", "mixed_fwd", 257, 37, rows=4, cite="csrc/sot_mixed.hip:508 dispatch_mixed_g<0, 64, 8>; :474 plan in the workspace"),
    C("mixed_fwd_rows_on_x", "sot_w1d_mixed_forward", "mixed_fwd", 37, 1025, rows=2, cite="csrc/sot_mixed.hip:509 <0, 128, 12>", rows_on_x=True),
    C("mixed_bwd_rows_on_y", "sot_w1d_mixed_backward", "mixed_bwd", 257, 37, rows=4, cite="csrc/sot_mixed.hip:508 <1, 64, 8>"),
    C("mixed_bwd_rows_on_x", "sot_w1d_mixed_backward", "mixed_bwd", 37, 1025, rows=2, cite="csrc/sot_mixed.hip:509 <1, 128, 12>", rows_on_x=True),
    C("mixed_posgrad_rows_on_y", "sot_w1d_mixed_position_grad", "mixed_posgrad", 257, 37, rows=4, cite="csrc/sot_mixed.hip:491 <2, 64, 8>"),
    C("mixed_posgrad_rows_on_x", "sot_w1d_mixed_position_grad", "mixed_posgrad", 37, 1025, rows=2, cite="csrc/sot_mixed.hip:491 <2, 128, 12>", rows_on_x=True),
    C("prepare300x411", "sot_prepare_positions", "prepare", 300, 411, cite=HIP + ": launch_prepare, sot_prepare_positions_kernel<false>", layouts=DENSE),
    C("prepare_unit1025", "sot_prepare_unit_positions", "prepare", 1025, cite=HIP + ": launch_prepare, <true>", layouts=DENSE, unit=True),
    C("reduce_mean5", "sot_w1d_reduce_mean", "reduce", 5, cite=HIP + ": sot_w1d_reduce_mean, sot_reduce_mean_kernel, fewer rows than lanes", layouts=DENSE),
    C("reduce_mean4099", "sot_w1d_reduce_mean", "reduce", 4099, cite=HIP + ": sot_w1d_reduce_mean, 16-byte loads on aligned rows, scalar otherwise", layouts=DENSE, hinge=0.3),
    C("scale3", "sot_scale_inplace", "scale", 3, cite=HIP + ": sot_scale_inplace, sot_scale_inplace_kernel, a tail shorter than one vector", layouts=DENSE),
    C("scale4099", "sot_scale_inplace", "scale", 4099, cite=HIP + ": sot_scale_inplace, 16-byte access on aligned data, scalar otherwise", layouts=DENSE),
    C("scale4099_by_one", "sot_scale_inplace", "scale", 4099, cite=HIP + ": sot_scale_inplace, scalar == 1: data is not touched", layouts=DENSE, scalar=1.0),
    C("column_sum9x300", "sot_column_sum", "colsum", 300, rows=None, cite="csrc/sot_posgrad.hip:237 run_column_sum"),
]

# ---- the side kernels: the smallest shape that satisfies each dispatch predicate of csrc/sot_stft.hip ----
STFT = "csrc/sot_stft.hip"
STFT_GEO = {   # name: (n_fft, hop, batch, samples, the predicate)
    "slot64": (64, 16, 3, 1000, STFT + " pick_forward_route -> slot: stft_mag_forward_kernel<5>, the clip ends inside a frame"),
    "slot512": (512, 128, 2, 3001, STFT + " pick_forward_route -> slot: stft_mag_forward_kernel<8>, the clip ends inside a frame"),
    "persistent2048": (2048, 512, 2, 5000, STFT + " pick_forward_route: fewer than 512 frames -> persistent slot"),
    "wavew2048": (2048, 256, 2, 256 * 300 - 17, STFT + " pick_forward_route: 512 <= 600 frames < 3072 -> wavew"),
    "wave2_2048": (2048, 256, 2, 256 * 1600 - 5, STFT + " pick_forward_route: 3200 frames >= 3072 -> wave2"),
}
for geo, (n_fft, hop, batch, samples, cite) in STFT_GEO.items():
    CASES += [
        C(f"stft_fwd_{geo}", "sot_stft_mag_forward", "stft_fwd", cite=cite, geo=geo, pair=False, spec=False),
        C(f"stft_fwd_spec_{geo}", "sot_stft_mag_forward_spec", "stft_fwd", cite=cite, geo=geo, pair=False, spec=True),
        C(f"stft_pair_{geo}", "sot_stft_mag_forward_pair", "stft_fwd", cite=cite, geo=geo, pair=True, spec=False),
        C(f"stft_pair_spec_{geo}", "sot_stft_mag_forward_pair_spec", "stft_fwd", cite=cite, geo=geo, pair=True, spec=True),
    ]
STFT_BWD_GEO = {   # name: (n_fft, hop, batch, samples, from the stored spectrum?, the predicate)
    "audio512": (512, 128, 2, 3001, False, STFT + " pick_backward_route -> recomputing slot: stft_mag_backward_partial_kernel<8> + stft_overlap_add_kernel"),
    "audio2048": (2048, 512, 2, 5000, False, STFT + " pick_backward_route -> recomputing slot: stft_mag_backward_partial_kernel<10>"),
    "spec_slot512": (512, 128, 2, 3001, True, STFT + " pick_backward_route -> slot from spectrum: stft_mag_backward_spec_kernel<8>"),
    "spec_clip2048": (2048, 512, 65, 512 * 6 - 7, True, STFT + " pick_backward_route: 65 >= 64 clips of 6 <= 16 frames, even hop -> clip"),
    "spec_wave2_2048": (2048, 256, 2, 256 * 1600 - 5, True, STFT + " pick_backward_route: 1600 >= 1024 groups, hop 256, 8-byte scratch rows -> wave2 from spectrum"),
    "spec_wave2_hop512": (2048, 512, 2, 512 * 1100 - 5, True, STFT + " pick_backward_route -> wave2 from spectrum, launch_backward_wave2<4> (hop 512): 1100 groups"),
}
for geo, (n_fft, hop, batch, samples, from_spec, cite) in STFT_BWD_GEO.items():
    entry = "sot_stft_mag_backward_spec" if from_spec else "sot_stft_mag_backward"
    close = {"O": WAVE2_SCRATCH, "S": WAVE2_SCRATCH} if "wave2" in geo else None
    CASES += [C(f"stft_bwd_{geo}", entry, "stft_bwd", cite=cite, close=close, geo=geo, accumulate=0),
              C(f"stft_bwd_{geo}_accumulate", entry, "stft_bwd", cite=cite, close=close, geo=geo, accumulate=1)]
MSS, OSC, FIR = "csrc/sot_mss.hip", "csrc/sot_osc.hip", "csrc/sot_fir.hip"
CASES += [
    C("dist_fwd_1000", "sot_spec_distance_forward", "dist_fwd", 1000, cite="csrc/sot_spec_distance.hip sot_spec_distance_forward: four partial blocks", layouts=DENSE, accumulate=0, l2=0),
    C("dist_fwd_262921_accumulate", "sot_spec_distance_forward", "dist_fwd", 262144 + 777, cite="csrc/sot_spec_distance.hip sot_spec_distance_forward: n_partial capped at kDistBlocks", layouts=DENSE, accumulate=1, l2=1),
    C("dist_bwd_1000", "sot_spec_distance_backward", "dist_bwd", 1000, cite="csrc/sot_spec_distance.hip sot_spec_distance_backward: spec_distance_backward_kernel", layouts=DENSE, l2=0),
    C("dist_bwd_262921", "sot_spec_distance_backward", "dist_bwd", 262144 + 777, cite="csrc/sot_spec_distance.hip sot_spec_distance_backward", layouts=DENSE, l2=1),
    C("dist_rows_fwd_5x1300", "sot_spec_distance_rows_forward", "dist_rows_fwd", 1300, rows=None, cite="csrc/sot_spec_distance.hip sot_spec_distance_rows_forward: one 1024-thread workgroup per row", layouts=DENSE, accumulate=0, l2=0),
    C("dist_rows_fwd_5x1300_accumulate", "sot_spec_distance_rows_forward", "dist_rows_fwd", 1300, rows=None, cite="csrc/sot_spec_distance.hip sot_spec_distance_rows_forward", layouts=DENSE, accumulate=1, l2=1),
    C("dist_rows_bwd_5x1300", "sot_spec_distance_rows_backward", "dist_rows_bwd", 1300, rows=None, cite="csrc/sot_spec_distance.hip sot_spec_distance_rows_backward: spec_distance_rows_backward_kernel", layouts=DENSE, l2=0),
    C("mss_one_chunk", "sot_mss_loss_and_grad", "mss", 3000, cite=MSS + ": one 4096-sample chunk per (scale, clip)", per_clip=0, grad=True),
    C("mss_two_chunks", "sot_mss_loss_and_grad", "mss", 5000, cite=MSS + ": a clip spanning two 4096-sample chunks", per_clip=0, grad=True),
    C("mss_two_chunks_per_clip", "sot_mss_loss_and_grad", "mss", 5000, cite=MSS + ": per_clip", per_clip=1, grad=True),
    C("mss_two_chunks_forward_only", "sot_mss_loss_and_grad", "mss", 5000, cite=MSS + ": grad_value == NULL", per_clip=0, grad=False),
    C("mss_one_chunk_per_clip_forward_only", "sot_mss_loss_and_grad", "mss", 3000, cite=MSS + ": per_clip, grad_value == NULL", per_clip=1, grad=False),
    C("metrics_two_groups", "sot_spec_metrics", "metrics", 5000, cite=MSS + ": metric mode, two groups on a union of three sizes", per_clip=0),
    C("metrics_two_groups_per_clip", "sot_spec_metrics", "metrics", 3000, cite=MSS + ": metric mode, per_clip", per_clip=1),
    # sizes: the smallest cases of tests/test_synth_geometry_gpu.py at both ends of pick_segment's range (K = 4: S = 512, K = 257: S = 8)
    C("osc_k4_s512", ("sot_oscillator_bank_forward", "sot_oscillator_bank_backward"), "osc", 3 * 512 + 5, 4, cite=OSC + ":688 / :718 four segments of 512", layouts=DENSE),
    C("osc_k257_s8", ("sot_oscillator_bank_forward", "sot_oscillator_bank_backward"), "osc", 3 * 8 + 5, 257, cite=OSC + ":688 / :718 four segments of 8", layouts=DENSE),
    C("osc_k512_one_segment", ("sot_oscillator_bank_forward", "sot_oscillator_bank_backward"), "osc", 5, 512, cite=OSC + ":680 one partial segment: the forward uses no workspace", layouts=DENSE),
    C("envelopes_k4", ("sot_synth_envelopes_forward", "sot_synth_envelopes_backward"), "envelopes", 512, 4, cite=OSC + ":620 / :638, hop 256, 2 frames", layouts=DENSE, frames=2, harmonic=False),
    C("envelopes_k257_harmonic", ("sot_synth_envelopes_forward", "sot_synth_envelopes_backward"), "envelopes", 15, 257, cite=OSC + ":620 / :638, hop 3, 5 frames", layouts=DENSE, frames=5, harmonic=True),
    C("synth_k4", ("sot_synth_forward", "sot_synth_backward", "sot_synth_tap_tables"), "synth", 1024, 4, cite=OSC + ":778 / :842, hop 512, 2 frames, two segments", layouts=DENSE, frames=2, harmonic=False),
    C("synth_k257_harmonic", ("sot_synth_forward", "sot_synth_backward", "sot_synth_tap_tables"), "synth", 15, 257, cite=OSC + ":778 / :842, hop 3, 5 frames", layouts=DENSE, frames=5, harmonic=True),
    C("fir_fwd_shared_1", "sot_fir_same_forward", "fir_fwd", 1, cite=FIR + ": samples = 1, one filter for every clip", shared=True),
    C("fir_fwd_per_clip_1024", "sot_fir_same_forward", "fir_fwd", 1024, cite=FIR + ": one full tile, taps per clip", shared=False),
    C("fir_fwd_shared_1025", "sot_fir_same_forward", "fir_fwd", 1025, cite=FIR + ": SOT_FIR_TILE + 1, one sample in the second tile", shared=True),
    C("fir_bwd_per_clip_1", "sot_fir_same_backward", "fir_bwd", 1, cite=FIR + ": samples = 1", shared=False),
    C("fir_bwd_shared_1024", "sot_fir_same_backward", "fir_bwd", 1024, cite=FIR + ": one full tile, shared filter", shared=True),
    C("fir_bwd_per_clip_1025", "sot_fir_same_backward", "fir_bwd", 1025, cite=FIR + ": SOT_FIR_TILE + 1", shared=False),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def batch_rows(case):
    """B = 2 ROWS + 1: two row groups, the last one partial; a route behind a batch threshold: the threshold + 1, or + 2"""
    if case.id == "fwd1025_two_wave":
        return kFwd1025OneWaveRows - 1
    if case.lo:
        return case.lo + 1 if (case.lo + 1) % case.rows else case.lo + 2
    return 2 * case.rows + 1


# ---- one call in one layout -------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(U8), b.contiguous().view(U8)) if a.numel() else True


class Run:
    """The buffers of one call: layout A / O / S / S4 as in the module docstring, or T -- plain contiguous torch.empty tensors, no guards.
    fill: what the inputs' padding holds ("zeros" / "poison"); outputs and workspaces are always poison."""

    def __init__(self, layout, fill="zeros"):
        self.layout, self.fill, self.dev = layout, fill, device()
        self.inputs, self.outputs, self.spaces, self.keep = {}, {}, [], []

    def _offset(self, dtype, align):
        if self.layout in ("A", "S4", "T"):
            return 0
        item = torch.empty((), dtype=dtype).element_size()
        if align is not None and align > 4:
            return align                    # exactly that alignment and no better (8 mod 16, 16 mod 32)
        return max(4, item) if item >= 4 else item

    def inp(self, name, t, strided=False, align=None):
        if name in self.inputs:
            return self.inputs[name][0]
        if self.layout == "T":
            view, g = t.contiguous().clone(), None
        else:
            stride = None
            if strided and t.ndim == 2 and self.layout in ("S", "S4"):
                stride = t.shape[1] + (3 if self.layout == "S" else 4)
            view, g = gd.guarded(t.shape, t.dtype, self.dev, row_stride=stride, offset_bytes=self._offset(t.dtype, align), fill=self.fill, name=f"input {name}")
            view.copy_(t)
            g.snapshot()
        self.inputs[name] = (view, g)
        return view

    def out(self, name, shape, dtype=F32, full=True, align=None, kind="exact", init=None):
        if self.layout == "T":
            view, g = torch.empty(shape, dtype=dtype, device=self.dev), None
        else:
            view, g = gd.guarded(shape, dtype, self.dev, offset_bytes=self._offset(dtype, align), name=f"output {name}")
        if init is not None:
            view.copy_(init)
        self.outputs[name] = (view, g, full and init is None, kind)
        return view

    def ws(self, nbytes, align=4, claim=None):
        """(pointer or None, bytes to pass): exactly nbytes usable bytes; claim: another size to tell the call (the oscillator forward)"""
        nbytes = int(nbytes)
        if nbytes == 0:
            return None, 0
        if self.layout == "T":
            view = torch.empty(nbytes, dtype=U8, device=self.dev)
            self.keep.append(view)
            return view.data_ptr(), int(claim or nbytes)
        view, g = gd.workspace(nbytes, 256 if self.layout in ("A", "S4") else align, self.dev)
        self.spaces.append((view, g))
        return view.data_ptr(), int(claim or nbytes)

    def finish(self):
        """conditions 1 - 3; the outputs as contiguous copies"""
        torch.cuda.synchronize()
        if self.layout != "T":
            for name, (view, g, full, kind) in self.outputs.items():
                g.assert_untouched()
                if full:
                    g.assert_fully_written()
            for view, g in self.spaces:
                g.assert_untouched()
            for name, (view, g) in self.inputs.items():
                g.assert_unchanged()
        return {name: view.clone() for name, (view, g, full, kind) in self.outputs.items()}

    def kinds(self):
        return {name: kind for name, (view, g, full, kind) in self.outputs.items()}


def P(t):
    return None if t is None else t.data_ptr()


def ok(nat, rc):
    assert rc == nat.SOT_OK, f"status {rc}: {nat.load().sot_status_string(rc).decode()}"


def stream(nat):
    return nat.stream_ptr(device())


def compare(case, layout, what, kinds, got, want, other=None):
    """condition 6: bit for bit, unless the line's `close` column names the layout.  other: a second documented answer (layout A without
    SOT_FLAG_TIE_FREE_GRADIENT, see test_loss_and_grad): there a gradient row has to be within the tolerance of one of the two"""
    assert set(got) == set(want)
    for name, kind in kinds.items():
        a, b = got[name], want[name]
        assert a.shape == b.shape and a.dtype == b.dtype, (case.id, what, name)
        if kind == "exact" or layout not in case.close:
            assert same_bits(a, b), (case.id, what, name, "bits differ")
        elif kind == "fwd":
            worst = float(((a.double() - b.double()).abs() / b.double().abs().clamp_min(1e-30)).max()) if a.numel() else 0.0
            print(f"{case.id} {what}: {name} worst relative difference {worst:.3e}")
            torch.testing.assert_close(a, b, **CLOSE)
        else:
            a2 = a.double().reshape(a.shape[0], -1) if a.ndim >= 2 else a.double().reshape(1, -1)
            b2 = b.double().reshape(a2.shape)
            err, scale = (a2 - b2).abs().amax(1), b2.abs().amax(1)
            if other is not None:
                c2 = other[name].double().reshape(a2.shape)
                second = (a2 - c2).abs().amax(1)
                took = (second <= GRAD_TOL * c2.abs().amax(1)) & (err > GRAD_TOL * scale)
                print(f"{case.id} {what}: {name}: {int(took.sum())} of {took.numel()} rows have the other documented answer, not A's (worst against A {float((err / scale.clamp_min(1e-300)).max()):.3e})")
                err = torch.where(took, second * scale / c2.abs().amax(1).clamp_min(1e-300), err)
            worst = float((err / scale.clamp_min(1e-300)).max())
            print(f"{case.id} {what}: {name} worst difference / row's largest entry {worst:.3e}")
            assert bool((err <= GRAD_TOL * scale).all()), (case.id, what, name, worst, int((err / scale.clamp_min(1e-300)).argmax()))


def check(case, call, wrapper=None, variants=(None,), other=None):
    """Conditions 1 - 6 for one line of CASES.  call(run, variant) makes the C call on run's buffers; wrapper(variant) -> {output: tensor};
    other(variant) -> {output: tensor}: see compare."""
    for variant in variants:
        res, kinds = {}, None
        for layout in case.layouts:
            pair = []
            for fill in ("zeros", "poison"):
                run = Run(layout, fill)
                call(run, variant)
                pair.append(run.finish())
                kinds = run.kinds()
                del run
            for name in pair[0]:
                assert same_bits(pair[0][name], pair[1][name]), (case.id, variant, layout, name, "the result depends on bytes outside the rows")
            res[layout] = pair[0]
        if wrapper is not None:
            want = wrapper(variant)
        else:
            plain = Run("T")
            call(plain, variant)
            want = plain.finish()
        for name, t in want.items():
            if t is not None:
                assert same_bits(res["A"][name], t.reshape(res["A"][name].shape)), (case.id, variant, name, "layout A differs from the wrapper's result")
        for layout in case.layouts[1:]:
            compare(case, layout, f"{variant} layout {layout} against A", kinds, res[layout], res["A"],
                    other(variant) if other is not None and layout in case.close else None)
        assert all(torch.isfinite(t.double()).all() for t in res["A"].values() if t.dtype in (F32, F64)), (case.id, variant)


# ---- SOT inputs: tests/row_kinds.py batches, made once per shape and never written to ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def sot_batch(B, n, m, rowpos, shuffled_grid=False):
    nat, dev = native(), device()
    x, y, _ = rk.make_weights(B, n, m, 7000 + n + m, dev)
    inp = dict(x=x, y=y, plan=None)
    gen = torch.Generator(device=dev).manual_seed(31 * B + n)
    if rowpos:
        inp["xpos"], _ = rk.make_positions(B, n, 100 + n, dev)
        inp["ypos"], _ = rk.make_positions(B, m, 200 + m, dev)
    else:
        inp["xpos"], inp["ypos"] = torch.linspace(0, 1, n, device=dev), torch.linspace(0, 1, m, device=dev)
        if shuffled_grid:
            inp["xpos"] = inp["xpos"][torch.randperm(n, generator=gen, device=dev)].contiguous()
            inp["ypos"] = inp["ypos"][torch.randperm(m, generator=gen, device=dev)].contiguous()
        else:
            inp["plan"] = nat.PositionPlan(inp["xpos"], inp["ypos"])
    inp["g"] = 0.5 + torch.rand(B, generator=gen, device=dev)
    if n + m <= 1200:      # the upstream gradients of the quantile tensors: the quantile cases keep n + m small
        inp["ups"] = [torch.randn(B, w, generator=gen, device=dev) for w in (n + m, n + m, n + m, n, m)]
    torch.cuda.synchronize()
    return inp


def sot_modes(nat, case):
    """(label, p, flag word): p = 1 -- on the merge kernels where the case is about them -- and the paper's cutoff mode (rk.MODES[1])"""
    extra = case.extra.get("flags", 0)
    if case.family in ("area", "tiefree"):
        return (("p1_area", 1.0, 8 | extra),)
    no_area = NO_AREA if case.family in ("fwd", "fwd_perm", "bwd", "train") else 0
    label, p, flags = rk.MODES[1]
    return (("p1", 1.0, 8 | extra | no_area), (label, p, flags | extra))


def sot_problem(run, nat, case, inp, p, flags, perm_out=None, perm_in=None):
    """the sot_problem on run's buffers, and the workspace sot_workspace_bytes reports for it (exactly)"""
    x, y = run.inp("x", inp["x"], strided=True), run.inp("y", inp["y"], strided=True)
    B, n = inp["x"].shape
    m = inp["y"].shape[1]
    pr = nat.SotProblem()
    pr.x, pr.y, pr.B, pr.n, pr.m = x.data_ptr(), y.data_ptr(), B, n, m
    pr.x_row_stride, pr.y_row_stride = x.stride(0), y.stride(0)
    pr.p = float(p)
    pr.row_perm_out, pr.row_perm_in = P(perm_out), P(perm_in)
    plan = inp["plan"]
    if plan is not None:
        pr.flags = nat.problem_flags(p, flags, plan)
        xs, ys = run.inp("xpos_sorted", plan.xpos_sorted), run.inp("ypos_sorted", plan.ypos_sorted)
        px, py, ident = run.inp("xperm", plan.xperm), run.inp("yperm", plan.yperm), run.inp("ident", plan.ident)
        pr.xpos, pr.ypos, pr.xperm, pr.yperm, pr.perm_is_identity = xs.data_ptr(), ys.data_ptr(), px.data_ptr(), py.data_ptr(), ident.data_ptr()
        pr.xpos_row_stride = pr.ypos_row_stride = 0
    else:
        pr.flags = int(flags)
        rowpos = inp["xpos"].ndim == 2
        xp, yp = run.inp("xpos", inp["xpos"], strided=rowpos), run.inp("ypos", inp["ypos"], strided=rowpos)
        pr.xpos, pr.ypos = xp.data_ptr(), yp.data_ptr()
        pr.xpos_row_stride, pr.ypos_row_stride = (xp.stride(0), yp.stride(0)) if rowpos else (0, 0)
        pr.xperm = pr.yperm = pr.perm_is_identity = None
    need = nat._needs_workspace(pr, pr.flags, plan)
    nbytes = int(nat.load().sot_workspace_bytes(ctypes.byref(pr))) if need else 0
    assert need == (nbytes > 0)
    if case.extra.get("no_workspace"):
        assert nbytes == 0, "sot_workspace_bytes reports room that nothing uses"
    ws, ws_n = run.ws(nbytes, align=4)
    return pr, ws, ws_n


def sot_inputs(case):
    B = batch_rows(case)
    if case.family == "csr":
        inp = dict(sot_batch(B, case.n, case.m, True))
        rows = torch.arange(B, dtype=I64, device=device())
        inp["xlen"], inp["ylen"] = 1 + rk.row_hash(rows, 0xA11) % case.n, 1 + rk.row_hash(rows, 0xB22) % case.m
        return inp
    return sot_batch(B, case.n, case.m, case.rowpos, bool(case.extra.get("plan_in_workspace")))


def sot_ids(*families):
    return [c.id for c in CASES if c.family in families]


@pytest.mark.parametrize("name", sot_ids("fwd", "area"))
def test_forward(name):
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B = inp["x"].shape[0]
    for label, p, flags in sot_modes(nat, case):
        def call(run, variant):
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags)
            if case.family == "area":
                assert pr.flags & SAME_GRID
            rows = run.out("row_loss", (B,), kind="fwd")
            ok(nat, nat.load().sot_w1d_forward(ctypes.byref(pr), rows.data_ptr(), ws, ws_n, stream(nat)))
        check(case, call, lambda v: dict(row_loss=nat.forward_rows(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["plan"])), (label,))


@pytest.mark.parametrize("name", sot_ids("fwd_perm"))
def test_forward_with_stored_permutations(name):
    """row_perm_out: the [B, n + m] uint16 image is an output, defined for every element; row_perm_in: the same image as an input"""
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B, n, m = inp["x"].shape[0], case.n, case.m
    for label, p, flags in sot_modes(nat, case):
        def call(run, variant):
            perm = run.out("perm", (B, n + m), U16)
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags, perm_out=perm)
            assert ws is None
            first = run.out("first", (B,), kind="fwd")
            ok(nat, nat.load().sot_w1d_forward(ctypes.byref(pr), first.data_ptr(), None, 0, stream(nat)))
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags, perm_in=perm)
            assert ws is None
            again = run.out("again", (B,), kind="fwd")
            ok(nat, nat.load().sot_w1d_forward(ctypes.byref(pr), again.data_ptr(), None, 0, stream(nat)))

        def wrapper(variant):
            perm = nat.row_permutations(inp["x"], inp["y"], inp["xpos"], inp["ypos"], flags)
            first = nat.forward_rows(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, None, perm_out=perm)
            again = nat.forward_rows(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, None, perm_in=perm)
            return dict(perm=perm, first=first, again=again)
        check(case, call, wrapper, (label,))
    xs = torch.argsort(inp["xpos"], dim=1, stable=True)
    perm = nat.row_permutations(inp["x"], inp["y"], inp["xpos"], inp["ypos"], 8)
    nat.forward_rows(inp["x"], inp["y"], inp["xpos"], inp["ypos"], 1.0, 8, None, perm_out=perm)
    assert torch.equal(perm.view(torch.int16)[:, :n].long(), xs)      # the image the layouts were compared with is the stable sort


@pytest.mark.parametrize("name", sot_ids("bwd"))
def test_backward(name):
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B, n, m = inp["x"].shape[0], case.n, case.m
    for label, p, flags in sot_modes(nat, case):
        def call(run, need_gx):
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags)
            g = run.inp("g", inp["g"])
            gx = run.out("gx", (B, n), kind="grad") if need_gx else None
            gy = run.out("gy", (B, m), kind="grad")
            ok(nat, nat.load().sot_w1d_backward(ctypes.byref(pr), g.data_ptr(), 1, 0.25, P(gx), gy.data_ptr(), ws, ws_n, stream(nat)))

        def wrapper(need_gx):
            gx, gy = nat.backward_rows(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["g"], need_gx=need_gx, plan=inp["plan"], grad_scale=0.25)
            return dict(gx=gx, gy=gy) if need_gx else dict(gy=gy)
        check(case, call, wrapper, (True, False))


@pytest.mark.parametrize("name", sot_ids("train", "tiefree"))
def test_loss_and_grad(name):
    """SOT_FLAG_TIE_FREE_GRADIENT is a permission, not a definition (include/sot_hip.h): where the merge-free training kernel serves the call, a row
    with exactly tied CDF levels gets the derivative in the CDF values, elsewhere the reference's tie order; rows without ties are the same.
    The 2048-bin kernel needs 16-byte aligned rows (csrc/sot_hip.hip: run_backward, `full` needs backward_full_supports(n, aligned16)), so
    layouts O and S run the merge walk: measured on tiefree2048, layouts O and S against A, 2 of the 3 rows (tied rows: a normalised row's two
    CDFs end at equal levels more often than not, tests/row_kinds.py) differ, by up to 1.3e-2 of the row's largest entry, and are
    the gradient of the call without the flag; the row losses differ by 1.4e-7 (the header: <= 3e-7).  The 1025-bin kernel has predicated access and
    serves every layout: tiefree1025 is held to A bit for bit like every other line.  Where tiefree2048's `close` column names the layout
    (O, S) a gradient row has to be within 1e-5 of ONE of the two documented answers, both taken in layout A: with the flag and without."""
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B, m = inp["x"].shape[0], case.m
    for label, p, flags in sot_modes(nat, case):
        flags |= TIE_FREE if case.family == "tiefree" else 0

        def call(run, variant):
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags)
            rows, mean, total = run.out("row_loss", (B,), kind="fwd"), run.out("mean", (1,), kind="fwd"), run.out("sum", (1,), F64, kind="fwd")
            gy = run.out("gy", (B, m), kind="grad")
            ok(nat, nat.load().sot_w1d_loss_and_grad(ctypes.byref(pr), rows.data_ptr(), float(B), mean.data_ptr(), total.data_ptr(), 1.0 / B, gy.data_ptr(),
                                                     None, ws, ws_n, stream(nat)))

        def wrapper(variant):
            mean, rows, gy = nat.loss_and_grad(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["plan"])
            return dict(mean=mean, row_loss=rows, gy=gy)

        def without_the_flag(variant):
            mean, rows, gy = nat.loss_and_grad(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags & ~TIE_FREE, inp["plan"])
            return dict(mean=mean.reshape(1), row_loss=rows, gy=gy)
        check(case, call, wrapper, (label,), other=without_the_flag if case.close else None)


@pytest.mark.parametrize("name", sot_ids("fused", "loss"))
def test_loss(name):
    """sot_w1d_loss: with completion_counters (one kernel; the 16 words sit in a guarded buffer and read zero after the call) and without
    (the forward kernel and sot_w1d_reduce_mean back to back)"""
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B = inp["x"].shape[0]
    hinge = case.extra.get("hinge")
    for label, p, flags in sot_modes(nat, case):
        def call(run, variant):
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags)
            rows, mean, total = run.out("row_loss", (B,), kind="fwd"), run.out("mean", (1,), kind="fwd"), run.out("sum", (1,), F64, kind="fwd")
            counters = run.out("counters", (nat.COMPLETION_COUNTER_WORDS,), I32, init=torch.zeros(16, dtype=I32, device=device())) if case.family == "fused" else None
            ok(nat, nat.load().sot_w1d_loss(ctypes.byref(pr), rows.data_ptr(), float(B), 0 if hinge is None else 1, float(hinge or 0.0), mean.data_ptr(),
                                            total.data_ptr(), P(counters), ws, ws_n, stream(nat)))
            if counters is not None:
                torch.cuda.synchronize()
                assert int(counters.abs().sum()) == 0, "the completion counters are not left zero"

        def wrapper(variant):
            mean, rows, total = nat.loss_fused(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["plan"], hinge=hinge, want_sum=True,
                                               fused_mean=case.family == "fused")
            return dict(mean=mean, row_loss=rows, sum=total)
        check(case, call, wrapper, (label,))


@pytest.mark.parametrize("name", sot_ids("posgrad"))
def test_position_grad(name):
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B, n, m = inp["x"].shape[0], case.n, case.m
    for label, p, flags in sot_modes(nat, case):
        def call(run, variant):
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags)
            g = run.inp("g", inp["g"])
            gxp, gyp = run.out("gxp", (B, n), kind="grad"), run.out("gyp", (B, m), kind="grad")
            ok(nat, nat.load().sot_w1d_position_grad(ctypes.byref(pr), g.data_ptr(), 1, 0.25, gxp.data_ptr(), gyp.data_ptr(), ws, ws_n, stream(nat)))

        def wrapper(variant):   # per-row positions: the wrapper returns the rows themselves
            gxp, gyp = nat.position_grads(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["g"], grad_scale=0.25)
            return dict(gxp=gxp, gyp=gyp)
        check(case, call, wrapper if case.rowpos else None, (label,))


@pytest.mark.parametrize("name", sot_ids("quant"))
def test_quantiles(name):
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B, n, m = inp["x"].shape[0], case.n, case.m
    names = ("uq", "vq", "Q", "U", "V")
    for label, p, flags in sot_modes(nat, case):
        def call(run, variant):
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags)
            outs = [run.out(k, (B, w), kind="fwd") for k, w in zip(names, (n + m, n + m, n + m, n, m))]
            ok(nat, nat.load().sot_w1d_quantiles(ctypes.byref(pr), *[o.data_ptr() for o in outs], ws, ws_n, stream(nat)))
        check(case, call, lambda v: dict(zip(names, nat.quantiles(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["plan"]))), (label,))


@pytest.mark.parametrize("name", sot_ids("quantgrad"))
def test_quantiles_backward(name):
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B, n, m = inp["x"].shape[0], case.n, case.m
    names = ("gx", "gy", "gxp", "gyp")
    for label, p, flags in sot_modes(nat, case):
        def call(run, variant):
            pr, ws, ws_n = sot_problem(run, nat, case, inp, p, flags)
            ups = [run.inp(f"up{k}", u) for k, u in enumerate(inp["ups"])]
            outs = [run.out(k, (B, w), kind="grad") for k, w in zip(names, (n, m, n, m))]
            ok(nat, nat.load().sot_w1d_quantiles_backward(ctypes.byref(pr), *[u.data_ptr() for u in ups], *[o.data_ptr() for o in outs], ws, ws_n, stream(nat)))

        def wrapper(variant):
            return dict(zip(names, nat.quantiles_backward(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["ups"], (True,) * 4)))
        check(case, call, wrapper if case.rowpos else None, (label,))


@pytest.mark.parametrize("name", sot_ids("csr"))
def test_forward_csr(name):
    nat, case = native(), BY_ID[name]
    inp = sot_inputs(case)
    B = inp["x"].shape[0]
    xw, xp, xoff, yw, yp, yoff = rl.csr_of(inp)
    for label, p, flags in sot_modes(nat, case):
        def call(run, variant):
            a = [run.inp(k, t) for k, t in (("xw", xw), ("xp", xp), ("xoff", xoff), ("yw", yw), ("yp", yp), ("yoff", yoff))]
            rows = run.out("row_loss", (B,), kind="fwd")
            ok(nat, nat.load().sot_w1d_forward_csr(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), xw.numel(), a[3].data_ptr(), a[4].data_ptr(), a[5].data_ptr(),
                                                   yw.numel(), B, case.n, case.m, float(p), int(flags), rows.data_ptr(), stream(nat)))
        check(case, call, lambda v: dict(row_loss=nat.forward_rows_csr(xw, xp, xoff, yw, yp, yoff, case.n, case.m, p, flags)), (label,))


@pytest.mark.parametrize("name", sot_ids("sort"))
def test_segmented_sort(name):
    nat, case = native(), BY_ID[name]
    B, n = batch_rows(case), case.n
    keys, _ = rk.make_positions(B, n, 100 + n, device())
    def call(run, variant):
        k = run.inp("keys", keys, strided=True)
        vals, idx = run.out("sorted_keys", (B, n)), run.out("indices", (B, n), I64)
        ok(nat, nat.load().sot_segmented_sort(k.data_ptr(), B, n, k.stride(0), vals.data_ptr(), idx.data_ptr(), stream(nat)))
    check(case, call, lambda v: dict(zip(("sorted_keys", "indices"), nat.segmented_sort(keys))))


# ---- mixed supports ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_batch(B, n, m, rows_on_x):
    dev = device()
    gen = torch.Generator(device=dev).manual_seed(977 * n + m)
    x, y, _ = rk.make_weights(B, n, m, 9000 + n + m, dev)
    ns, K = (m, n) if rows_on_x else (n, m)
    grid = torch.linspace(0, 1, ns, device=dev)[torch.randperm(ns, generator=gen, device=dev)].contiguous()
    rowpos = torch.rand(B, K, generator=gen, device=dev) * 1.5 - 0.2
    if K >= 2:
        rowpos[:, 1] = rowpos[:, 0]
    g = 0.5 + torch.rand(B, generator=gen, device=dev)
    return dict(x=x, y=y, xpos=rowpos if rows_on_x else grid, ypos=grid if rows_on_x else rowpos, g=g)


def mixed_call(run, nat, inp, p, flags):
    x, y = run.inp("x", inp["x"], strided=True), run.inp("y", inp["y"], strided=True)
    xp, yp = run.inp("xpos", inp["xpos"], strided=True), run.inp("ypos", inp["ypos"], strided=True)
    pr = nat.SotProblem()
    pr.x, pr.y, pr.xpos, pr.ypos = x.data_ptr(), y.data_ptr(), xp.data_ptr(), yp.data_ptr()
    pr.B, pr.n, pr.m = x.shape[0], x.shape[1], y.shape[1]
    pr.x_row_stride, pr.y_row_stride = x.stride(0), y.stride(0)
    pr.xpos_row_stride = xp.stride(0) if xp.ndim == 2 else 0
    pr.ypos_row_stride = yp.stride(0) if yp.ndim == 2 else 0
    pr.p, pr.flags = float(p), int(flags)
    nbytes = int(nat.load().sot_w1d_mixed_workspace_bytes(ctypes.byref(pr)))
    assert nbytes > 0
    return (pr,) + run.ws(nbytes, align=4)


@pytest.mark.parametrize("name", sot_ids("mixed_fwd", "mixed_bwd", "mixed_posgrad"))
def test_mixed_supports(name):
    nat, case = native(), BY_ID[name]
    inp = mixed_batch(batch_rows(case), case.n, case.m, bool(case.extra.get("rows_on_x")))
    B, n, m = inp["x"].shape[0], case.n, case.m
    K = n if case.extra.get("rows_on_x") else m
    args = (inp["x"], inp["y"], inp["xpos"], inp["ypos"])
    lib = nat.load()
    for label, p, flags in sot_modes(nat, case):
        def call(run, variant):
            pr, ws, ws_n = mixed_call(run, nat, inp, p, flags)
            if case.family == "mixed_fwd":
                rows = run.out("row_loss", (B,), kind="fwd")
                return ok(nat, lib.sot_w1d_mixed_forward(ctypes.byref(pr), rows.data_ptr(), ws, ws_n, stream(nat)))
            g = run.inp("g", inp["g"])
            if case.family == "mixed_bwd":
                gx, gy = run.out("gx", (B, n), kind="grad"), run.out("gy", (B, m), kind="grad")
                return ok(nat, lib.sot_w1d_mixed_backward(ctypes.byref(pr), g.data_ptr(), 1, 0.25, gx.data_ptr(), gy.data_ptr(), ws, ws_n, stream(nat)))
            gpos = run.out("gpos", (B, K), kind="grad")
            ok(nat, lib.sot_w1d_mixed_position_grad(ctypes.byref(pr), g.data_ptr(), 1, 0.25, gpos.data_ptr(), ws, ws_n, stream(nat)))

        def wrapper(variant):
            if case.family == "mixed_fwd":
                return dict(row_loss=nat.mixed_forward_rows(*args, p, flags))
            if case.family == "mixed_bwd":
                return dict(zip(("gx", "gy"), nat.mixed_backward_rows(*args, p, flags, inp["g"], grad_scale=0.25)))
            return dict(gpos=nat.mixed_position_grad(*args, p, flags, inp["g"], grad_scale=0.25))
        check(case, call, wrapper, (label,))


# ---- the small entry points -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sot_ids("prepare"))
def test_prepare_positions(name):
    nat, case = native(), BY_ID[name]
    n, m, dev = case.n, case.m, device()
    gen = torch.Generator(device=dev).manual_seed(n)
    xpos = (torch.rand(n, generator=gen, device=dev) * 8000.0).contiguous()
    ypos = torch.sort(torch.rand(m, generator=gen, device=dev) * 8000.0).values.contiguous()     # one side unsorted, one sorted on arrival
    fn = nat.load().sot_prepare_unit_positions if case.extra.get("unit") else nat.load().sot_prepare_positions
    def call(run, variant):
        a, b = run.inp("xpos", xpos), run.inp("ypos", ypos)
        outs = [run.out("xs", (n,)), run.out("ys", (m,)), run.out("xperm", (n,), I32), run.out("yperm", (m,), I32), run.out("ident", (2,), I32)]
        ok(nat, fn(a.data_ptr(), b.data_ptr(), n, m, *[o.data_ptr() for o in outs], stream(nat)))
    check(case, call)
    plan = nat.PositionPlan(xpos, ypos, unit=bool(case.extra.get("unit")))
    run = Run("A")
    call(run, None)
    got = run.finish()
    for k, t in zip(("xs", "ys", "xperm", "yperm", "ident"), (plan.xpos_sorted, plan.ypos_sorted, plan.xperm, plan.yperm, plan.ident)):
        assert same_bits(got[k], t), k
    assert got["ident"].tolist() == [0, 1]


@pytest.mark.parametrize("name", sot_ids("reduce"))
def test_reduce_mean(name):
    nat, case = native(), BY_ID[name]
    B, hinge = case.n, case.extra.get("hinge")
    rows = torch.rand(B, generator=torch.Generator(device=device()).manual_seed(B), device=device())
    def call(run, variant):
        r = run.inp("rows", rows)
        mean, total = run.out("mean", (1,), kind="fwd"), run.out("sum", (1,), F64, kind="fwd")
        ok(nat, nat.load().sot_w1d_reduce_mean(r.data_ptr(), B, float(B), 0 if hinge is None else 1, float(hinge or 0.0), mean.data_ptr(), total.data_ptr(), stream(nat)))

    def wrapper(variant):
        mean, total = nat.reduce_mean(rows, hinge=hinge, want_sum=True)
        return dict(mean=mean, sum=total)
    check(case, call, wrapper)


@pytest.mark.parametrize("name", sot_ids("scale"))
def test_scale_inplace(name):
    """data is input and output at once: its guard stays untouched, and the product is the float32 product torch forms"""
    nat, case = native(), BY_ID[name]
    count, dev = case.n, device()
    data = torch.randn(count, generator=torch.Generator(device=dev).manual_seed(count), device=dev)
    scalar = torch.tensor([case.extra.get("scalar", 0.37)], device=dev)
    def call(run, variant):
        s = run.inp("scalar", scalar)
        d = run.out("data", (count,), init=data)
        ok(nat, nat.load().sot_scale_inplace(d.data_ptr(), count, s.data_ptr(), stream(nat)))
    check(case, call, lambda v: dict(data=nat.scale_inplace(data.clone(), scalar.reshape(()))))
    run = Run("O")
    call(run, None)
    assert same_bits(run.finish()["data"], data * scalar)


@pytest.mark.parametrize("name", sot_ids("colsum"))
def test_column_sum(name):
    nat, case = native(), BY_ID[name]
    B, n, dev = 9, case.n, device()
    rows = torch.randn(B, n, generator=torch.Generator(device=dev).manual_seed(n), device=dev)
    def call(run, variant):
        r = run.inp("rows", rows, strided=True)
        out = run.out("out", (n,), kind="fwd")
        ok(nat, nat.load().sot_column_sum(r.data_ptr(), B, n, r.stride(0), out.data_ptr(), stream(nat)))
    check(case, call)
    run = Run("S")
    call(run, None)
    torch.testing.assert_close(run.finish()["out"], rows.double().sum(0).float(), rtol=1e-6, atol=1e-6)


# ---- STFT -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def audio_batch(batch, samples, seed):
    gen = torch.Generator(device=device()).manual_seed(seed)
    return torch.randn(batch, samples, generator=gen, device=device()), torch.randn(batch, samples, generator=gen, device=device())


@pytest.mark.parametrize("name", sot_ids("stft_fwd"))
def test_stft_forward(name):
    """mag (and spec) are defined for every element: frames past the end of the clip are transforms of zero-padded samples"""
    nat, case = native(), BY_ID[name]
    n_fft, hop, batch, samples, _ = STFT_GEO[case.extra["geo"]]
    pair, want_spec = case.extra["pair"], case.extra["spec"]
    each = 1 if pair else batch
    batch = 2 * each if pair else batch
    a_t, b_t = audio_batch(each, samples, n_fft + hop)
    window = torch.hann_window(n_fft, device=device())
    lib = nat.load()
    frames, bins = int(lib.sot_stft_frames(samples, hop)), n_fft // 2 + 1
    def call(run, variant):
        a, w = run.inp("audio_a", a_t, strided=True), run.inp("window", window, align=8)
        mag = run.out("mag", (batch, frames, bins), kind="fwd")
        spec = run.out("spec", (each, frames, bins, 2), kind="fwd", align=8) if want_spec else None
        if pair:
            b = run.inp("audio_b", b_t, strided=True)
            if want_spec:
                rc = lib.sot_stft_mag_forward_pair_spec(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), each, samples, w.data_ptr(), n_fft, hop, mag.data_ptr(), spec.data_ptr(), stream(nat))
            else:
                rc = lib.sot_stft_mag_forward_pair(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), each, samples, w.data_ptr(), n_fft, hop, mag.data_ptr(), stream(nat))
        elif want_spec:
            rc = lib.sot_stft_mag_forward_spec(a.data_ptr(), each, samples, a.stride(0), w.data_ptr(), n_fft, hop, mag.data_ptr(), spec.data_ptr(), stream(nat))
        else:
            rc = lib.sot_stft_mag_forward(a.data_ptr(), each, samples, a.stride(0), w.data_ptr(), n_fft, hop, mag.data_ptr(), stream(nat))
        ok(nat, rc)

    def wrapper(variant):
        if pair:
            res = nat.stft_mag_forward_pair(a_t, b_t, window, n_fft, hop, want_spec_b=want_spec)
            out = dict(mag=torch.cat((res[0], res[1])))
        else:
            res = nat.stft_mag_forward(a_t, window, n_fft, hop, want_spec=want_spec)
            res = res if want_spec else (res,)
            out = dict(mag=res[0])
        if want_spec:
            out["spec"] = res[-1]
        return out
    check(case, call, wrapper)


@pytest.mark.parametrize("name", sot_ids("stft_bwd"))
def test_stft_backward(name):
    nat, case = native(), BY_ID[name]
    n_fft, hop, batch, samples, from_spec, _ = STFT_BWD_GEO[case.extra["geo"]]
    accumulate = case.extra["accumulate"]
    dev, lib = device(), nat.load()
    audio, base = audio_batch(batch, samples, n_fft + hop + 1)
    window = torch.hann_window(n_fft, device=dev)
    frames, bins = int(lib.sot_stft_frames(samples, hop)), n_fft // 2 + 1
    gen = torch.Generator(device=dev).manual_seed(frames)
    grad_mag = torch.randn(batch, frames, bins, generator=gen, device=dev)
    scale = torch.tensor([0.75], device=dev)
    spec_t = nat.stft_mag_forward(audio, window, n_fft, hop, want_spec=True)[1] if from_spec else None
    nbytes = int(lib.sot_stft_backward_workspace_bytes(batch, samples, n_fft, hop))
    assert nbytes == 4 * batch * ((frames + 1) // 2) * (n_fft + hop)
    def call(run, acc):
        a, w = run.inp("audio", audio, strided=True), run.inp("window", window, align=8)
        gm, sc = run.inp("grad_mag", grad_mag), run.inp("grad_scale", scale)
        sp = run.inp("spec", spec_t, align=8) if from_spec else None
        ga = run.out("grad_audio", (batch, samples), kind="grad", init=base if acc else None)
        ws, ws_n = run.ws(nbytes, align=4)
        if from_spec:
            rc = lib.sot_stft_mag_backward_spec(a.data_ptr(), sp.data_ptr(), batch, samples, a.stride(0), w.data_ptr(), n_fft, hop, gm.data_ptr(), sc.data_ptr(), ga.data_ptr(), acc, ws, ws_n, stream(nat))
        else:
            rc = lib.sot_stft_mag_backward(a.data_ptr(), batch, samples, a.stride(0), w.data_ptr(), n_fft, hop, gm.data_ptr(), sc.data_ptr(), ga.data_ptr(), acc, ws, ws_n, stream(nat))
        ok(nat, rc)

    def wrapper(acc):
        return dict(grad_audio=nat.stft_mag_backward(audio, window, n_fft, hop, grad_mag, grad_scale=scale, accumulate_into=base.clone() if acc else None, spec=spec_t))
    check(case, call, wrapper, (accumulate,))
    if accumulate:     # the sum against the non-accumulating call: one float32 addition per sample
        plain, added = Run("A"), Run("A")
        call(plain, 0)
        call(added, 1)
        assert same_bits(added.finish()["grad_audio"], base + plain.finish()["grad_audio"])


# ---- spectral distances, the fused multi-scale loss, the metrics --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def magnitudes(rows, count, seed):
    gen = torch.Generator(device=device()).manual_seed(seed)
    t, v = torch.rand(rows, count, generator=gen, device=device()), torch.rand(rows, count, generator=gen, device=device())
    t[:, ::7] = 0.0          # below eps: no gradient through the logarithm
    v[:, 3::11] = 0.0
    return t, v


@pytest.mark.parametrize("name", sot_ids("dist_fwd", "dist_bwd", "dist_rows_fwd", "dist_rows_bwd"))
def test_spec_distance(name):
    nat, case = native(), BY_ID[name]
    dev, lib = device(), nat.load()
    by_rows = "rows" in case.family
    rows, count = (5, case.n) if by_rows else (1, case.n)
    t_t, v_t = magnitudes(rows, count, count)
    l2, acc = case.extra["l2"], case.extra.get("accumulate", 0)
    base = torch.arange(1, rows + 1, dtype=F32, device=dev) * 0.5
    up_t = torch.linspace(0.5, 1.5, rows, device=dev)
    w = (1.0, 0.5, 1e-5, l2)
    def call(run, acc):
        t, v = run.inp("target", t_t.reshape(-1)), run.inp("value", v_t.reshape(-1))
        if case.family == "dist_fwd":
            out = run.out("out", (1,), kind="fwd", init=base[:1] if acc else None)
            ws, ws_n = run.ws(lib.sot_spec_distance_workspace_bytes(), align=8)
            return ok(nat, lib.sot_spec_distance_forward(t.data_ptr(), v.data_ptr(), count, *w, out.data_ptr(), acc, ws, ws_n, stream(nat)))
        if case.family == "dist_rows_fwd":
            out = run.out("out", (rows,), kind="fwd", init=base if acc else None)
            return ok(nat, lib.sot_spec_distance_rows_forward(t.data_ptr(), v.data_ptr(), rows, count, *w, out.data_ptr(), acc, stream(nat)))
        up = run.inp("upstream", up_t)
        gt, gv = run.out("grad_target", (rows, count), kind="grad"), run.out("grad_value", (rows, count), kind="grad")
        if case.family == "dist_bwd":
            return ok(nat, lib.sot_spec_distance_backward(t.data_ptr(), v.data_ptr(), count, *w, up.data_ptr(), 0.25, gt.data_ptr(), gv.data_ptr(), stream(nat)))
        ok(nat, lib.sot_spec_distance_rows_backward(t.data_ptr(), v.data_ptr(), rows, count, *w, up.data_ptr(), 0.25, gt.data_ptr(), gv.data_ptr(), stream(nat)))

    def wrapper(acc):
        if case.family in ("dist_fwd", "dist_rows_fwd"):
            into = (base.clone() if by_rows else base[0].clone()) if acc else None
            return dict(out=nat.spec_distance_forward(t_t, v_t, 1.0, 0.5, 1e-5, bool(l2), accumulate_into=into, per_row=by_rows))
        gt, gv = nat.spec_distance_backward(t_t, v_t, 1.0, 0.5, up_t, 0.25, 1e-5, bool(l2), need_target=True, need_value=True, per_row=by_rows)
        return dict(grad_target=gt, grad_value=gv)
    check(case, call, wrapper, (acc,))
    if acc:     # the sum against the non-accumulating call: one float32 addition
        plain, added = Run("A"), Run("A")
        call(plain, 0)
        call(added, 1)
        plain_res, added_res = plain.finish()["out"], added.finish()["out"]
        assert same_bits(added_res, base[:added_res.numel()] + plain_res)


MSS_SIZES = (64, 512, 2048)


def mss_setup(run, nat, samples, sizes):
    t_t, v_t = audio_batch(2, samples, samples)
    t, v = run.inp("target", t_t, strided=True), run.inp("value", v_t, strided=True)
    wins = [run.inp(f"window{s}", torch.hann_window(s, device=device()), align=8) for s in sizes]
    csizes = (ctypes.c_int * len(sizes))(*sizes)
    wptr = (ctypes.c_void_p * len(sizes))(*[w.data_ptr() for w in wins])
    run.keep += [csizes, wptr]
    return t, v, wins, csizes, wptr


@pytest.mark.parametrize("name", sot_ids("mss"))
def test_mss_loss_and_grad(name):
    nat, case = native(), BY_ID[name]
    lib, samples, per_clip, want_grad = nat.load(), case.n, case.extra["per_clip"], case.extra["grad"]
    t_t, v_t = audio_batch(2, samples, samples)
    def call(run, variant):
        t, v, wins, csizes, wptr = mss_setup(run, nat, samples, MSS_SIZES)
        nbytes = lib.sot_mss_workspace_bytes(2, samples, ctypes.cast(csizes, ctypes.c_void_p), 3)
        assert nbytes > 0
        loss = run.out("loss", (2,) if per_clip else (1,), kind="fwd")
        grad = run.out("grad", (2, samples), kind="grad") if want_grad else None
        ws, ws_n = run.ws(nbytes, align=16)
        ok(nat, lib.sot_mss_loss_and_grad(t.data_ptr(), t.stride(0), v.data_ptr(), v.stride(0), 2, samples, ctypes.cast(csizes, ctypes.c_void_p),
                                          ctypes.cast(wptr, ctypes.c_void_p), 3, 1.0, 1.0, 1e-5, 0, per_clip, 0.5, loss.data_ptr(), P(grad), ws, ws_n, stream(nat)))

    def wrapper(variant):
        wins = [torch.hann_window(s, device=device()) for s in MSS_SIZES]
        loss, grad = nat.mss_loss_and_grad(t_t, v_t, MSS_SIZES, wins, 1.0, 1.0, 1e-5, False, bool(per_clip), want_grad, 0.5)
        return dict(loss=loss, grad=grad) if want_grad else dict(loss=loss)
    check(case, call, wrapper)


@pytest.mark.parametrize("name", sot_ids("metrics"))
def test_spec_metrics(name):
    nat, case = native(), BY_ID[name]
    lib, samples, per_clip = nat.load(), case.n, case.extra["per_clip"]
    t_t, v_t = audio_batch(2, samples, samples)
    groups = [((64, 512), 1.0, 1.0, 0.0, False), ((2048, 512), 0.0, 0.0, 1.0, True)]
    def call(run, variant):
        t, v, wins, csizes, wptr = mss_setup(run, nat, samples, MSS_SIZES)
        grp = (nat.SotMetricGroup * 2)()
        for i, (gs, mag_w, log_w, lsd_w, l2) in enumerate(groups):
            grp[i].n_sizes = len(gs)
            for j, s in enumerate(gs):
                grp[i].fft_sizes[j] = s
            grp[i].mag_weight, grp[i].logmag_weight, grp[i].lsd_weight, grp[i].l2 = mag_w, log_w, lsd_w, int(l2)
        run.keep.append(grp)
        nbytes = lib.sot_spec_metrics_workspace_bytes(2, samples, ctypes.cast(csizes, ctypes.c_void_p), 3, 2)
        assert nbytes > 0
        out = run.out("out", (2, 2) if per_clip else (2,), kind="fwd")
        ws, ws_n = run.ws(nbytes, align=8)
        ok(nat, lib.sot_spec_metrics(t.data_ptr(), t.stride(0), v.data_ptr(), v.stride(0), 2, samples, ctypes.cast(csizes, ctypes.c_void_p),
                                     ctypes.cast(wptr, ctypes.c_void_p), 3, ctypes.cast(grp, ctypes.c_void_p), 2, 1e-5, per_clip, out.data_ptr(), ws, ws_n, stream(nat)))

    def wrapper(variant):
        wins = [torch.hann_window(s, device=device()) for s in MSS_SIZES]
        return dict(out=nat.spec_metrics(t_t, v_t, MSS_SIZES, wins, groups, 1e-5, bool(per_clip)))
    check(case, call, wrapper)


# ---- the synthesiser ----------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


@pytest.mark.parametrize("name", sot_ids("osc"))
def test_oscillator_bank(name):
    """The forward is told the whole workspace and given a buffer of its first half only: the header says it uses no more.  The backward
    runs on its own workspace (segment phases rebuilt) and on the forward's (workspace_from_forward)."""
    import synth_model as sm
    nat, case = native(), BY_ID[name]
    lib, samples, k, batch = nat.load(), case.n, case.m, 2
    freq_t, amp_t, grad_t = (_dev(a) for a in sm.bank_inputs(1000 * k + samples, batch, samples, k))
    nbytes = int(lib.sot_oscillator_bank_workspace_bytes(batch, samples, k))
    assert nbytes > 0 and nbytes % 16 == 0
    def call(run, from_forward):
        f, a, g = run.inp("freq", freq_t), run.inp("amp", amp_t), run.inp("grad_audio", grad_t)
        audio = run.out("audio", (batch, samples), kind="fwd")
        gf, ga = run.out("grad_freq", (batch, samples, k), kind="grad"), run.out("grad_amp", (batch, samples, k), kind="grad")
        if from_forward:
            ws, ws_n = run.ws(nbytes, align=8)
            ok(nat, lib.sot_oscillator_bank_forward(f.data_ptr(), a.data_ptr(), batch, samples, k, sm.SR, audio.data_ptr(), ws, ws_n, stream(nat)))
        else:
            half, claimed = run.ws(nbytes // 2, align=8, claim=nbytes)
            ok(nat, lib.sot_oscillator_bank_forward(f.data_ptr(), a.data_ptr(), batch, samples, k, sm.SR, audio.data_ptr(), half, claimed, stream(nat)))
            ws, ws_n = run.ws(nbytes, align=8)
        ok(nat, lib.sot_oscillator_bank_backward(f.data_ptr(), a.data_ptr(), batch, samples, k, sm.SR, g.data_ptr(), gf.data_ptr(), ga.data_ptr(), ws, ws_n,
                                                 int(from_forward), stream(nat)))

    def wrapper(from_forward):
        audio, ws = nat.oscillator_bank_forward(freq_t, amp_t, sm.SR, return_workspace=True)
        gf, ga = nat.oscillator_bank_backward(freq_t, amp_t, sm.SR, grad_t, forward_workspace=ws if from_forward else None)
        return dict(audio=audio, grad_freq=gf, grad_amp=ga)
    check(case, call, wrapper, (0, 1))


@pytest.mark.parametrize("name", sot_ids("envelopes"))
def test_synth_envelopes(name):
    import synth_model as sm
    nat, case = native(), BY_ID[name]
    lib, samples, k, frames, harmonic, batch = nat.load(), case.n, case.m, case.extra["frames"], case.extra["harmonic"], 2
    amp_t, freq_t = (_dev(a) for a in sm.control_inputs(1000 * k + samples, batch, frames, k, harmonic))
    window = torch.hann_window(2 * samples // frames, device=device())
    gen = torch.Generator(device=device()).manual_seed(k)
    gae_t, gfe_t = torch.randn(batch, samples, k, generator=gen, device=device()), torch.randn(batch, samples, k, generator=gen, device=device())
    def call(run, variant):
        a, f, w = run.inp("amp_frames", amp_t), run.inp("freq_frames", freq_t), run.inp("window", window)
        gae, gfe = run.inp("grad_amp_env", gae_t), run.inp("grad_freq_env", gfe_t)
        amp_env, freq_env = run.out("amp_env", (batch, samples, k), kind="fwd"), run.out("freq_env", (batch, samples, k), kind="fwd")
        ga, gf = run.out("grad_amp_frames", amp_t.shape, kind="grad"), run.out("grad_freq_frames", freq_t.shape, kind="grad")
        ok(nat, lib.sot_synth_envelopes_forward(a.data_ptr(), f.data_ptr(), w.data_ptr(), batch, frames, k, int(harmonic), samples, sm.SR, amp_env.data_ptr(),
                                                freq_env.data_ptr(), stream(nat)))
        ok(nat, lib.sot_synth_envelopes_backward(a.data_ptr(), f.data_ptr(), w.data_ptr(), batch, frames, k, int(harmonic), samples, sm.SR, gae.data_ptr(), gfe.data_ptr(),
                                                 ga.data_ptr(), gf.data_ptr(), stream(nat)))

    def wrapper(variant):
        amp_env, freq_env = nat.synth_envelopes_forward(amp_t, freq_t, window, samples, sm.SR, harmonic)
        ga, gf = nat.synth_envelopes_backward(amp_t, freq_t, window, samples, sm.SR, harmonic, gae_t, gfe_t)
        return dict(amp_env=amp_env, freq_env=freq_env, grad_amp_frames=ga, grad_freq_frames=gf)
    check(case, call, wrapper)


@pytest.mark.parametrize("name", sot_ids("synth"))
def test_synth(name):
    """sot_synth_forward on the forward-sized workspace; sot_synth_backward on its own workspace with the tables built inside (variant 0), and
    on the caller's tap tables (sot_synth_tap_tables: a buffer of exactly sot_synth_tap_table_bytes, every byte defined) with the segment
    phases of a forward run on the backward-sized workspace (variant 1)"""
    import synth_model as sm
    nat, case = native(), BY_ID[name]
    lib, samples, k, frames, harmonic, batch = nat.load(), case.n, case.m, case.extra["frames"], case.extra["harmonic"], 2
    amp_t, freq_t = (_dev(a) for a in sm.control_inputs(1000 * k + samples, batch, frames, k, harmonic))
    window = torch.hann_window(2 * samples // frames, device=device())
    grad_t = torch.randn(batch, samples, generator=torch.Generator(device=device()).manual_seed(k), device=device())
    fwd_bytes, bwd_bytes = int(lib.sot_synth_workspace_bytes(batch, frames, samples, k, 0)), int(lib.sot_synth_workspace_bytes(batch, frames, samples, k, 1))
    table_bytes = int(lib.sot_synth_tap_table_bytes(frames, samples))
    assert 0 < fwd_bytes < bwd_bytes and table_bytes == 12 * 3 * samples
    def call(run, reuse):
        a, f, w, g = run.inp("amp_frames", amp_t), run.inp("freq_frames", freq_t), run.inp("window", window), run.inp("grad_audio", grad_t)
        audio = run.out("audio", (batch, samples), kind="fwd")
        ga, gf = run.out("grad_amp_frames", amp_t.shape, kind="grad"), run.out("grad_freq_frames", freq_t.shape, kind="grad")
        head = (a.data_ptr(), f.data_ptr(), w.data_ptr(), batch, frames, k, int(harmonic), samples, sm.SR)
        tables = None
        if reuse:
            tables = run.out("tap_tables", (table_bytes,), U8, align=8)
            ok(nat, lib.sot_synth_tap_tables(w.data_ptr(), frames, samples, tables.data_ptr(), stream(nat)))
            ws, ws_n = run.ws(bwd_bytes, align=8)
            ok(nat, lib.sot_synth_forward(*head, audio.data_ptr(), ws, ws_n, stream(nat)))
        else:
            fws, fws_n = run.ws(fwd_bytes, align=8)
            ok(nat, lib.sot_synth_forward(*head, audio.data_ptr(), fws, fws_n, stream(nat)))
            ws, ws_n = run.ws(bwd_bytes, align=8)
        ok(nat, lib.sot_synth_backward(*head, g.data_ptr(), ga.data_ptr(), gf.data_ptr(), P(tables), ws, ws_n, int(reuse), stream(nat)))

    def wrapper(reuse):
        audio, ws = nat.synth_forward(amp_t, freq_t, window, samples, sm.SR, harmonic, for_backward=bool(reuse))
        tables = nat.synth_tap_tables(window, frames, samples) if reuse else None
        ga, gf = nat.synth_backward(amp_t, freq_t, window, samples, sm.SR, harmonic, grad_t, forward_workspace=ws if reuse else None, tap_tables=tables)
        out = dict(audio=audio, grad_amp_frames=ga, grad_freq_frames=gf)
        if reuse:
            out["tap_tables"] = tables[:table_bytes]
        return out
    check(case, call, wrapper, (0, 1))


# ---- FIR ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sot_ids("fir_fwd", "fir_bwd"))
def test_fir(name):
    nat, case = native(), BY_ID[name]
    lib, dev, samples, shared, batch, n_taps, start = nat.load(), device(), case.n, case.extra["shared"], 3, 128, 62
    gen = torch.Generator(device=dev).manual_seed(samples)
    audio_t, grad_t = torch.randn(batch, samples, generator=gen, device=dev), torch.randn(batch, samples, generator=gen, device=dev)
    taps_t = torch.randn(n_taps, generator=gen, device=dev) if shared else torch.randn(batch, n_taps, generator=gen, device=dev)
    nbytes = int(lib.sot_fir_workspace_bytes(batch, samples, n_taps))
    def call(run, variant):
        a, t = run.inp("audio", audio_t, strided=True), run.inp("taps", taps_t, strided=True)
        t_stride = 0 if shared else t.stride(0)
        if case.family == "fir_fwd":
            out = run.out("out", (batch, samples), kind="grad")
            return ok(nat, lib.sot_fir_same_forward(a.data_ptr(), a.stride(0), t.data_ptr(), t_stride, batch, samples, n_taps, start, out.data_ptr(), stream(nat)))
        g = run.inp("grad_out", grad_t)
        ga, gt = run.out("grad_audio", (batch, samples), kind="grad"), run.out("grad_taps", (batch, n_taps), kind="grad")
        ws, ws_n = run.ws(nbytes, align=8)
        ok(nat, lib.sot_fir_same_backward(g.data_ptr(), a.data_ptr(), a.stride(0), t.data_ptr(), t_stride, batch, samples, n_taps, start, ga.data_ptr(), gt.data_ptr(),
                                          ws, ws_n, stream(nat)))

    def wrapper(variant):
        if case.family == "fir_fwd":
            return dict(out=nat.fir_same_forward(audio_t, taps_t, start))
        ga, gt = nat.fir_same_backward(grad_t, audio_t, taps_t, start, need_audio=True, need_taps=True)
        return dict(grad_audio=ga, grad_taps=None if shared else gt)     # a shared filter: the wrapper sums the rows
    check(case, call, wrapper)


# ---- condition 7: refusals and empty batches ---------------------------------------------------------------------------------------------
Refusal = collections.namedtuple("Refusal", "id entries status what")
REFUSALS = []
OK_, INVALID_P, BAD_SHAPE, UNSUPPORTED, NULLP, WORKSPACE = 0, -1, -2, -3, -4, -5


class Blank:
    """Buffers a refused call is handed: every one an EMPTY view in the middle of a poisoned allocation -- whatever the call writes is caught"""

    def __init__(self):
        self.guards = []

    def ptr(self, dtype=F32, align=256):
        view, g = gd.guarded((0,), dtype, device(), offset_bytes=align % 256, name=f"buffer {len(self.guards)} of a refused call")
        self.guards.append(g)
        return gd.ptr(view, g)

    def assert_untouched(self):
        torch.cuda.synchronize()
        for g in self.guards:
            g.assert_untouched()


def small_problem(nat, B=3, n=16, m=16, p=2.0, flags=8, rowpos=True):
    dev = device()
    t = dict(x=torch.rand(max(B, 1), n, device=dev), y=torch.rand(max(B, 1), m, device=dev),
             xpos=torch.rand(max(B, 1), n, device=dev) if rowpos else torch.linspace(0, 1, n, device=dev),
             ypos=torch.rand(max(B, 1), m, device=dev) if rowpos else torch.linspace(0, 1, m, device=dev), g=torch.ones(max(B, 1), device=dev))
    pr = nat.SotProblem()
    pr.x, pr.y, pr.xpos, pr.ypos = (t[k].data_ptr() for k in ("x", "y", "xpos", "ypos"))
    pr.B, pr.n, pr.m, pr.x_row_stride, pr.y_row_stride = B, n, m, n, m
    pr.xpos_row_stride, pr.ypos_row_stride = (n, m) if rowpos else (0, 0)
    pr.p, pr.flags = p, flags
    return pr, t


def _sot_refusals():
    """(id, entry, status, problem changes, call) for the calls that take a sot_problem"""
    def fwd(lib, pr, t, b):
        return lib.sot_w1d_forward(ctypes.byref(pr), b.ptr(), b.ptr(U8), 1 << 16, None)

    def bwd(lib, pr, t, b):
        return lib.sot_w1d_backward(ctypes.byref(pr), t["g"].data_ptr(), 1, 1.0, b.ptr(), b.ptr(), b.ptr(U8), 1 << 16, None)

    def train(lib, pr, t, b):
        return lib.sot_w1d_loss_and_grad(ctypes.byref(pr), b.ptr(), 3.0, b.ptr(), b.ptr(F64), 1.0, b.ptr(), None, b.ptr(U8), 1 << 16, None)

    def loss(lib, pr, t, b):
        return lib.sot_w1d_loss(ctypes.byref(pr), b.ptr(), 3.0, 0, 0.0, b.ptr(), b.ptr(F64), b.ptr(I32), b.ptr(U8), 1 << 16, None)

    def quant(lib, pr, t, b):
        return lib.sot_w1d_quantiles(ctypes.byref(pr), b.ptr(), b.ptr(), b.ptr(), b.ptr(), b.ptr(), b.ptr(U8), 1 << 16, None)

    def quantgrad(lib, pr, t, b):
        return lib.sot_w1d_quantiles_backward(ctypes.byref(pr), None, None, None, t["x"].data_ptr(), None, b.ptr(), b.ptr(), b.ptr(), b.ptr(), b.ptr(U8), 1 << 16, None)

    def posgrad(lib, pr, t, b):
        return lib.sot_w1d_position_grad(ctypes.byref(pr), t["g"].data_ptr(), 1, 1.0, b.ptr(), b.ptr(), b.ptr(U8), 1 << 16, None)
    calls = dict(sot_w1d_forward=fwd, sot_w1d_backward=bwd, sot_w1d_loss_and_grad=train, sot_w1d_loss=loss, sot_w1d_quantiles=quant,
                 sot_w1d_quantiles_backward=quantgrad, sot_w1d_position_grad=posgrad)
    changes = [("p_below_1", INVALID_P, dict(p=0.5)), ("bad_stride", BAD_SHAPE, dict(x_row_stride=15)), ("positions_half_shared", BAD_SHAPE, dict(ypos_row_stride=0)),
               ("unsupported_size", UNSUPPORTED, dict(n=40000, m=40000, x_row_stride=40000, y_row_stride=40000, xpos_row_stride=40000, ypos_row_stride=40000))]
    out = []
    for entry, fn in calls.items():
        for what, status, change in changes:
            out.append((f"{entry}-{what}", entry, status, change, fn))
        empty = BAD_SHAPE if entry in ("sot_w1d_loss", "sot_w1d_loss_and_grad") else OK_      # the mean of zero rows is undefined
        out.append((f"{entry}-empty_batch", entry, empty, dict(B=0), fn))
    return out


SOT_REFUSALS = _sot_refusals()
for _id, _entry, _status, _change, _fn in SOT_REFUSALS:
    REFUSALS.append(Refusal(_id, (_entry,), _status, str(_change)))


@pytest.mark.parametrize("rid", [r[0] for r in SOT_REFUSALS])
def test_refused_sot_calls_write_nothing(rid):
    nat = native()
    _, entry, status, change, fn = next(r for r in SOT_REFUSALS if r[0] == rid)
    pr, t = small_problem(nat)
    for k, v in change.items():
        setattr(pr, k, v)
    b = Blank()
    assert fn(nat.load(), pr, t, b) == status
    b.assert_untouched()


def test_workspace_one_byte_short_is_refused():
    """shared positions that the call has to plan: SOT_ERR_WORKSPACE with one byte less than sot_workspace_bytes, SOT_OK with exactly that"""
    nat = native()
    lib = nat.load()
    pr, t = small_problem(nat, rowpos=False)
    need = int(lib.sot_workspace_bytes(ctypes.byref(pr)))
    b = Blank()
    ws, g = gd.workspace(need, 256, device())
    for fn in (lambda n: lib.sot_w1d_forward(ctypes.byref(pr), b.ptr(), ws.data_ptr(), n, None),
               lambda n: lib.sot_w1d_backward(ctypes.byref(pr), None, 0, 1.0, b.ptr(), b.ptr(), ws.data_ptr(), n, None),
               lambda n: lib.sot_w1d_loss(ctypes.byref(pr), b.ptr(), 3.0, 0, 0.0, b.ptr(), None, None, ws.data_ptr(), n, None),
               lambda n: lib.sot_w1d_quantiles(ctypes.byref(pr), b.ptr(), None, None, None, None, ws.data_ptr(), n, None)):
        assert fn(need - 1) == WORKSPACE
    b.assert_untouched()
    assert int((ws.view(I32) != gd.POISON).sum()) == 0, "a refused call wrote into its workspace"
    g.assert_untouched()
REFUSALS.append(Refusal("workspace_one_byte_short", ("sot_w1d_forward", "sot_w1d_backward", "sot_w1d_loss", "sot_w1d_quantiles"), WORKSPACE, "sot_workspace_bytes() - 1"))


OTHER_REFUSALS = {}


def other(id, entries, status):
    def deco(fn):
        OTHER_REFUSALS[id] = (fn, status)
        REFUSALS.append(Refusal(id, (entries,) if isinstance(entries, str) else tuple(entries), status, fn.__doc__ or ""))
        return fn
    return deco


def _mixed_pr(nat, **change):
    pr, t = small_problem(nat, n=33, m=16)
    t["grid"] = torch.linspace(0, 1, 33, device=device())
    pr.xpos, pr.xpos_row_stride = t["grid"].data_ptr(), 0
    for k, v in change.items():
        setattr(pr, k, v)
    return pr, t


for _entry in ("sot_w1d_mixed_forward", "sot_w1d_mixed_backward", "sot_w1d_mixed_position_grad"):
    def _mixed(lib, b, pr, t, entry=_entry):
        if entry == "sot_w1d_mixed_forward":
            return lib.sot_w1d_mixed_forward(ctypes.byref(pr), b.ptr(), b.ptr(U8), 1 << 16, None)
        if entry == "sot_w1d_mixed_backward":
            return lib.sot_w1d_mixed_backward(ctypes.byref(pr), t["g"].data_ptr(), 1, 1.0, b.ptr(), b.ptr(), b.ptr(U8), 1 << 16, None)
        return lib.sot_w1d_mixed_position_grad(ctypes.byref(pr), t["g"].data_ptr(), 1, 1.0, b.ptr(), b.ptr(U8), 1 << 16, None)
    other(f"{_entry}-both_shared", _entry, BAD_SHAPE)(lambda nat, b, f=_mixed: f(nat.load(), b, *_mixed_pr(nat, ypos_row_stride=0)))
    other(f"{_entry}-p_below_1", _entry, INVALID_P)(lambda nat, b, f=_mixed: f(nat.load(), b, *_mixed_pr(nat, p=0.0)))
    other(f"{_entry}-row_side_2049", _entry, UNSUPPORTED)(lambda nat, b, f=_mixed: f(nat.load(), b, *_mixed_pr(nat, m=2049, y_row_stride=2049, ypos_row_stride=2049)))
    other(f"{_entry}-empty_batch", _entry, OK_)(lambda nat, b, f=_mixed: f(nat.load(), b, *_mixed_pr(nat, B=0)))


def _some(n, dtype=F32):
    return torch.ones(n, dtype=dtype, device=device()) if dtype != F32 else torch.rand(n, device=device())


@other("csr-p_below_1", "sot_w1d_forward_csr", INVALID_P)
def _(nat, b):
    w, off = _some(12), torch.tensor([0, 4, 8, 12], device=device())
    return nat.load().sot_w1d_forward_csr(w.data_ptr(), w.data_ptr(), off.data_ptr(), 12, w.data_ptr(), w.data_ptr(), off.data_ptr(), 12, 3, 4, 4, 0.5, 8, b.ptr(), None)


@other("csr-empty_batch", "sot_w1d_forward_csr", OK_)
def _(nat, b):
    w, off = _some(12), torch.tensor([0], device=device())
    return nat.load().sot_w1d_forward_csr(w.data_ptr(), w.data_ptr(), off.data_ptr(), 12, w.data_ptr(), w.data_ptr(), off.data_ptr(), 12, 0, 4, 4, 1.0, 8, b.ptr(), None)


@other("sort-bad_stride", "sot_segmented_sort", BAD_SHAPE)
def _(nat, b):
    return nat.load().sot_segmented_sort(_some(64).data_ptr(), 4, 16, 15, b.ptr(), b.ptr(I64), None)


@other("sort-unsupported_size", "sot_segmented_sort", UNSUPPORTED)
def _(nat, b):
    return nat.load().sot_segmented_sort(_some(20000).data_ptr(), 1, 20000, 20000, b.ptr(), b.ptr(I64), None)


@other("sort-empty_batch", "sot_segmented_sort", OK_)
def _(nat, b):
    return nat.load().sot_segmented_sort(_some(64).data_ptr(), 0, 16, 16, b.ptr(), b.ptr(I64), None)


for _entry in ("sot_prepare_positions", "sot_prepare_unit_positions"):
    other(f"{_entry}-n_0", _entry, BAD_SHAPE)(lambda nat, b, e=_entry: getattr(nat.load(), e)(_some(16).data_ptr(), _some(16).data_ptr(), 0, 16, b.ptr(), b.ptr(), b.ptr(I32), b.ptr(I32), b.ptr(I32), None))
    other(f"{_entry}-unsupported_size", _entry, UNSUPPORTED)(lambda nat, b, e=_entry: getattr(nat.load(), e)(_some(20000).data_ptr(), _some(16).data_ptr(), 20000, 16, b.ptr(), b.ptr(), b.ptr(I32), b.ptr(I32), b.ptr(I32), None))


@other("reduce_mean-negative_batch", "sot_w1d_reduce_mean", BAD_SHAPE)
def _(nat, b):
    """(B == 0 is a defined call: test_empty_batch_of_the_two_calls_that_are_defined_for_it)"""
    return nat.load().sot_w1d_reduce_mean(_some(4).data_ptr(), -1, 4.0, 0, 0.0, b.ptr(), b.ptr(F64), None)


@other("scale-negative_count", "sot_scale_inplace", BAD_SHAPE)
def _(nat, b):
    return nat.load().sot_scale_inplace(b.ptr(), -1, _some(1).data_ptr(), None)


@other("scale-empty", "sot_scale_inplace", OK_)
def _(nat, b):
    return nat.load().sot_scale_inplace(b.ptr(), 0, _some(1).data_ptr(), None)


def test_empty_batch_of_the_two_calls_that_are_defined_for_it():
    """include/sot_hip.h: sot_w1d_reduce_mean and sot_column_sum with B == 0 are defined calls -- the sum of no rows.  Guarded outputs: the mean is
    0 / denom = 0, the fp64 sum 0, the column sums n zeros; nothing outside them is written, and the row pointer (NULL here) is not followed."""
    nat = native()
    lib = nat.load()
    for layout in ("A", "O"):
        run = Run(layout)
        mean, total = run.out("mean", (1,)), run.out("sum", (1,), F64)
        ok(nat, lib.sot_w1d_reduce_mean(None, 0, 4.0, 1, 0.5, mean.data_ptr(), total.data_ptr(), stream(nat)))
        got = run.finish()
        assert same_bits(got["mean"], torch.zeros(1, device=device())) and same_bits(got["sum"], torch.zeros(1, dtype=F64, device=device()))
        for n in (1, 16, 300):
            run = Run(layout)
            out = run.out("out", (n,))
            ok(nat, lib.sot_column_sum(None, 0, n, n + 3, out.data_ptr(), stream(nat)))
            assert same_bits(run.finish()["out"], torch.zeros(n, device=device())), n
REFUSALS.append(Refusal("reduce_mean-empty_batch", ("sot_w1d_reduce_mean",), OK_, "B == 0: a defined call, mean 0 and sum 0 in guarded outputs"))
REFUSALS.append(Refusal("column_sum-empty_batch", ("sot_column_sum",), OK_, "B == 0: a defined call, n zeros in a guarded output"))


@other("column_sum-bad_stride", "sot_column_sum", BAD_SHAPE)
def _(nat, b):
    """(B == 0 is a defined call: test_empty_batch_of_the_two_calls_that_are_defined_for_it)"""
    return nat.load().sot_column_sum(_some(64).data_ptr(), 4, 16, 15, b.ptr(), None)


def _stft_forward(nat, b, entry, batch=2, n_fft=64, stride=100, window_offset=0):
    lib, a, w = nat.load(), _some(200), torch.hann_window(n_fft + 2, device=device())
    wp = w.data_ptr() + window_offset
    if entry == "sot_stft_mag_forward":
        return lib.sot_stft_mag_forward(a.data_ptr(), batch, 100, stride, wp, n_fft, 16, b.ptr(), None)
    if entry == "sot_stft_mag_forward_spec":
        return lib.sot_stft_mag_forward_spec(a.data_ptr(), batch, 100, stride, wp, n_fft, 16, b.ptr(), b.ptr(), None)
    if entry == "sot_stft_mag_forward_pair":
        return lib.sot_stft_mag_forward_pair(a.data_ptr(), stride, a.data_ptr(), stride, batch // 2, 100, wp, n_fft, 16, b.ptr(), None)
    return lib.sot_stft_mag_forward_pair_spec(a.data_ptr(), stride, a.data_ptr(), stride, batch // 2, 100, wp, n_fft, 16, b.ptr(), b.ptr(), None)


for _entry in ("sot_stft_mag_forward", "sot_stft_mag_forward_spec", "sot_stft_mag_forward_pair", "sot_stft_mag_forward_pair_spec"):
    other(f"{_entry}-n_fft_96", _entry, UNSUPPORTED)(lambda nat, b, e=_entry: _stft_forward(nat, b, e, n_fft=96))
    other(f"{_entry}-bad_stride", _entry, BAD_SHAPE)(lambda nat, b, e=_entry: _stft_forward(nat, b, e, stride=99))
    other(f"{_entry}-window_4_mod_8", _entry, BAD_SHAPE)(lambda nat, b, e=_entry: _stft_forward(nat, b, e, window_offset=4))
    other(f"{_entry}-empty_batch", _entry, OK_)(lambda nat, b, e=_entry: _stft_forward(nat, b, e, batch=0))


def _stft_backward(nat, b, entry, batch=2, short=0, n_fft=64):
    lib, a, w, gm = nat.load(), _some(200), torch.hann_window(64, device=device()), _some(2 * 7 * 33)
    need = int(lib.sot_stft_backward_workspace_bytes(2, 100, 64, 16))
    if entry == "sot_stft_mag_backward":
        return lib.sot_stft_mag_backward(a.data_ptr(), batch, 100, 100, w.data_ptr(), n_fft, 16, gm.data_ptr(), None, b.ptr(), 0, b.ptr(U8), need - short, None)
    spec = _some(2 * 7 * 33 * 2)
    return lib.sot_stft_mag_backward_spec(a.data_ptr(), spec.data_ptr(), batch, 100, 100, w.data_ptr(), n_fft, 16, gm.data_ptr(), None, b.ptr(), 0, b.ptr(U8), need - short, None)


for _entry in ("sot_stft_mag_backward", "sot_stft_mag_backward_spec"):
    other(f"{_entry}-workspace_one_byte_short", _entry, WORKSPACE)(lambda nat, b, e=_entry: _stft_backward(nat, b, e, short=1))
    other(f"{_entry}-n_fft_8192", _entry, UNSUPPORTED)(lambda nat, b, e=_entry: _stft_backward(nat, b, e, n_fft=8192))
    other(f"{_entry}-empty_batch", _entry, OK_)(lambda nat, b, e=_entry: _stft_backward(nat, b, e, batch=0))


@other("dist_fwd-workspace_one_byte_short", "sot_spec_distance_forward", WORKSPACE)
def _(nat, b):
    return nat.load().sot_spec_distance_forward(_some(64).data_ptr(), _some(64).data_ptr(), 64, 1.0, 1.0, 1e-5, 0, b.ptr(), 0, b.ptr(U8, 8), 8 * 1024 - 1, None)


@other("dist_fwd-empty", "sot_spec_distance_forward", BAD_SHAPE)
def _(nat, b):
    return nat.load().sot_spec_distance_forward(_some(64).data_ptr(), _some(64).data_ptr(), 0, 1.0, 1.0, 1e-5, 0, b.ptr(), 0, b.ptr(U8, 8), 8 * 1024, None)


@other("dist_bwd-empty", "sot_spec_distance_backward", BAD_SHAPE)
def _(nat, b):
    return nat.load().sot_spec_distance_backward(_some(64).data_ptr(), _some(64).data_ptr(), 0, 1.0, 1.0, 1e-5, 0, _some(1).data_ptr(), 1.0, b.ptr(), b.ptr(), None)


@other("dist_rows_fwd-no_rows", "sot_spec_distance_rows_forward", BAD_SHAPE)
def _(nat, b):
    return nat.load().sot_spec_distance_rows_forward(_some(64).data_ptr(), _some(64).data_ptr(), 0, 16, 1.0, 1.0, 1e-5, 0, b.ptr(), 0, None)


@other("dist_rows_bwd-no_rows", "sot_spec_distance_rows_backward", BAD_SHAPE)
def _(nat, b):
    return nat.load().sot_spec_distance_rows_backward(_some(64).data_ptr(), _some(64).data_ptr(), 0, 16, 1.0, 1.0, 1e-5, 0, _some(4).data_ptr(), 1.0, b.ptr(), b.ptr(), None)


def _mss(nat, b, batch=2, sizes=(64,), short=0, ws_align=16, stride=300):
    lib, a = nat.load(), _some(600)
    wins = [torch.hann_window(max(s, 64), device=device()) for s in sizes]
    csizes, wptr = (ctypes.c_int * len(sizes))(*sizes), (ctypes.c_void_p * len(sizes))(*[w.data_ptr() for w in wins])
    need = int(lib.sot_mss_workspace_bytes(2, 300, ctypes.cast((ctypes.c_int * 1)(64), ctypes.c_void_p), 1))
    return lib.sot_mss_loss_and_grad(a.data_ptr(), stride, a.data_ptr(), stride, batch, 300, ctypes.cast(csizes, ctypes.c_void_p), ctypes.cast(wptr, ctypes.c_void_p), len(sizes),
                                     1.0, 1.0, 1e-5, 0, 0, 1.0, b.ptr(), b.ptr(), b.ptr(U8, ws_align), need - short, None)


other("mss-size_4096", "sot_mss_loss_and_grad", UNSUPPORTED)(lambda nat, b: _mss(nat, b, sizes=(4096,)))
other("mss-workspace_one_byte_short", "sot_mss_loss_and_grad", WORKSPACE)(lambda nat, b: _mss(nat, b, short=1))
other("mss-workspace_8_mod_16", "sot_mss_loss_and_grad", BAD_SHAPE)(lambda nat, b: _mss(nat, b, ws_align=8))
other("mss-bad_stride", "sot_mss_loss_and_grad", BAD_SHAPE)(lambda nat, b: _mss(nat, b, stride=299))
other("mss-empty_batch", "sot_mss_loss_and_grad", OK_)(lambda nat, b: _mss(nat, b, batch=0))


def _metrics(nat, b, batch=2, n_groups=1, size=64, short=0):
    lib, a, w = nat.load(), _some(600), torch.hann_window(64, device=device())
    csizes, wptr = (ctypes.c_int * 1)(size), (ctypes.c_void_p * 1)(w.data_ptr())
    grp = (nat.SotMetricGroup * 5)()
    for g in grp:
        g.n_sizes, g.mag_weight, g.l2 = 1, 1.0, 0
        g.fft_sizes[0] = size
    need = int(lib.sot_spec_metrics_workspace_bytes(2, 300, ctypes.cast((ctypes.c_int * 1)(64), ctypes.c_void_p), 1, 1))
    return lib.sot_spec_metrics(a.data_ptr(), 300, a.data_ptr(), 300, batch, 300, ctypes.cast(csizes, ctypes.c_void_p), ctypes.cast(wptr, ctypes.c_void_p), 1,
                                ctypes.cast(grp, ctypes.c_void_p), n_groups, 1e-5, 0, b.ptr(), b.ptr(U8, 8), need - short, None)


other("metrics-five_groups", "sot_spec_metrics", BAD_SHAPE)(lambda nat, b: _metrics(nat, b, n_groups=5))
other("metrics-size_32", "sot_spec_metrics", UNSUPPORTED)(lambda nat, b: _metrics(nat, b, size=32))
other("metrics-workspace_one_byte_short", "sot_spec_metrics", WORKSPACE)(lambda nat, b: _metrics(nat, b, short=1))
other("metrics-empty_batch", "sot_spec_metrics", OK_)(lambda nat, b: _metrics(nat, b, batch=0))


def _osc(nat, b, entry, batch=2, k=4):
    lib, f = nat.load(), _some(2 * 40 * 4)
    if entry == "sot_oscillator_bank_forward":
        return lib.sot_oscillator_bank_forward(f.data_ptr(), f.data_ptr(), batch, 40, k, 16000.0, b.ptr(), b.ptr(U8, 8), 1 << 16, None)
    return lib.sot_oscillator_bank_backward(f.data_ptr(), f.data_ptr(), batch, 40, k, 16000.0, f.data_ptr(), b.ptr(), b.ptr(), b.ptr(U8, 8), 1 << 16, 0, None)


for _entry in ("sot_oscillator_bank_forward", "sot_oscillator_bank_backward"):
    other(f"{_entry}-513_sinusoids", _entry, UNSUPPORTED)(lambda nat, b, e=_entry: _osc(nat, b, e, k=513))
    other(f"{_entry}-empty_batch", _entry, OK_)(lambda nat, b, e=_entry: _osc(nat, b, e, batch=0))


def _synth(nat, b, entry, batch=2, samples=40):
    lib, c, w = nat.load(), _some(2 * 4 * 4), torch.hann_window(20, device=device())
    head = (c.data_ptr(), c.data_ptr(), w.data_ptr(), batch, 4, 4, 0, samples, 16000.0)
    if entry == "sot_synth_envelopes_forward":
        return lib.sot_synth_envelopes_forward(*head, b.ptr(), b.ptr(), None)
    if entry == "sot_synth_envelopes_backward":
        return lib.sot_synth_envelopes_backward(*head, _some(2 * 40 * 4).data_ptr(), _some(2 * 40 * 4).data_ptr(), b.ptr(), b.ptr(), None)
    if entry == "sot_synth_forward":
        return lib.sot_synth_forward(*head, b.ptr(), b.ptr(U8, 8), 1 << 16, None)
    return lib.sot_synth_backward(*head, _some(2 * 40).data_ptr(), b.ptr(), b.ptr(), None, b.ptr(U8, 8), 1 << 16, 0, None)


for _entry in ("sot_synth_envelopes_forward", "sot_synth_envelopes_backward", "sot_synth_forward", "sot_synth_backward"):
    other(f"{_entry}-samples_no_multiple_of_frames", _entry, BAD_SHAPE)(lambda nat, b, e=_entry: _synth(nat, b, e, samples=41))
    other(f"{_entry}-empty_batch", _entry, OK_)(lambda nat, b, e=_entry: _synth(nat, b, e, batch=0))


@other("synth_backward-workspace_one_byte_short", "sot_synth_backward", WORKSPACE)
def _(nat, b):
    lib, c, w = nat.load(), _some(2 * 4 * 4), torch.hann_window(20, device=device())
    need = int(lib.sot_synth_workspace_bytes(2, 4, 40, 4, 1))
    return lib.sot_synth_backward(c.data_ptr(), c.data_ptr(), w.data_ptr(), 2, 4, 4, 0, 40, 16000.0, _some(80).data_ptr(), b.ptr(), b.ptr(), None, b.ptr(U8, 8), need - 1, 0, None)


@other("tap_tables-samples_no_multiple_of_frames", "sot_synth_tap_tables", BAD_SHAPE)
def _(nat, b):
    return nat.load().sot_synth_tap_tables(torch.hann_window(20, device=device()).data_ptr(), 4, 41, b.ptr(U8, 8), None)


def _fir(nat, b, entry, batch=2, n_taps=8, stride=50, short=0):
    lib, a, t = nat.load(), _some(100), _some(16)
    if entry == "sot_fir_same_forward":
        return lib.sot_fir_same_forward(a.data_ptr(), stride, t.data_ptr(), n_taps, batch, 50, n_taps, 3 if n_taps > 4 else 0, b.ptr(), None)
    need = int(lib.sot_fir_workspace_bytes(2, 50, 8))
    return lib.sot_fir_same_backward(a.data_ptr(), a.data_ptr(), stride, t.data_ptr(), n_taps, batch, 50, n_taps, 3 if n_taps > 4 else 0, b.ptr(), b.ptr(), b.ptr(U8, 8), need - short, None)


for _entry in ("sot_fir_same_forward", "sot_fir_same_backward"):
    other(f"{_entry}-two_taps", _entry, UNSUPPORTED)(lambda nat, b, e=_entry: _fir(nat, b, e, n_taps=2))
    other(f"{_entry}-bad_stride", _entry, BAD_SHAPE)(lambda nat, b, e=_entry: _fir(nat, b, e, stride=49))
    other(f"{_entry}-empty_batch", _entry, OK_)(lambda nat, b, e=_entry: _fir(nat, b, e, batch=0))
other("sot_fir_same_backward-workspace_one_byte_short", "sot_fir_same_backward", WORKSPACE)(lambda nat, b: _fir(nat, b, "sot_fir_same_backward", short=1))


@pytest.mark.parametrize("rid", list(OTHER_REFUSALS))
def test_refused_calls_write_nothing(rid):
    nat = native()
    fn, status = OTHER_REFUSALS[rid]
    b = Blank()
    assert fn(nat, b) == status
    b.assert_untouched()


# ---- the helper itself, on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", tg.PLANTS, ids=[p.id for p in tg.PLANTS])
def test_guard_helper_reports_a_planted_byte_on_the_device(plant):
    tg.check_plant(device(), plant)


def test_guard_helper_on_the_device():
    tg.check_unwritten_word(device())
    tg.check_workspace(device())
    tg.check_poisoned_pair(device())
