"""-m gpu: the SECOND AND LATER ROWS of a workgroup, on every route of the row kernels.

Every row kernel is persistent: launch_persistent (csrc/sot_host.hpp) starts min(row groups, resident workgroups) workgroups and each
walks rows w, w + grid, w + 2 grid, ... through the same LDS regions.  A loop-carried error -- stale LDS of the previous row, a missing
barrier between two rows, a partial last row group in the wrong barrier -- shows from a workgroup's second row on, and the other tests
reach that row only by the grace of an occupancy figure nobody asserts.  Here the batch forces it:

    a workgroup holds at least four waves and a CU at most 32, so at most R(G) = CUs * 2048 / G rows are resident (G threads per row);
    B = 3 R(G) + 3 rows give every workgroup at least two rows and most of them three, WHATEVER the occupancy query answers,
    and B % ROWS != 0 leaves the last row group partial (ROWS = 2, 4, 8 rows per workgroup).

Rows are heterogeneous (tests/row_kinds.py: nine weight kinds and six position kinds, drawn per row from a hash of the row index), so a row
follows rows of another nature.  Each case asserts, in three modes (p = 1 on the merge kernel, paper mode, p = 3 with dont_normalize):

  1. ROLL INVARIANCE, bit for bit: the call on the batch rolled along dim 0 by 1 and by B // 2 + 1, rolled back, equals the first call under
     torch.equal on every output.  B and hence the route are unchanged; the large shift moves first-iteration rows into later iterations and
     back, the shift by 1 changes a row's slot, wave half and neighbours.  A condition, not a tolerance.
  2. ENDS ALONE: rows [0, c) and [B - c, B), c = min(CUs, 64), as calls of their own (one row group per workgroup) equal the big call's rows
     bit for bit -- where another kernel serves small batches (CASES: ends = "close") within rtol 2e-6, atol 1e-12, the figure of
     tests/test_gpu_parity.py for "same terms, another association".
  3. THE ORACLE on the check sample (first 16 rows, last 16, first and last row of every kind), at the tolerance of the existing test of the
     same route: 1e-5 relative + 1e-12 forward (2e-5 on per-row positions, tests/test_gpu_fuzz.py), 1e-5 of the row's largest gradient entry
     (per-row positions: 2e-4 for p in {1, 2} and 1e-3 for general p, the figures tests/test_gpu_fuzz.py documents for
     tools/r6/fuzz_rowpos.py).  Position gradients and the gradients of the quantile tensors are compared with autograd of the op-for-op
     restatement on the CPU (tests/test_gpu_edge.py: 2e-5; tests/test_quantiles_grad.py: 1e-5 of the row's largest entry) on the sample rows
     whose merged levels and positions hold no exact tie -- at least half of the sample, asserted.

A new row kernel adds a line to CASES.  Not reachable by this method: the 129-bin full kernel below 8192 rows (64 threads per row: R = 32 CUs
= 8192 rows on 256 CUs, and from 8192 rows on the half-wave kernel takes the call), so no batch it serves forces a second row.
"""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import row_kinds as rk
from gpu_util import device, native

pytestmark = pytest.mark.gpu

kFwd1025OneWaveRows = 6144   # csrc/sot_full_fwd.hpp:28
kRt1024OneWaveRows = 8192    # csrc/sot_full_fwd.hpp:29
kHalf129Rows = 8192          # csrc/sot_full_fwd.hip: dispatch_forward_full
kHalf257Rows = 40960         # csrc/sot_full_fwd.hip: dispatch_forward_full

Case = collections.namedtuple("Case", "id family n m G rows cite B lo hi rowpos ends iters extra")


def C(id, family, n, G, rows, cite, m=None, B=None, lo=0, hi=None, rowpos=False, ends="bits", iters="three", **extra):
    return Case(id, family, n, n if m is None else m, G, rows, cite, B, lo, hi, rowpos, ends, iters, extra)


NS = 32    # SOT_FLAG_NO_SPECIALIZE
FWD = "csrc/sot_full_fwd.hip"
RT = "csrc/sot_full_rt_fwd.hip"
BWD = "csrc/sot_full_bwd.hip"
PICK = "csrc/sot_launch.hpp: pick_cfg"
HIP = "csrc/sot_hip.hip"

# id, family, n, G = threads per row, ROWS per workgroup, the dispatch line the case mirrors.  B = 3 R(G) + 3 unless given; lo / hi: the batch
# range in which the route exists; iters: what B guarantees; ends: "bits" where the kernel does not depend on B, "close" where another kernel
# serves the c-row calls.
CASES = [
    # ---- compile-time forward (merge kernels; three modes) ----
    C("fwd512", "fwd", 512, 64, 4, FWD + ": dispatch_forward_full_pow2 (sot_full_fwd.hpp), dispatch_forward_full_g<64, 8, 4>"),
    C("fwd1024", "fwd", 1024, 128, 2, FWD + ": dispatch_forward_full_pow2 (sot_full_fwd.hpp), <128, 8, 2>"),
    C("fwd2048", "fwd", 2048, 256, 1, FWD + ": dispatch_forward_full_pow2 (sot_full_fwd.hpp), <256, 8, 1>"),
    C("fwd4096", "fwd", 4096, 512, 1, FWD + ": dispatch_forward_full_pow2 (sot_full_fwd.hpp), <512, 8, 1>"),
    C("fwd8192", "fwd", 8192, 1024, 1, FWD + ": dispatch_forward_full, <1024, 8, 1>"),
    C("fwd129_half", "fwd", 129, 32, 8, FWD + ": dispatch_forward_full, dispatch_forward_half<5, 8, 129> (HalfRowGeo, sot_full_fwd.hpp)", lo=kHalf129Rows, ends="close"),
    # NOT REACHABLE by this method: FWD: dispatch_forward_full, <64, 3, 4, 129>, the 129-bin full kernel, serves batches below 8192 rows and R(64) = 32 CUs = 8192
    C("fwd257", "fwd", 257, 64, 4, FWD + ": dispatch_forward_full, <64, 5, 4, 257>, below the 40960-row threshold", hi=kHalf257Rows - 1),
    C("fwd257_half", "fwd", 257, 32, 8, FWD + ": dispatch_forward_full, dispatch_forward_half<9, 8, 257>", lo=kHalf257Rows, ends="close"),
    C("fwd513", "fwd", 513, 64, 4, FWD + ": dispatch_forward_full, <64, 9, 4, 513>"),
    # two waves per row exists only below kFwd1025OneWaveRows: the largest batch it takes, 6143 rows > R(128) = 4096: SECOND ONLY
    C("fwd1025_two_wave", "fwd", 1025, 128, 2, FWD + ": dispatch_forward_full, <128, 9, 2, 1025>", B=kFwd1025OneWaveRows - 1, hi=kFwd1025OneWaveRows - 1, iters="second only"),
    C("fwd1025_one_wave", "fwd", 1025, 64, 4, FWD + ": dispatch_forward_full, <64, 17, 4, 1025>", lo=kFwd1025OneWaveRows, ends="close"),
    C("fwd2049", "fwd", 2049, 256, 1, FWD + ": dispatch_forward_full, <256, 9, 1, 2049>"),
    # ---- merge-free forward (p = 1 on one grid: sot_area_full_kernel; one mode) ----
    C("area512", "area", 512, 64, 4, FWD + ": dispatch_area_full_pow2 (sot_full_fwd.hpp), dispatch_area_full_g<64, 8, 4>"),
    C("area1024", "area", 1024, 128, 2, FWD + ": dispatch_area_full_pow2 (sot_full_fwd.hpp), <128, 8, 2>"),
    C("area2048", "area", 2048, 256, 1, FWD + ": dispatch_area_full_pow2 (sot_full_fwd.hpp), <256, 8, 1> (the plain loop: a row's loss is stored behind barrier 1 of the next row)"),
    C("area4096", "area", 4096, 512, 1, FWD + ": dispatch_area_full_pow2 (sot_full_fwd.hpp), <512, 8, 1>"),
    C("area8192", "area", 8192, 1024, 1, FWD + ": dispatch_area_full, <1024, 8, 1>"),
    C("area129_half", "area", 129, 32, 8, FWD + ": dispatch_area_full, dispatch_area_half<5, 8, 129> (every batch size)"),
    C("area257", "area", 257, 64, 4, FWD + ": dispatch_area_full, <64, 5, 4, 257>"),
    C("area513", "area", 513, 64, 4, FWD + ": dispatch_area_full, <64, 9, 4, 513>"),
    C("area1025", "area", 1025, 64, 4, FWD + ": dispatch_area_full, <64, 17, 4, 1025>"),
    C("area2049", "area", 2049, 256, 1, FWD + ": dispatch_area_full, <256, 9, 1, 2049>"),
    # ---- run-time lengths ----
    C("rt2000", "fwd", 2000, 256, 1, RT + ":17 <256, 8, 1, -1> (2048 geometry)"),
    C("rt1500", "fwd", 1500, 192, 1, RT + ":15 <192, 8, 1, -1> (1536 geometry)"),
    C("rt200", "fwd", 200, 64, 4, RT + ":10 <64, 4, 4, -1> (256 geometry)"),
    C("rt1000_one_wave", "fwd", 1000, 64, 4, RT + ":13 <64, 16, 4, -1> (1024 geometry, one wave per row)", lo=kRt1024OneWaveRows, ends="close"),
    # ---- generic kernels (SOT_FLAG_NO_SPECIALIZE), one length per geometry of pick_cfg ----
    C("gen100", "fwd", 100, 64, 4, PICK + " (64, 8)", flags=NS),
    C("gen1100", "fwd", 1100, 128, 2, PICK + " (128, 12)", flags=NS),
    C("gen1800", "fwd", 1800, 256, 1, PICK + " (256, 8)", flags=NS),
    C("gen5000", "fwd", 5000, 1024, 1, PICK + " (1024, 8)", flags=NS),
    C("gen9000", "fwd", 9000, 1024, 1, PICK + " (1024, 16): R = 2 CUs", flags=NS),
    C("gen300x411", "fwd", 300, 64, 4, PICK + " (64, 8), n != m", m=411, flags=NS),
    # ---- per-row positions: the pre-sort kernel (launch_rowpos_sort: one wave per array, 2 B arrays; it loops too: 2 B > 3 * 32 CUs except at
    #      2048 points, where 2 B = 12294 arrays guarantee its second round and, by the launch's own cap of 16 waves per CU, the third) + RP kernels ----
    C("rp512", "fwd", 512, 64, 4, HIP + ": run_forward, full_rp -> dispatch_forward_full_rowpos_g<64>; " + HIP + ": launch_rowpos_sort", rowpos=True),
    C("rp1024", "fwd", 1024, 128, 2, HIP + ": run_forward -> dispatch_forward_full_rowpos_g<128>", rowpos=True),
    C("rp2048", "fwd", 2048, 256, 1, HIP + ": run_forward -> dispatch_forward_full_rowpos_g<256>", rowpos=True),
    C("rp700_generic", "fwd", 700, 128, 2, HIP + ": run_forward, dispatch_forward<true>, " + PICK + " (128, 12)", rowpos=True),
    C("rp2048_stored_perm", "fwd_perm", 2048, 256, 1, HIP + ": setup_launch, row_perm_out, then row_perm_in", rowpos=True),
    C("rp700_stored_perm", "fwd_perm", 700, 128, 2, HIP + ": setup_launch, on the generic gathering kernel", rowpos=True),
    # ---- backward: both gradients / y only ----
    C("bwd512", "bwd", 512, 64, 4, BWD + ": dispatch_backward_full_pow2 (sot_full_bwd.hpp), dispatch_backward_full_g<64, 8, 4>"),
    C("bwd1024", "bwd", 1024, 128, 2, BWD + ": dispatch_backward_full_pow2 (sot_full_bwd.hpp), <128, 8, 2, 0, 1>; y only: the slim layout dispatch_backward_full_y<128, 8, 2, 0, true, 1>"),
    C("bwd2048", "bwd", 2048, 256, 1, BWD + ": dispatch_backward_full_pow2 (sot_full_bwd.hpp), <256, 8, 1, 0, 1>; y only: dispatch_backward_full_y<256, 8, 2> (two rows per workgroup)"),
    C("bwd4096", "bwd", 4096, 512, 1, BWD + ": dispatch_backward_full_pow2 (sot_full_bwd.hpp), <512, 8, 1>"),
    C("bwd129", "bwd", 129, 64, 4, BWD + ": dispatch_backward_full, <64, 3, 4, 129>"),
    C("bwd257", "bwd", 257, 64, 4, BWD + ": dispatch_backward_full, <64, 5, 4, 257>"),
    C("bwd513", "bwd", 513, 64, 4, BWD + ": dispatch_backward_full, <64, 9, 4, 513, 1>; y only: slim"),
    C("bwd1025", "bwd", 1025, 128, 2, BWD + ": dispatch_backward_full, <128, 9, 2, 1025, 1>; y only: slim"),
    C("bwd2049", "bwd", 2049, 256, 1, BWD + ": dispatch_backward_full, <256, 9, 1, 2049, 1>; y only: slim"),
    C("bwd_rt2000", "bwd", 2000, 256, 1, "csrc/sot_full_rt_bwd.hip:21 <256, 8, 1, -1>"),
    C("bwd_rt1500", "bwd", 1500, 192, 1, "csrc/sot_full_rt_bwd.hip:20 <192, 8, 1, -1>"),
    C("bwd_rt200", "bwd", 200, 64, 4, "csrc/sot_full_rt_bwd.hip:15 <64, 4, 4, -1>"),
    C("bwd_rt1000", "bwd", 1000, 128, 2, "csrc/sot_full_rt_bwd.hip:19 <128, 8, 2, -1, 1>; y only :18 slim"),
    C("bwd_gen100", "bwd", 100, 64, 4, PICK + " (64, 8)", flags=NS),
    C("bwd_gen1100", "bwd", 1100, 128, 2, PICK + " (128, 12)", flags=NS),
    C("bwd_gen1800", "bwd", 1800, 256, 1, PICK + " (256, 8)", flags=NS),
    C("bwd_gen2100", "bwd", 2100, 1024, 1, PICK + " (1024, 8): the smallest length of the geometry in round figures (see the note below CASES)", flags=NS),
    C("bwd_gen300x411", "bwd", 300, 64, 4, PICK + " (64, 8), n != m", m=411, flags=NS),
    C("bwd_rp512", "bwd", 512, 64, 4, HIP + ": run_backward, full_rp -> dispatch_backward_full_rowpos_g<64>", rowpos=True),
    C("bwd_rp2048", "bwd", 2048, 256, 1, HIP + ": run_backward -> dispatch_backward_full_rowpos_g<256>", rowpos=True),
    C("bwd_rp700_generic", "bwd", 700, 128, 2, HIP + ": run_backward, dispatch_backward<true>, " + PICK + " (128, 12)", rowpos=True),
    # ---- training form (row losses + d mean / d y from one pass) and the merge-free training form ----
    C("train512", "train", 512, 64, 4, HIP + ": run_backward, row losses from the y-only kernel; " + BWD + ": dispatch_backward_full_pow2 (sot_full_bwd.hpp)"),
    C("train2048", "train", 2048, 256, 1, HIP + ": run_backward; " + BWD + ": dispatch_backward_full_pow2 (sot_full_bwd.hpp)"),
    C("train1025", "train", 1025, 128, 2, HIP + ": run_backward; " + BWD + ": dispatch_backward_full"),
    C("tiefree2048", "tiefree", 2048, 256, 1, HIP + ": run_backward, area -> " + BWD + ": dispatch_area_train, dispatch_area_train_g<256, 8, 1>"),
    C("tiefree1025", "tiefree", 1025, 128, 2, HIP + ": run_backward -> " + BWD + ": dispatch_area_train, dispatch_area_train_g<128, 9, 2, 1025>"),
    # ---- position gradients: one shared and one per-row case per generic geometry whose gradient layout fits the LDS ((1024, 16) does not) ----
    C("posgrad300", "posgrad", 300, 64, 4, "csrc/sot_posgrad.hip:202 setup_launch, " + PICK + " (64, 8)"),
    #      (the longer side picks the geometry; the other side is short because chance ties between the two sides' levels grow with n m / 2^24)
    C("posgrad700x120", "posgrad", 700, 128, 2, PICK + " (128, 12)", m=120),
    C("posgrad1600x100", "posgrad", 1600, 256, 1, PICK + " (256, 8)", m=100),
    C("posgrad2100x90", "posgrad", 2100, 1024, 1, PICK + " (1024, 8)", m=90),
    C("posgrad_rp300", "posgrad", 300, 64, 4, PICK + " (64, 8), per-row positions", rowpos=True),
    C("posgrad_rp700x120", "posgrad", 700, 128, 2, PICK + " (128, 12), per-row positions", m=120, rowpos=True),
    C("posgrad_rp1600x100", "posgrad", 1600, 256, 1, PICK + " (256, 8), per-row positions", m=100, rowpos=True),
    C("posgrad_rp2100x90", "posgrad", 2100, 1024, 1, PICK + " (1024, 8), per-row positions", m=90, rowpos=True),
    # ---- quantile tensors and their gradients: n + m <= 600 keeps the [B, n + m] outputs small, which leaves the geometries (64, 8) and (128, 12) ----
    C("quant300", "quant", 300, 64, 4, HIP + ": sot_w1d_quantiles, run_forward(quant), " + PICK + " (64, 8)"),
    C("quant520x80", "quant", 520, 128, 2, PICK + " (128, 12)", m=80),
    C("quant_rp300", "quant", 300, 64, 4, PICK + " (64, 8), per-row positions", rowpos=True),
    C("quant_rp520x80", "quant", 520, 128, 2, PICK + " (128, 12), per-row positions", m=80, rowpos=True),
    C("quantgrad300", "quantgrad", 300, 64, 4, "csrc/sot_quantgrad.hip:239 setup_launch, " + PICK + " (64, 8)"),
    C("quantgrad520x80", "quantgrad", 520, 128, 2, PICK + " (128, 12)", m=80),
    C("quantgrad_rp300", "quantgrad", 300, 64, 4, PICK + " (64, 8), per-row positions", rowpos=True),
    C("quantgrad_rp520x80", "quantgrad", 520, 128, 2, PICK + " (128, 12), per-row positions", m=80, rowpos=True),
    # ---- ragged rows: lengths 1 ... max_n drawn per row, so long and short rows alternate in a workgroup ----
    C("csr64", "csr", 64, 64, 4, "csrc/sot_csr.hip:39 " + PICK + " (64, 8) of (max_n, max_m)"),
    C("csr500", "csr", 500, 64, 4, "csrc/sot_csr.hip:39 " + PICK + " (64, 8)"),
    # ---- segmented sort: one wave per row (sot_segmented_sort: n <= 2048), i.e. R = 32 CUs rows ----
    C("sort100", "sort", 100, 64, 4, HIP + ": sot_segmented_sort, launch_segmented_sort_wave<2>"),
    C("sort512", "sort", 512, 64, 4, HIP + ": sot_segmented_sort, launch_segmented_sort_wave<8>"),
    C("sort2048", "sort", 2048, 64, 4, HIP + ": sot_segmented_sort, launch_segmented_sort_wave<32>"),
    # ---- the batch mean in the row kernel's last workgroup ----
    C("fused2048", "fused", 2048, 256, 1, HIP + ": run_forward, mean_tail; " + FWD + ": dispatch_area_full_pow2 (sot_full_fwd.hpp) / dispatch_forward_full_pow2 (sot_full_fwd.hpp)"),
    C("fused513", "fused", 513, 64, 4, HIP + ": run_forward, mean_tail; " + FWD + ": dispatch_area_full / dispatch_forward_full"),
]
# Lengths the issue leaves open are the smallest that reach the kernel or geometry (just past the previous geometry's capacity, no multiple of
# the tile).  The generic backward on (1024, 8) first ran at 5000 points as the forward does: paper mode's d / d y came out at 1.065e-5 of the
# row's largest entry from the oracle, over the 1e-5 the existing tests establish on rows of up to 4096 bins -- two float32 evaluations drift
# apart as sqrt(n) (same figure: 2.1e-6 at 200 points, 2.7e-6 at 1000, 3.3e-6 at 1024, 7.7e-6 at 2000), roll and ends were bit-exact.  The
# bound stays; the case moved to the geometry's smallest length, where the loop under test is the same.
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

CLOSE = dict(rtol=2e-6, atol=1e-12)


def ids(*families):
    return [c.id for c in CASES if c.family in families]


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def batch_rows(case):
    """B of a case, and the assertion that it forces what the table says"""
    R = cus() * 2048 // case.G
    B = case.B if case.B is not None else 3 * R + 3
    assert B >= case.lo and (case.hi is None or B <= case.hi), (case.id, B, "the route does not exist at this batch size on this chip")
    assert B > R and (case.iters == "second only" or B >= 3 * R), (case.id, B, R)
    assert case.rows == 1 or B % case.rows != 0, (case.id, B, "the last row group must be partial")
    print(f"{case.id}: {cus()} CUs, R({case.G}) = {R}, B = {B} ({case.iters})")
    return B


def mode_flags(nat, case, name, p, flags):
    """the library's flag word of one mode: p = 1 runs the merge kernels (SOT_FLAG_NO_AREA) except where the case is about the merge-free ones"""
    return flags | case.extra.get("flags", 0) | (nat.FLAG_NO_AREA if p == 1.0 and case.family in ("fwd", "fwd_perm", "bwd", "train") else 0)


def modes_of(case):
    return (("p1_area", 1.0, 8),) if case.family in ("area", "tiefree") else rk.MODES


@functools.lru_cache(maxsize=None)
def batch(B, n, m, rowpos, tie_free=False):
    """The inputs of one shape ON THE DEVICE, made once and never written to: heterogeneous weights, per-row positions of mixed kinds or one
    grid with its plan, upstream gradients, and the check sample.  tie_free: the shares of tests/row_kinds.py for the comparisons with the
    CPU route, which leave tied rows out."""
    nat = native()
    dev = device()
    wshare, pshare, floor = (rk.TIE_FREE_SHARE, rk.TIE_FREE_POSITION_SHARE, 0.25) if tie_free else (rk.WEIGHT_SHARE, rk.POSITION_SHARE, 0.0)
    x, y, wk = rk.make_weights(B, n, m, 7000 + n + m, dev, wshare, floor)
    inp = dict(x=x, y=y, plan=None)
    kinds = [wk]
    if rowpos:
        inp["xpos"], pk = rk.make_positions(B, n, 100 + n, dev, pshare)
        inp["ypos"], _ = rk.make_positions(B, m, 200 + m, dev, pshare)
        kinds.append(pk)
    else:
        inp["xpos"] = torch.linspace(0, 1, n, device=dev)
        inp["ypos"] = torch.linspace(0, 1, m, device=dev)
        inp["plan"] = nat.PositionPlan(inp["xpos"], inp["ypos"])
        assert inp["plan"].same_grid() == (n == m)
    inp["g"] = 0.5 + torch.rand(B, generator=torch.Generator(device=dev).manual_seed(B + n), device=dev)
    inp["sample"] = rk.check_sample(B, *kinds)
    torch.cuda.synchronize()
    return inp


def row_keys(case, inp):
    return [k for k in ("x", "y", "g", "ups", "xlen", "ylen") + (("xpos", "ypos") if case.rowpos or case.family == "csr" else ()) if inp.get(k) is not None]


def _map_rows(case, inp, f):
    out = dict(inp)
    for k in row_keys(case, inp):
        out[k] = [f(t) for t in inp[k]] if isinstance(inp[k], list) else f(inp[k])
    return out


def rolled(case, inp, shift):
    return _map_rows(case, inp, lambda t: torch.roll(t, shift, 0))


def part(case, inp, lo, hi):
    return _map_rows(case, inp, lambda t: t[lo:hi].clone())


# ---- the calls: every function returns a tuple of tensors with one row per batch row ---------------------------------------------------
def _grad_row_problem(nat, inp, p, flags):
    pr = nat.make_problem(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["plan"])
    ws = nat.workspace(pr, inp["x"].device) if nat._needs_workspace(pr, flags, inp["plan"]) else None
    return pr, ws


def call_position_grads(nat, inp, p, flags):
    """sot_w1d_position_grad: the per-row gradients [B, n], [B, m], also for a shared grid (the binding's position_grads sums those over the batch)"""
    x, y = inp["x"], inp["y"]
    gxp, gyp = torch.empty_like(x), torch.empty_like(y)
    pr, ws = _grad_row_problem(nat, inp, p, flags)
    g = inp["g"].contiguous()
    nat.check(nat.load().sot_w1d_position_grad(ctypes.byref(pr), g.data_ptr(), 1, 0.25, gxp.data_ptr(), gyp.data_ptr(), nat._ptr(ws),
                                               ws.numel() if ws is not None else 0, nat.stream_ptr(x.device)), p)
    return gxp, gyp


def call_quantiles_backward(nat, inp, p, flags):
    """sot_w1d_quantiles_backward with all five upstream gradients: per-row (grad_x, grad_y, grad_xpos, grad_ypos)"""
    x, y = inp["x"], inp["y"]
    outs = [torch.empty_like(x), torch.empty_like(y), torch.empty_like(x), torch.empty_like(y)]
    pr, ws = _grad_row_problem(nat, inp, p, flags)
    ups = [u.contiguous() for u in inp["ups"]]
    nat.check(nat.load().sot_w1d_quantiles_backward(ctypes.byref(pr), *[u.data_ptr() for u in ups], *[o.data_ptr() for o in outs], nat._ptr(ws),
                                                    ws.numel() if ws is not None else 0, nat.stream_ptr(x.device)), p)
    return tuple(outs)


TRAIN_GRAD_SCALE = 1.0 / 4096   # the binding's loss_and_grad scales by 1 / B, which would make a row's gradient depend on the batch it is in


def call_loss_and_grad(nat, inp, p, flags):
    """sot_w1d_loss_and_grad with a gradient scale of its own: (row losses, d / d y)"""
    x, y = inp["x"], inp["y"]
    B = x.shape[0]
    rows, mean, gy = torch.empty(B, device=x.device), torch.empty((), device=x.device), torch.empty_like(y)
    pr, ws = _grad_row_problem(nat, inp, p, flags)
    nat.check(nat.load().sot_w1d_loss_and_grad(ctypes.byref(pr), rows.data_ptr(), float(B), mean.data_ptr(), None, TRAIN_GRAD_SCALE, gy.data_ptr(), None,
                                               nat._ptr(ws), ws.numel() if ws is not None else 0, nat.stream_ptr(x.device)), p)
    return rows, gy


def csr_of(inp):
    def flat(rows, lens):
        keep = torch.arange(rows.shape[1], device=rows.device)[None, :] < lens[:, None]
        off = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=rows.device)
        off[1:] = torch.cumsum(lens, 0)
        return keep, off
    kx, xoff = flat(inp["x"], inp["xlen"])
    ky, yoff = flat(inp["y"], inp["ylen"])
    return inp["x"][kx], inp["xpos"][kx], xoff, inp["y"][ky], inp["ypos"][ky], yoff


def run(nat, case, inp, p, flags, need_gx=True):
    x, y, xpos, ypos, plan = inp["x"], inp["y"], inp["xpos"], inp["ypos"], inp["plan"]
    fam = case.family
    if fam in ("fwd", "area"):
        return (nat.forward_rows(x, y, xpos, ypos, p, flags, plan),)
    if fam == "fwd_perm":
        perm = nat.row_permutations(x, y, xpos, ypos, flags)
        first = nat.forward_rows(x, y, xpos, ypos, p, flags, None, perm_out=perm)
        again = nat.forward_rows(x, y, xpos, ypos, p, flags, None, perm_in=perm)
        return first, perm.view(torch.int16), again
    if fam == "bwd":
        gx, gy = nat.backward_rows(x, y, xpos, ypos, p, flags, inp["g"], need_gx=need_gx, plan=plan, grad_scale=0.25)
        assert (gx is None) == (not need_gx)
        return (gx, gy) if need_gx else (gy,)
    if fam in ("train", "tiefree"):
        return call_loss_and_grad(nat, inp, p, flags | (nat.FLAG_TIE_FREE_GRADIENT if fam == "tiefree" else 0))
    if fam == "posgrad":
        return call_position_grads(nat, inp, p, flags)
    if fam == "quant":
        return tuple(nat.quantiles(x, y, xpos, ypos, p, flags, plan))
    if fam == "quantgrad":
        return call_quantiles_backward(nat, inp, p, flags)
    if fam == "csr":
        return (nat.forward_rows_csr(*csr_of(inp), case.n, case.m, p, flags),)
    if fam == "sort":
        return tuple(nat.segmented_sort(x))
    raise ValueError(fam)


def assert_rows_equal(case, what, got, want, lo=0):
    for k, (a, b) in enumerate(zip(got, want)):
        if not torch.equal(a, b):
            bad = torch.nonzero((a != b).reshape(a.shape[0], -1).any(1)).flatten()
            diff = (a.double() - b.double()).abs().max()
            raise AssertionError(f"{case.id} {what}: output {k} differs on {bad.numel()} of {a.shape[0]} rows, first rows {(bad[:8] + lo).tolist()}, "
                                 f"largest difference {float(diff):.3e}")


def check_roll_and_ends(nat, case, inp, p, flags, base, **kw):
    B = inp["x"].shape[0]
    for shift in (1, B // 2 + 1):
        again = run(nat, case, rolled(case, inp, shift), p, flags, **kw)
        assert_rows_equal(case, f"rolled by {shift}", [torch.roll(t, -shift, 0) for t in again], base)
    c = min(cus(), 64)
    for lo, hi in ((0, c), (B - c, B)):
        alone = run(nat, case, part(case, inp, lo, hi), p, flags, **kw)
        if case.ends == "bits":
            assert_rows_equal(case, f"rows [{lo}, {hi}) alone", alone, [t[lo:hi] for t in base], lo)
        else:
            for a, b in zip(alone, base):
                torch.testing.assert_close(a, b[lo:hi], **CLOSE)


# ---- references on the check sample ----------------------------------------------------------------------------------------------------
def sample_arrays(case, inp):
    s = inp["sample"].to(inp["x"].device)
    xc, yc = inp["x"][s].cpu(), inp["y"][s].cpu()
    if case.rowpos:
        return s, xc, yc, inp["xpos"][s].cpu(), inp["ypos"][s].cpu()
    return s, xc, yc, inp["xpos"].cpu(), inp["ypos"].cpu()


def forward_tolerance(case):
    return 2e-5 if case.rowpos or case.family == "csr" else 1e-5


def assert_forward(case, label, got, want):
    got, want = got.astype(np.float64), want.astype(np.float64)
    err = np.abs(got - want)
    rel = float(np.max(err / np.maximum(np.abs(want), 1e-30) * (err > 1e-12)))
    print(f"{case.id} {label}: rows against the oracle, worst relative error {rel:.3e}")
    assert np.all(err <= forward_tolerance(case) * np.abs(want) + 1e-12), (case.id, label, rel)


def assert_gradient(case, label, got, want, tol):
    scale = np.abs(want).max(axis=1, keepdims=True) + 1e-30
    per_row = np.max(np.abs(got.astype(np.float64) - want) / scale, axis=1)
    worst = float(per_row.max())
    print(f"{case.id} {label}: worst error / row's largest entry {worst:.3e} (compared row {int(per_row.argmax())} of {len(per_row)})")
    assert worst <= tol, (case.id, label, worst, int(per_row.argmax()))


def gradient_tolerance(case, p):
    if case.rowpos:
        return 2e-4 if p in (1.0, 2.0) else 1e-3    # tests/test_gpu_fuzz.py: test_random_per_row_position_cases_on_every_route
    return 1e-5


def restatement_kwargs(p, flags):
    return dict(p=p, square_dist=bool(flags & 1), dont_normalize=bool(flags & 2), limit_quantile_range=bool(flags & 4), require_sort=bool(flags & 8))


def tie_free_rows(case, xc, yc, xp, yp, p, flags):
    """Sample rows whose merged levels (on the CPU route) and positions hold no exact tie; at least half of the sample."""
    from oracle import torch_restatement as tr
    Q = tr.sot_loss(xc, yc, xp, yp, return_quantiles=True, **restatement_kwargs(p, flags))[2]
    tied = (Q[:, 1:] == Q[:, :-1]).any(1)
    for pos in (xp, yp):
        if pos.ndim == 2:
            srt = torch.sort(pos, 1)[0]
            tied |= (srt[:, 1:] == srt[:, :-1]).any(1)
    keep = ~tied
    assert 2 * int(keep.sum()) >= keep.numel(), (case.id, int(keep.sum()), keep.numel())
    return keep


def expand_positions(pos, rows):
    return pos.clone() if pos.ndim == 2 else pos.unsqueeze(0).expand(rows, -1).clone()


# ---- the tests -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ids("fwd", "area", "fwd_perm", "csr"))
def test_forward_rows(name):
    from oracle import sot_oracle as so
    nat = native()
    case = BY_ID[name]
    B = batch_rows(case)
    inp = csr_batch(B, case.n, case.m) if case.family == "csr" else batch(B, case.n, case.m, case.rowpos)
    wants = {}
    for label, p, oflags in modes_of(case):
        flags = mode_flags(nat, case, label, p, oflags)
        if case.family == "area":
            assert nat.problem_flags(p, flags, inp["plan"]) & nat.FLAG_SAME_GRID
        base = run(nat, case, inp, p, flags)
        assert all(torch.isfinite(t.float()).all() for t in base)
        check_roll_and_ends(nat, case, inp, p, flags, base)
        if case.family == "csr":
            s = inp["sample"]
            xl, yl = inp["xlen"].cpu(), inp["ylen"].cpu()
            dev = inp["x"].device
            xw, xp, yw, yp = (inp[k][s.to(dev)].cpu().numpy() for k in ("x", "xpos", "y", "ypos"))
            want = np.array([so.forward(xw[i:i + 1, :xl[r]], yw[i:i + 1, :yl[r]], xp[i:i + 1, :xl[r]], yp[i:i + 1, :yl[r]], p=p, flags=oflags)[0]
                             for i, r in enumerate(s.tolist())])
        else:
            s, xc, yc, xp, yp = sample_arrays(case, inp)
            want = so.forward(xc.numpy(), yc.numpy(), xp.numpy(), yp.numpy(), p=p, flags=oflags)
        wants[label] = want.astype(np.float64)
        assert_forward(case, label, base[0][s.to(base[0].device)].cpu().numpy(), want)
        if case.family == "fwd_perm":
            assert torch.equal(base[0], base[2]), "the stored permutations give other rows than the sort that stored them"
            perm = base[1][s.to(base[1].device)].cpu().numpy().view(np.uint16).astype(np.int64)
            assert np.array_equal(perm[:, :case.n], np.argsort(xp.numpy(), axis=1, kind="stable"))
            assert np.array_equal(perm[:, case.n:], np.argsort(yp.numpy(), axis=1, kind="stable"))
    # the sample tells the modes apart: a kernel of another mode cannot pass the comparison above (tests/test_row_kinds.py)
    labels = list(wants)
    for i, a in enumerate(labels):
        for b in labels[i + 1:]:
            sep = np.abs(wants[a] - wants[b]) / np.maximum(np.maximum(wants[a], wants[b]), 1e-300)
            assert np.mean(sep >= 1e-3) >= 0.5, (a, b, float(np.mean(sep >= 1e-3)))


@functools.lru_cache(maxsize=None)
def csr_batch(B, max_n, max_m):
    """Ragged rows as padded arrays + lengths (the CSR arrays are cut from them per call, so a rolled batch is rebuilt in rolled order)."""
    dev = device()
    inp = batch(B, max_n, max_m, True)
    rows = torch.arange(B, dtype=torch.int64, device=dev)
    out = dict(inp)
    out["xlen"] = 1 + rk.row_hash(rows, 0xA11) % max_n
    out["ylen"] = 1 + rk.row_hash(rows, 0xB22) % max_m
    return out


@pytest.mark.parametrize("need_gx", [True, False], ids=["both", "y_only"])
@pytest.mark.parametrize("name", ids("bwd"))
def test_backward_rows(name, need_gx):
    from oracle import sot_oracle as so
    nat = native()
    case = BY_ID[name]
    inp = batch(batch_rows(case), case.n, case.m, case.rowpos)
    s, xc, yc, xp, yp = sample_arrays(case, inp)
    for label, p, oflags in modes_of(case):
        flags = mode_flags(nat, case, label, p, oflags)
        base = run(nat, case, inp, p, flags, need_gx=need_gx)
        assert all(torch.isfinite(t).all() for t in base)
        check_roll_and_ends(nat, case, inp, p, flags, base, need_gx=need_gx)
        wx, wy = so.backward(xc.numpy(), yc.numpy(), xp.numpy(), yp.numpy(), (0.25 * inp["g"][s]).cpu().numpy(), p=p, flags=oflags)
        for which, got, want in zip(("gx", "gy") if need_gx else ("gy",), base, (wx, wy) if need_gx else (wy,)):
            assert_gradient(case, f"{label} {which}", got[s].cpu().numpy(), want, gradient_tolerance(case, p))


@pytest.mark.parametrize("name", ids("train", "tiefree"))
def test_training_form(name):
    from oracle import sot_oracle as so
    nat = native()
    case = BY_ID[name]
    B = batch_rows(case)
    inp = batch(B, case.n, case.m, False, case.family == "tiefree")
    s, xc, yc, xp, yp = sample_arrays(case, inp)
    for label, p, oflags in modes_of(case):
        flags = mode_flags(nat, case, label, p, oflags)
        base = run(nat, case, inp, p, flags)
        assert all(torch.isfinite(t).all() for t in base)
        check_roll_and_ends(nat, case, inp, p, flags, base)
        want, dbg = so.forward(xc.numpy(), yc.numpy(), xp.numpy(), yp.numpy(), p=p, flags=oflags, debug=True)
        assert_forward(case, label, base[0][s].cpu().numpy(), want)
        _, wy = so.backward(xc.numpy(), yc.numpy(), xp.numpy(), yp.numpy(), np.full(len(s), TRAIN_GRAD_SCALE, np.float32), p=p, flags=oflags)
        got = base[1][s].cpu().numpy()
        if case.family == "tiefree":
            # at exactly tied levels this kernel returns the derivative in the CDF values, the oracle the reference's tie order
            # (tests/test_gpu_parity.py: test_merge_free_training_form_p1): the oracle is the yardstick on the rows without a tie.  Normalised
            # rows of ~2000 bins are tied more often than not (both CDFs end at 1; n m / 2^24 chance meetings), so the batch has the shares of
            # the CPU-route comparisons, and a quarter of the sample -- ten rows, each a full check of the row's arithmetic -- must remain.
            keep = ~(dbg["Q"][:, 1:] == dbg["Q"][:, :-1]).any(1)
            print(f"{case.id}: {int(keep.sum())} of {len(keep)} sample rows tie-free")
            assert 4 * int(keep.sum()) >= len(keep), (int(keep.sum()), len(keep))
            got, wy = got[keep], wy[keep]
        assert_gradient(case, f"{label} gy", got, wy, 1e-5)


@pytest.mark.parametrize("name", ids("posgrad"))
def test_position_grads(name):
    from oracle import torch_restatement as tr
    nat = native()
    case = BY_ID[name]
    inp = batch(batch_rows(case), case.n, case.m, case.rowpos, True)
    s, xc, yc, xp, yp = sample_arrays(case, inp)
    up = (0.25 * inp["g"][s]).cpu()
    for label, p, oflags in rk.MODES:
        flags = mode_flags(nat, case, label, p, oflags)
        base = run(nat, case, inp, p, flags)
        assert all(torch.isfinite(t).all() for t in base)
        check_roll_and_ends(nat, case, inp, p, flags, base)
        xpr, ypr = expand_positions(xp, len(s)).requires_grad_(True), expand_positions(yp, len(s)).requires_grad_(True)
        keep = tie_free_rows(case, xc, yc, xpr.detach(), ypr.detach(), p, oflags)
        (tr.sot_loss(xc, yc, xpr, ypr, reduce=False, **restatement_kwargs(p, oflags)) * up).sum().backward()
        for which, got, want in (("gxpos", base[0], xpr.grad), ("gypos", base[1], ypr.grad)):
            assert_gradient(case, f"{label} {which} ({int(keep.sum())} of {len(keep)} sample rows tie-free)", got[s].cpu().numpy()[keep.numpy()],
                            want.numpy()[keep.numpy()].astype(np.float64), 2e-5)


def quantile_upstreams(B, n, m):
    dev = device()
    g = torch.Generator(device=dev).manual_seed(31 * n + m)
    return [torch.randn(B, k, generator=g, device=dev) for k in (n + m, n + m, n + m, n, m)]


@pytest.mark.parametrize("name", ids("quant"))
def test_quantile_tensors(name):
    """U and V against the CPU restatement; Q, uq and vq EXACTLY what the reference's operations (sort of the merged levels, left rank,
    clamp, lookup: oracle/torch_restatement.py inverse_cdf) make of the kernel's own U and V -- no tie can excuse a difference there."""
    from oracle import torch_restatement as tr
    nat = native()
    case = BY_ID[name]
    inp = batch(batch_rows(case), case.n, case.m, case.rowpos)
    s, xc, yc, xp, yp = sample_arrays(case, inp)
    # the reference's operations behind a STABLE position sort (the kernels' order between equal positions; torch's default sort has none)
    (xps, ox), (yps, oy) = (torch.sort(expand_positions(pos, len(s)), dim=1, stable=True) for pos in (xp, yp))
    xcs, ycs = torch.gather(xc, 1, ox), torch.gather(yc, 1, oy)
    for label, p, oflags in rk.MODES:
        flags = mode_flags(nat, case, label, p, oflags) & ~nat.FLAG_NO_AREA
        base = run(nat, case, inp, p, flags)
        assert all(torch.isfinite(t).all() for t in base)
        check_roll_and_ends(nat, case, inp, p, flags, base)
        uq, vq, Q, U, V = (t[s].cpu() for t in base)
        ref = tr.sot_loss(xcs, ycs, xps, yps, return_quantiles=True, **dict(restatement_kwargs(p, oflags), require_sort=False))
        for which, got, want in (("U", U, ref[3]), ("V", V, ref[4])):
            assert_gradient(case, f"{label} {which}", got.numpy(), want.numpy().astype(np.float64), 1e-5)
        assert torch.equal(Q, torch.sort(torch.cat((U, V), 1), 1)[0]), label
        assert torch.equal(uq, tr.inverse_cdf(Q, U, xps)) and torch.equal(vq, tr.inverse_cdf(Q, V, yps)), label


@pytest.mark.parametrize("name", ids("quantgrad"))
def test_quantile_gradients(name):
    from oracle import torch_restatement as tr
    nat = native()
    case = BY_ID[name]
    B = batch_rows(case)
    inp = dict(batch(B, case.n, case.m, case.rowpos, True))
    inp["ups"] = quantile_upstreams(B, case.n, case.m)
    s, xc, yc, xp, yp = sample_arrays(case, inp)
    ws = [u[s].cpu() for u in inp["ups"]]
    for label, p, oflags in rk.MODES:
        flags = mode_flags(nat, case, label, p, oflags) & ~nat.FLAG_NO_AREA
        base = run(nat, case, inp, p, flags)
        assert all(torch.isfinite(t).all() for t in base)
        check_roll_and_ends(nat, case, inp, p, flags, base)
        leaves = [xc.clone().requires_grad_(True), yc.clone().requires_grad_(True), expand_positions(xp, len(s)).requires_grad_(True),
                  expand_positions(yp, len(s)).requires_grad_(True)]
        keep = tie_free_rows(case, xc, yc, leaves[2].detach(), leaves[3].detach(), p, oflags).numpy()
        outs = tr.sot_loss(*leaves, return_quantiles=True, **restatement_kwargs(p, oflags))
        sum((o * w).sum() for o, w in zip(outs, ws)).backward()
        for which, got, leaf in zip(("gx", "gy", "gxpos", "gypos"), base, leaves):
            assert_gradient(case, f"{label} {which} ({int(keep.sum())} of {len(keep)} sample rows tie-free)", got[s].cpu().numpy()[keep],
                            leaf.grad.numpy()[keep].astype(np.float64), 1e-5)


@pytest.mark.parametrize("name", ids("sort"))
def test_segmented_sort(name):
    """Keys of every position kind (sorted, reversed, random, all equal, clustered, duplicated): values and indices of torch.sort(stable=True)."""
    nat = native()
    case = BY_ID[name]
    B = batch_rows(case)
    keys, kinds = rk.make_positions(B, case.n, 300 + case.n, device())
    inp = dict(x=keys, y=None, xpos=None, ypos=None, plan=None)
    base = run(nat, case, inp, 1.0, 0)
    check_roll_and_ends(nat, case, inp, 1.0, 0, base)
    s = rk.check_sample(B, kinds).to(keys.device)
    want_v, want_i = torch.sort(keys[s].cpu(), dim=1, stable=True)
    assert torch.equal(base[0][s].cpu(), want_v) and torch.equal(base[1][s].cpu(), want_i)


@pytest.mark.parametrize("name", ids("fused"))
def test_fused_mean(name):
    """loss_fused(fused_mean=True): the rows of the two-kernel call bit for bit (and roll-invariant), the mean within 1e-6 relative of the float64
    mean of its own rows (its summation order depends on the row index: not part of the roll test), the counter pool zero afterwards."""
    nat = native()
    case = BY_ID[name]
    B = batch_rows(case)
    inp = batch(B, case.n, case.m, False)
    for label, p, oflags in (("p1_area", 1.0, 8),) + rk.MODES:
        flags = oflags | (nat.FLAG_NO_AREA if label == "p1" else 0)

        def fused(i):
            return nat.loss_fused(i["x"], i["y"], i["xpos"], i["ypos"], p, flags, i["plan"], fused_mean=True)
        mean, rows, _ = fused(inp)
        _, two, _ = nat.loss_fused(inp["x"], inp["y"], inp["xpos"], inp["ypos"], p, flags, inp["plan"], fused_mean=False)
        assert torch.equal(rows, two), (label, float((rows - two).abs().max()))
        for shift in (1, B // 2 + 1):
            _, again, _ = fused(rolled(case, inp, shift))
            assert_rows_equal(case, f"{label} rolled by {shift}", [torch.roll(again, -shift, 0)], [rows])
        want = float(rows.double().mean())
        print(f"{case.id} {label}: mean against the float64 mean of its rows {abs(float(mean) - want) / abs(want):.3e}")
        assert abs(float(mean) - want) <= 1e-6 * abs(want), (label, float(mean), want)
        torch.cuda.synchronize()
        for buf, _ in nat._counter_pools.values():
            assert int(buf.abs().sum()) == 0, "completion counters must be left zero"
    assert nat._counter_pools, "the fused mean did not use the counter pool"
