#!/usr/bin/env python3
"""bench.py -- SOT-loss evaluations/s on [B, N_fft] spectrum pairs (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the line: the contract fields, `config` and the headline kernel's
`roofline` (measured inside the timed region).  --full adds everything that takes runs of its own: the roofline side kernels
(paper mode, merge pipeline, training form), the two-stream and stream-event timings, the secondary workloads under `extras`
(unless --no-extras), the CPU baseline (unless --no-cpu-baseline) and the parity check against the stored reference scalar.
--dump-outputs DIR writes what the last timed step returned (DIR/loss.npy, DIR/row_losses.npy) for output-for-output comparisons.

N = 1 runs in this process.  N > 1: when the process is not already a rank (no RANK in the environment) it starts N fresh
rank processes -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 bench.py ...` as a
CHILD process, before anything here touches a GPU -- forwards rank 0's JSON line and exits with the children's return
code; when it already is a rank (the driver launches it that way) WORLD_SIZE must equal --gpus.  Fewer visible GPUs than
N is an error (non-zero exit), never a 1-GPU number.

A "step" is one pass of the hot path over one batch of synthetic spectrum pairs already resident in
HBM: Wasserstein1D forward (fused HIP kernel + fixed-order mean).  With N>1 every rank owns its own
B rows (weak scaling, no data-path collective) and the step ends with ONE RCCL all-reduce of the
scalar partial sum.  Inputs rotate over several distinct sets so that the 256 MiB Infinity Cache
cannot serve them.

Rank 0 prints ONE JSON line with the contract fields plus
  roofline     -- dominant kernel (sot_forward_full_kernel: the forward specialised for rows that fill their geometry): algorithmic bytes per launch / average launch
                  duration measured live with HIP events attached to its dispatches inside the timed region;
  cpu_baseline -- (--full) the op-for-op torch restatement of the reference (oracle/torch_restatement.py,
                  kind "port") timed on this host's cores on a bounded sample of the same workload.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

MODES = {
    "p1": dict(p=1),  # north_star: L1-normalised Wasserstein-1
    "cutoff": dict(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True),  # paper SOT-2048
    "nocut": dict(p=2, square_dist=True),
}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md "Chip-level parameters": HBM3E 8.0 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--prewarm", type=int, default=400,
                    help="untimed steps before the W warm-up steps: the first few hundred launches run ~10 %% slower (clock ramp)")
    ap.add_argument("--rows", type=int, default=8192, help="rows (spectrum pairs) per GPU")
    ap.add_argument("--nfft", type=int, default=2048, help="row length N")
    ap.add_argument("--mode", choices=list(MODES), default="p1")
    ap.add_argument("--sets", type=int, default=6, help="distinct rotating input sets (>= 4 defeats the 256 MiB L3)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--graph-steps", action="store_true", help="replay each step from a HIP graph (opt-in)")
    ap.add_argument("--lanes", type=int, default=0, choices=[0, 1, 2],
                    help="HIP streams the steps alternate over: 1 = one stream; 2 = the mean kernel / all-reduce of a step "
                         "overlaps the next step's forward kernel; 0 (default) = 1 on one GPU (per-kernel times then agree "
                         "with rocprofv3), 2 when there is a collective to hide (N > 1)")
    ap.add_argument("--cpu-rows", type=int, default=8192)   # all rows of the headline workload (set 0); ~15 s of CPU work
    ap.add_argument("--no-extras", action="store_true", help="skip the secondary workloads reported under `extras` (with --full)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: roofline side kernels, two-stream / stream-event timings, the "
                         "secondary workloads, the CPU baseline and the parity check (off: only the headline figure)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (loss, row losses) as DIR/<name>.npy")
    ap.add_argument("--global-rows", type=int, default=0,
                    help="STRONG scaling (BASELINE config 3: 65536): the total batch is fixed and every rank takes global / N rows "
                         "(shard r = the rows [r, r + 1) * global / N of the 8 x 8192-row blocks seeded 1234 + block); overrides --rows")
    return resolve_rows(ap.parse_args())


def resolve_rows(args):
    """--global-rows G: rows per rank = G / N (must divide); `scaling` is then "strong" (total work fixed as N grows)."""
    args.scaling = "weak"
    if args.global_rows:
        if args.global_rows % args.gpus:
            sys.exit(f"bench.py: --global-rows {args.global_rows} is not a multiple of --gpus {args.gpus}")
        args.rows = args.global_rows // args.gpus
        args.scaling = "strong"
    return args


# kernel the shared-position forward dispatches for a row length (csrc/sot_forward_full.inc: dispatch_forward_full):
# threads per row, contiguous elements per thread, rows per workgroup, compile-time row length (0: the row fills its geometry)
FULL_ROW_GEOMETRY = {512: (64, 8, 4, 0), 1024: (128, 8, 2, 0), 2048: (256, 8, 1, 0), 4096: (512, 8, 1, 0), 8192: (1024, 8, 1, 0),
                     129: (64, 3, 4, 129), 257: (64, 5, 4, 257), 513: (64, 9, 4, 513), 1025: (128, 9, 2, 1025), 2049: (256, 9, 1, 2049)}


def forward_kernel_name(n, mode, backward=False, same_grid=True, batch=0):
    """Name of the dominant kernel as rocprofv3 lists it (template arguments G, CPT, ROWS, PM, LIM, SQ, NX[, WANT_X, SLIM]); `batch`: rows
    of the launch (large batches of 1025-bin / <= 1024-point rows run the merge forward with one wave per row)."""
    c = MODES[mode]
    pm, lim, sq = int(c.get("p", 1)), bool(c.get("limit_quantile_range", False)), bool(c.get("square_dist", False))
    geo = FULL_ROW_GEOMETRY.get(n)
    b = lambda v: "true" if v else "false"  # noqa: E731
    if geo is None:   # any other length: the next capacity's geometry with the length at run time (NX = -1), backward up to 4096
        cap = next((c for c in (256, 512, 1024, 1536, 2048, 3072, 4096, 8192) if n <= c), None) if n > 128 else None
        if cap is None or (backward and cap > 4096):
            return "sot_backward_kernel (generic)" if backward else "sot_forward_kernel (generic)"
        g, cpt, rows = {256: (64, 4, 4), 512: (64, 8, 4), 1024: (128, 8, 2), 1536: (192, 8, 1), 2048: (256, 8, 1), 3072: (384, 8, 1), 4096: (512, 8, 1),
                        8192: (1024, 8, 1)}[cap]
        pmt = pm if pm in (1, 2) else 0
        if pm == 1 and not lim and not backward and same_grid:
            if cap == 1024:
                g, cpt, rows = 64, 16, 4      # one wave per row
            return f"sot_area_full_kernel<{g}, {cpt}, {rows}, {b(sq)}, -1>"
        if backward:   # y-only (training) kernel; the 1024-point geometry in the layout without U gradient slots, capped at 128 VGPRs
            tail = "false, true, 4" if cap == 1024 else "false, false, 1"
            return f"sot_backward_full_kernel<{g}, {cpt}, {rows}, {pmt}, {b(lim)}, {b(sq)}, -1, {tail}, false>"
        if cap == 1024 and batch >= 8192:
            g, cpt, rows = 64, 16, 4
        return f"sot_forward_full_kernel<{g}, {cpt}, {rows}, {pmt}, {b(lim)}, {b(sq)}, -1, false>"
    if pm not in (1, 2):
        pm = 0
    g, cpt, rows, nx = geo
    if pm == 1 and not lim and not backward and same_grid:   # p = 1 on one grid: the merge-free kernel (sot_area_full_kernel)
        if n == 1025:
            g, cpt, rows = 64, 17, 4          # one wave per row
        if n == 129:
            return f"sot_area_half_kernel<5, 8, {b(sq)}, 129>"    # two rows per wave
        return f"sot_area_full_kernel<{g}, {cpt}, {rows}, {b(sq)}, {nx}>"
    if backward:   # the y-only (training) kernels <..., WANT_X, SLIM, MINB>: 2048-bin rows run two per workgroup in the layout without
        # U gradient slots, 1025- and 513-bin rows in that layout compiled for four workgroups per CU
        if n == 2048:
            return f"sot_backward_full_kernel<{g}, {cpt}, 2, {pm}, {b(lim)}, {b(sq)}, {nx}, false, true, 1, false>"
        if n in (1025, 513):
            return f"sot_backward_full_kernel<{g}, {cpt}, {rows}, {pm}, {b(lim)}, {b(sq)}, {nx}, false, true, 4, false>"
        if n in (1024, 2049):
            return f"sot_backward_full_kernel<{g}, {cpt}, {rows}, {pm}, {b(lim)}, {b(sq)}, {nx}, false, true, 1, false>"
        return f"sot_backward_full_kernel<{g}, {cpt}, {rows}, {pm}, {b(lim)}, {b(sq)}, {nx}, false, false, 1, false>"
    if (n == 257 and batch >= 40960) or (n == 129 and batch >= 8192):   # two rows per wave
        return f"sot_forward_half_kernel<{9 if n == 257 else 5}, 8, {pm}, {b(lim)}, {b(sq)}, {n}>"
    if n == 1025 and batch >= 6144:
        g, cpt, rows = 64, 17, 4
    return f"sot_forward_full_kernel<{g}, {cpt}, {rows}, {pm}, {b(lim)}, {b(sq)}, {nx}, false>"


def global_batch_rows(first, count, n, block=8192):
    """Rows [first, first + count) of BASELINE config 3's global batch: consecutive blocks of `block` rows, block k drawn with the CPU
    generator seeded 1234 + k (x before y) -- what the 8 ranks of the weak-scaling run hold, cut differently for fewer ranks."""
    from sot_amd.bench_inputs import spectrum_pairs
    xs, ys = [], []
    k = first // block
    while k * block < first + count:
        x, y = spectrum_pairs("uniform", block, n, n, 1234 + k)
        lo, hi = max(first, k * block) - k * block, min(first + count, (k + 1) * block) - k * block
        xs.append(x[lo:hi])
        ys.append(y[lo:hi])
        k += 1
    return torch.cat(xs).contiguous(), torch.cat(ys).contiguous()


def launcher_command(gpus, argv, port, python=None):
    """The child command that starts `gpus` rank processes of this script (one per GPU) on this node."""
    return [python or sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *argv]


def visible_gpus():
    """Number of GPUs a child process would see, counted WITHOUT the HIP runtime (the parent of the rank processes must not
    initialise a GPU): the visibility variables if set, else the KFD topology (nodes with SIMDs are GPUs); only when neither
    exists, torch.cuda.device_count() (which may fall back to hipGetDeviceCount)."""
    import glob
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([t for t in v.split(",") if t.strip() != ""])
    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if nodes:
        count = 0
        for path in nodes:
            try:
                for line in open(path):
                    if line.startswith("simd_count") and int(line.split()[1]) > 0:
                        count += 1
            except OSError:
                pass
        return count
    return torch.cuda.device_count()


def launch_ranks(args, argv):
    """--gpus N > 1 from a plain process: start the N ranks as a child process tree and forward its output.  Nothing in
    this (parent) process initialises a GPU (visible_gpus() reads the environment / sysfs)."""
    import socket
    import subprocess
    visible = visible_gpus()
    if visible < args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} requested but only {visible} GPU(s) are visible; refusing to report a "
                         f"{visible}-GPU number as a {args.gpus}-GPU one\n")
        return 3
    with socket.socket() as sk:  # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this host driver
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.run(launcher_command(args.gpus, argv, port), env=env)  # stdout/stderr inherited: rank 0's JSON line passes through
    return proc.returncode


def other_workloads(dev, nat, sets, pos_x, pos_y, timed, n):
    """Secondary measurements outside the contract's timed region (N = 1 only), one entry per workload the README / DESIGN
    quote: each entry carries the call's time (HIP events on the launch stream around n back-to-back calls), the kernel it
    is dominated by, the algorithmic bytes of SURVEY 8(d) and their fraction of the 8 TB/s HBM peak.  Inputs rotate over
    two sets; shapes other than the headline's are smaller than the Infinity Cache and say so ("l3_resident")."""
    from sot_amd import spectra
    from sot_amd.bench_inputs import ragged_supports, spectrum_pairs
    from sot_amd.losses import Wasserstein1D, wasserstein_1d_csr
    out = {}

    def entry(ms, kernel, nbytes, **kw):
        return {"ms": ms, "kernel": kernel, "algorithmic_bytes": nbytes, "achieved_gbs": nbytes / (ms * 1e-3) / 1e9,
                "frac": nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, **kw}

    def sot_entries(tag, rows, nbins, pairs, px, py, l3):
        cut = Wasserstein1D(**MODES["cutoff"]).to(dev)
        cm = [cut._marshal(x, y, px, py, {}) for x, y in pairs]
        one = torch.ones(1, device=dev)
        k = len(cm)

        def fwd(i):
            x2, y2, xp, yp, flags, plan, _ = cm[i % k]
            nat.forward_rows(x2, y2, xp, yp, float(cut.p), flags, plan)

        def fwd_mean(i):
            x2, y2, xp, yp, flags, plan, _ = cm[i % k]
            nat.loss_fused(x2, y2, xp, yp, float(cut.p), flags, plan)

        def fwd_mean_one_kernel(i):   # the same with the mean in the row kernel's last workgroup (opt-in, see include/sot_hip.h)
            x2, y2, xp, yp, flags, plan, _ = cm[i % k]
            nat.loss_fused(x2, y2, xp, yp, float(cut.p), flags, plan, fused_mean=True)

        def bwd_y(i):
            x2, y2, xp, yp, flags, plan, _ = cm[i % k]
            nat.backward_rows(x2, y2, xp, yp, float(cut.p), flags, one, need_gx=False, plan=plan, grad_scale=1.0 / rows)

        def loss_and_grad(i):   # the training form: loss, batch mean and d mean / d y out of one pass over the rows
            x2, y2, xp, yp, flags, plan, _ = cm[i % k]
            nat.loss_and_grad(x2, y2, xp, yp, float(cut.p), flags, plan)

        fb = 4 * 2 * nbins + 4
        with torch.no_grad():
            out[f"{tag}_cutoff_forward"] = entry(timed(fwd, n), forward_kernel_name(nbins, "cutoff", batch=rows), rows * fb, l3_resident=l3)
            out[f"{tag}_cutoff_forward_with_mean"] = entry(timed(fwd_mean, n), forward_kernel_name(nbins, "cutoff", batch=rows) + " + batch mean", rows * fb, l3_resident=l3)
            out[f"{tag}_cutoff_forward_with_in_kernel_mean"] = entry(timed(fwd_mean_one_kernel, n), forward_kernel_name(nbins, "cutoff", batch=rows) + " (mean by its last workgroup)",
                                                                      rows * fb, l3_resident=l3)
            out[f"{tag}_cutoff_backward_y"] = entry(timed(bwd_y, n), forward_kernel_name(nbins, "cutoff", backward=True, batch=rows), rows * (fb + 4 * nbins), l3_resident=l3)
            out[f"{tag}_cutoff_loss_and_grad"] = entry(timed(loss_and_grad, n), forward_kernel_name(nbins, "cutoff", backward=True, batch=rows) + " + batch mean",
                                                       rows * (fb + 4 * nbins), l3_resident=l3)
        return cut

    # (0) the headline workload through the general (merge) kernel: p = 1 on one grid normally takes the merge-free kernel
    B, N = sets[0][0].shape
    p1 = Wasserstein1D(**MODES["p1"]).to(dev)
    pm = [p1._marshal(x, y, pos_x, pos_y, {}) for x, y in sets]

    def p1_merge(i):
        x2, y2, xp, yp, flags, plan, _ = pm[i % len(pm)]
        nat.forward_rows(x2, y2, xp, yp, 1.0, flags | nat.FLAG_NO_AREA, plan)

    with torch.no_grad():
        out[f"b{B}n{N}_p1_forward_merge_kernel"] = entry(timed(p1_merge, n), forward_kernel_name(N, "p1", same_grid=False, batch=B), B * (8 * N + 4),
                                                         l3_resident=False if len(sets) * 2 * B * N * 4 > 2**28 else True)

    # (0a') the p = 1 TRAINING FORM (loss, batch mean and d mean / d y in one call) on the headline shape: the default runs the merge walk (the
    #       reference's float32 tie order); with the opt-in SOT_FLAG_TIE_FREE_GRADIENT (Wasserstein1D(..., tie_free_gradient=True)) it is merge-free
    def p1_train(extra):
        def call(i):
            x2, y2, xp, yp, flags, plan, _ = pm[i % len(pm)]
            nat.loss_and_grad(x2, y2, xp, yp, 1.0, flags | extra, plan)
        return call

    with torch.no_grad():
        l3p = False if len(sets) * 2 * B * N * 4 > 2**28 else True
        out[f"b{B}n{N}_p1_loss_and_grad"] = entry(timed(p1_train(0), n), forward_kernel_name(N, "p1", backward=True, batch=B) + " + batch mean (merge walk: the reference's tie order)",
                                                  B * (12 * N + 4), l3_resident=l3p)
        out[f"b{B}n{N}_p1_loss_and_grad_tie_free"] = entry(timed(p1_train(nat.FLAG_TIE_FREE_GRADIENT), n),
                                                           "sot_area_train_kernel<256, 8, 1, false, 0> + batch mean (opt-in: merge-free, derivative in the CDF values at tied levels)"
                                                           if N == 2048 else "sot_area_train_kernel (opt-in)", B * (12 * N + 4), l3_resident=l3p)

    # (0b) the headline workload THROUGH THE MODULE (the timed step is a pre-bound C call): mod(x, y, x_pos=..., y_pos=...)
    #      launched from Python under no_grad, forward + batch mean per call -- the hot-call cache and the C++ host path included
    with torch.no_grad():
        out[f"b{B}n{N}_p1_module_forward"] = entry(timed(lambda i: p1(sets[i % len(sets)][0], sets[i % len(sets)][1], x_pos=pos_x, y_pos=pos_y), n),
                                                   forward_kernel_name(N, "p1", batch=B) + " + batch mean, through Wasserstein1D.forward",
                                                   B * (8 * N + 4), l3_resident=False if len(sets) * 2 * B * N * 4 > 2**28 else True)

    # (0c) the pipeline north_star names literally -- sort of the supports + gather, losses.py:286-290 -- on the headline shape:
    #      (a) an UNSORTED shared grid (a permuted linspace): planned once, the row kernel gathers through the permutation
    #          (bytes as for the sorted grid: 4 (n + m) + 4 per row);
    #      (b) PER-ROW positions (every row its own unsorted grid): the segmented in-LDS bitonic sort with index payload inside the
    #          row kernel (sot_forward_kernel<..., ROWPOS ...>); algorithmic bytes 8 (n + m) + 4 per row
    gperm = torch.Generator().manual_seed(99)
    perm = torch.randperm(N, generator=gperm).to(dev)
    ux, uy = pos_x[perm].contiguous(), pos_y[perm].contiguous()
    uplan = nat.PositionPlan(ux, uy)
    cutflags = 15
    two = sets[:2]

    def unsorted_shared(i):
        x2, y2 = two[i % 2]
        nat.forward_rows(x2, y2, ux, uy, 2.0, cutflags, uplan)

    rows_pr = min(B, 4096)   # per-row positions of the full batch would be another 2 x 67 MB per set; 4096 rows fill the chip 4 x over
    gpr = torch.Generator(device=dev).manual_seed(5)
    prx = [torch.rand(rows_pr, N, device=dev, generator=gpr) for _ in range(2)]
    pry = [torch.rand(rows_pr, N, device=dev, generator=gpr) for _ in range(2)]

    def per_row(i):
        x2, y2 = two[i % 2]
        nat.forward_rows(x2[:rows_pr], y2[:rows_pr], prx[i % 2], pry[i % 2], 2.0, cutflags, None)

    srx = [torch.sort(t_, dim=1).values for t_ in prx]   # the same grids already in ascending order per row: the kernel's sortedness test
    sry = [torch.sort(t_, dim=1).values for t_ in pry]   # passes and the sort is skipped (per-row positions without the sort)

    def per_row_sorted(i):
        x2, y2 = two[i % 2]
        nat.forward_rows(x2[:rows_pr], y2[:rows_pr], srx[i % 2], sry[i % 2], 2.0, cutflags, None)

    with torch.no_grad():
        out[f"b{B}n{N}_unsorted_shared_forward"] = entry(timed(unsorted_shared, n), forward_kernel_name(N, "cutoff", batch=B) + " (gathers through the plan's permutation)",
                                                         B * (8 * N + 4), l3_resident=True, note="position plan (sort of the shared grid) made once, outside the timed loop")
        out[f"b{rows_pr}n{N}_per_row_positions_forward"] = entry(timed(per_row, n), "sot_rowpos_sort_kernel<32, true, true> (round 6: one wavefront per row, packed-word wave sort, permutations into the workspace) + sot_forward_kernel<ROWPOS> gathering through them",
                                                                 rows_pr * (16 * N + 4), l3_resident=True, rows=rows_pr)
        out[f"b{rows_pr}n{N}_per_row_sorted_positions_forward"] = entry(timed(per_row_sorted, n), "sot_forward_kernel<ROWPOS> (rows already sorted: sortedness test only)",
                                                                        rows_pr * (16 * N + 4), l3_resident=True, rows=rows_pr)

    # (0d) THE REFERENCE'S OWN OP SEQUENCE ON THIS GPU: losses.py:129-313 is ~25 ATen calls and device-agnostic, so a user of the
    #      reference on an MI355X runs exactly this composition (the package's torch-op route, sot_amd/_torch_path.py: the same ops in the
    #      same order; it is product code for CPU / float64 tensors, not the oracle).  Same inputs, same GPU, HIP events around a few
    #      calls: the figure the HIP kernels are to be compared with on this hardware, next to the CPU baseline.
    from sot_amd import _torch_path as tpath

    def torch_ops(mode, rows, xpos, ypos, grad=False):
        kw = MODES[mode]
        args = dict(p=kw.get("p", 1), square_dist=kw.get("square_dist", False), dont_normalize=kw.get("dont_normalize", False),
                    limit_quantile_range=kw.get("limit_quantile_range", False), require_sort=True, hinge_on=False)

        def call(i):
            x2, y2 = two[i % 2]
            x2, y2 = x2[:rows], y2[:rows]
            if not grad:
                return tpath.module_forward(x2, y2, xpos[i % 2] if isinstance(xpos, list) else xpos, ypos[i % 2] if isinstance(ypos, list) else ypos, **args)
            yv = y2.detach().requires_grad_(True)
            tpath.module_forward(x2, yv, xpos, ypos, **args).backward()
        return call

    # (0c') the segmented sort on its own (sot_segmented_sort = torch.sort(keys, 1) of losses.py:287-288: values + int64 indices, stable) and the
    #       gradients w.r.t. per-row positions (sot_w1d_position_grad: one deterministic kernel; no reference call site asks for them)
    one_pg = torch.ones(1, device=dev)
    with torch.no_grad():
        out[f"b{rows_pr}n{N}_segmented_sort"] = entry(timed(lambda i: nat.segmented_sort(prx[i % 2]), n), "sot_segmented_sort_wave_kernel<32, true> (round 6: one wavefront per row, packed 32-bit words, run repair; merge-sort fallback)",
                                                      rows_pr * 16 * N, l3_resident=True, rows=rows_pr, note="4 B in, 4 + 8 B out per key")
        out[f"b{rows_pr}n{N}_per_row_position_gradients_resorting"] = entry(timed(lambda i: nat.position_grads(two[i % 2][0][:rows_pr], two[i % 2][1][:rows_pr], prx[i % 2], pry[i % 2], 2.0, cutflags, one_pg), n),
                                                                            "sot_rowpos_sort_kernel + sot_position_grad_kernel<256, 8, true> called on its own (pre-sort into the workspace, then gather + CDFs + walk + tails)", rows_pr * (24 * N + 4), l3_resident=True, rows=rows_pr)
        # round 5: a training step sorts each row's supports ONCE -- the forward leaves the permutations ([B, n + m] uint16), the backward and
        # position-gradient kernels gather through them (what the module's autograd node does)
        perms = [nat.row_permutations(two[j][0][:rows_pr], two[j][1][:rows_pr], prx[j], pry[j], cutflags) for j in range(2)]
        out[f"b{rows_pr}n{N}_per_row_positions_forward_storing_permutations"] = entry(
            timed(lambda i: nat.forward_rows(two[i % 2][0][:rows_pr], two[i % 2][1][:rows_pr], prx[i % 2], pry[i % 2], 2.0, cutflags, None, perm_out=perms[i % 2]), n),
            "sot_rowpos_sort_kernel (permutations into the caller's image) + sot_forward_kernel<ROWPOS> gathering", rows_pr * (18 * N + 4), l3_resident=True, rows=rows_pr)
        out[f"b{rows_pr}n{N}_per_row_backward"] = entry(
            timed(lambda i: nat.backward_rows(two[i % 2][0][:rows_pr], two[i % 2][1][:rows_pr], prx[i % 2], pry[i % 2], 2.0, cutflags, one_pg, need_gx=False, perm_in=perms[i % 2]), n),
            "sot_backward_kernel<ROWPOS> gathering through the forward's permutations (no sort), d/dy", rows_pr * (22 * N + 4), l3_resident=True, rows=rows_pr)
        out[f"b{rows_pr}n{N}_per_row_backward_resorting"] = entry(
            timed(lambda i: nat.backward_rows(two[i % 2][0][:rows_pr], two[i % 2][1][:rows_pr], prx[i % 2], pry[i % 2], 2.0, cutflags, one_pg, need_gx=False), n),
            "sot_rowpos_sort_kernel + sot_backward_kernel<ROWPOS> called on its own (pre-sort into the workspace again)", rows_pr * (20 * N + 4), l3_resident=True, rows=rows_pr)
        out[f"b{rows_pr}n{N}_per_row_position_gradients"] = entry(
            timed(lambda i: nat.position_grads(two[i % 2][0][:rows_pr], two[i % 2][1][:rows_pr], prx[i % 2], pry[i % 2], 2.0, cutflags, one_pg, perm_in=perms[i % 2]), n),
            "sot_position_grad_kernel<256, 8, true> gathering through the forward's permutations (no sort)", rows_pr * (26 * N + 4), l3_resident=True, rows=rows_pr)
        del perms
    ref = {}
    with torch.no_grad():
        ref["p1_forward_ms"] = timed(torch_ops("p1", B, pos_x, pos_y), 6)
        ref["paper_mode_forward_ms"] = timed(torch_ops("cutoff", B, pos_x, pos_y), 6)
        ref[f"per_row_positions_{rows_pr}_rows_forward_ms"] = timed(torch_ops("cutoff", rows_pr, prx, pry), 6)
    ref["paper_mode_forward_backward_ms"] = timed(torch_ops("cutoff", B, pos_x, pos_y, grad=True), 4)
    ref["what"] = ("the reference's ATen op sequence (losses.py:129-313 via sot_amd/_torch_path.py) on the same GPU and inputs, B = %d rows "
                   "x %d bins; compare: value's ms_per_step (p = 1), extras.b%dn%d_cutoff_forward, _cutoff_module_forward_backward, "
                   "b%dn%d_per_row_positions_forward" % (B, N, B, N, rows_pr, N))
    out["reference_ops_on_this_gpu"] = ref
    del prx, pry, srx, sry, per_row, per_row_sorted
    torch.cuda.empty_cache()

    # (1) the headline shape in the paper's mode (p = 2, square_dist, dont_normalize, limit_quantile_range)
    cut = sot_entries(f"b{B}n{N}", B, N, sets, pos_x, pos_y, l3=False if len(sets) * 2 * B * N * 4 > 2**28 else True)
    ys = [s_[1].clone().requires_grad_(True) for s_ in sets[:2]]

    def autograd_step(i):   # the module through autograd: what a training loop calls
        yv = ys[i % 2]
        yv.grad = None
        cut(sets[i % 2][0], yv, x_pos=pos_x, y_pos=pos_y).backward()

    out[f"b{B}n{N}_cutoff_module_forward_backward"] = entry(timed(autograd_step, n), "autograd: loss_and_grad + scale", B * (12 * N + 4))
    del ys

    # (1b) the paper's own STEP: 64 clips x 16 frames = 1024 rows x 1025 bins through the module and autograd, launched from Python
    #      without graph capture (trainer.py:199-228) -- the kernels need ~10 us, so this entry measures the host path of the drop-in
    #      module; `host_us_per_call` is wall time per call over a long back-to-back run (the GPU stays ahead of the host), and
    #      `autograd_floor_us` the same loop around an autograd.Function that launches NOTHING (apply + loss.backward() through
    #      PyTorch's engine for a CUDA node): what no implementation behind torch.autograd can go below on this host.
    pf1 = spectra.unit_frequencies(2048, 16000.0, dev)
    pf1b = pf1.clone()
    gs = torch.Generator(device=dev).manual_seed(11)
    xs1 = torch.rand(1024, 1025, device=dev, generator=gs)
    ys1 = [torch.rand(1024, 1025, device=dev, generator=gs).requires_grad_(True) for _ in range(2)]

    def paper_step(i):
        yv = ys1[i % 2]
        yv.grad = None
        cut(xs1, yv, x_pos=pf1, y_pos=pf1b).backward()

    def wall_us(fn, count):
        for i in range(20):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(count):
            fn(i)
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        return 1e6 * host / count

    class _Nothing(torch.autograd.Function):   # no kernel: the forward hands out a preallocated scalar, the backward a fresh (uninitialised) gradient
        @staticmethod
        def forward(ctx, v, out):
            ctx.shape = v.shape
            return out.view_as(out)

        @staticmethod
        def backward(ctx, g):
            return torch.empty(ctx.shape, device=g.device), None

    zero_out = torch.zeros((), device=dev)

    def floor_step(i):
        yv = ys1[i % 2]
        yv.grad = None
        _Nothing.apply(yv, zero_out).backward()

    e = entry(timed(paper_step, n), "autograd: loss_and_grad (sot_backward_full_kernel<128, 9, 2, ..., 1025, false, true, 4> + mean) + scale",
              1024 * (12 * 1025 + 4), l3_resident=True)
    e["host_us_per_call"] = wall_us(paper_step, 400)
    e["autograd_floor_us"] = wall_us(floor_step, 400)
    out["b1024n1025_cutoff_module_forward_backward"] = e
    def paper_step_fresh_positions(i):   # trainer.py:187-197 verbatim: x_pos rebuilt and y_pos = x_pos.clone() on EVERY step -> a new position plan per step
        yv = ys1[i % 2]
        yv.grad = None
        xp_ = pf1 / 1.0
        cut(xs1, yv, x_pos=xp_, y_pos=xp_.clone()).backward()

    e2 = entry(timed(paper_step_fresh_positions, n), "the same + two elementwise torch kernels + sot_prepare_positions per step", 1024 * (12 * 1025 + 4), l3_resident=True)
    e2["host_us_per_call"] = wall_us(paper_step_fresh_positions, 400)
    out["b1024n1025_cutoff_module_forward_backward_fresh_positions"] = e2
    with torch.no_grad():
        out["b1024n1025_cutoff_module_forward"] = entry(timed(lambda i: cut(xs1, ys1[0], x_pos=pf1, y_pos=pf1b), n),
                                                         forward_kernel_name(1025, "cutoff", batch=1024) + " + batch mean", 1024 * (8 * 1025 + 4), l3_resident=True)
        out["b1024n1025_cutoff_module_forward"]["host_us_per_call"] = wall_us(lambda i: cut(xs1, ys1[0], x_pos=pf1, y_pos=pf1b), 400)
        # the entry above is two launches per call issued from Python: with ~10 us of host time per call against ~12 us of GPU time it reads the
        # host on a slower or busier box (round 4: 19.9 us on the driver's box, 12.4 on the builder's).  The same call replayed from a HIP graph
        # is the GPU-bound figure:
        try:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    cut(xs1, ys1[0], x_pos=pf1, y_pos=pf1b)
            torch.cuda.current_stream().wait_stream(side)
            fgraph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(fgraph):
                cut(xs1, ys1[0], x_pos=pf1, y_pos=pf1b)
            out["b1024n1025_cutoff_module_forward"]["graph_replay_us"] = 1e3 * timed(lambda i: fgraph.replay(), n)
        except Exception as exc:  # noqa: BLE001
            out["b1024n1025_cutoff_module_forward"]["graph_replay_us"] = repr(exc)[:200]
    # (1c) the same step captured ONCE by the user in a HIP graph and replayed (INTEGRATION.md "HIP-graph recipe"): eager is pinned at
    #      PyTorch's autograd floor for ~10 us of kernels, so the GPU-bound figure and how to get it; with persistent position tensors and with
    #      positions rebuilt inside the captured step (trainer.py:187-197: the plan launch is then part of the graph)
    def user_graph(fresh):
        ystat = ys1[0].detach().clone().requires_grad_(True)
        side = torch.cuda.Stream(device=dev)

        def step():
            if fresh:
                xp_ = pf1 / 1.0
                return cut(xs1, ystat, x_pos=xp_, y_pos=xp_.clone())
            return cut(xs1, ystat, x_pos=pf1, y_pos=pf1b)

        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                ystat.grad = None
                step().backward()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        ystat.grad = None
        with torch.cuda.graph(graph):
            static_loss = step()
            static_loss.backward()
        graph.replay()
        torch.cuda.synchronize()
        ycheck = ystat.detach().clone().requires_grad_(True)
        want = cut(xs1, ycheck, x_pos=pf1, y_pos=pf1b)
        want.backward()
        same = bool(torch.equal(want.detach(), static_loss.detach()) and torch.equal(ycheck.grad, ystat.grad))
        e = entry(timed(lambda i: graph.replay(), n), "torch.cuda.graph around `loss = mod(x, y, x_pos=, y_pos=); loss.backward()`: loss_and_grad kernel + mean + scale"
                  + (" + the caller's two position kernels + sot_prepare_positions" if fresh else ""), 1024 * (12 * 1025 + 4), l3_resident=True,
                  equals_eager=same)
        e["host_us_per_call"] = wall_us(lambda i: graph.replay(), 400)
        return e

    for key, fresh in (("b1024n1025_cutoff_step_user_graph", False), ("b1024n1025_cutoff_step_user_graph_fresh_positions", True)):
        try:
            out[key] = user_graph(fresh)
        except Exception as exc:  # noqa: BLE001
            out[key] = {"error": repr(exc)[:300]}
    del xs1, ys1

    # (2) the paper's own row shape: one-sided spectra of n_fft 2048 (1025 bins), 16384 rows, rfftfreq / max positions
    g = torch.Generator(device=dev).manual_seed(7)
    pf = spectra.unit_frequencies(2048, 16000.0, dev)
    pairs = [(torch.rand(16384, 1025, device=dev, generator=g), torch.rand(16384, 1025, device=dev, generator=g)) for _ in range(2)]
    sot_entries("b16384n1025", 16384, 1025, pairs, pf, pf.clone(), l3=True)
    del pairs

    # (3) BASELINE config 4: 8192 x 512 peaky rows with a per-row amplitude cutoff, masked-dense and CSR forms
    rs = ragged_supports(8192, 512, 1234)
    xm, ym = (t.to(dev) for t in rs["dense"])
    (xw, xp_, xo), (yw, yp_, yo) = [tuple(t.to(dev) for t in side) for side in rs["csr"]]
    p512 = rs["pos"].to(dev)
    p512b = p512.clone()
    plan512 = nat.PositionPlan(p512, p512b)
    kw = dict(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True)
    flags = 15
    dense_bytes = 8192 * (8 * 512 + 4)
    csr_bytes = 8 * (xw.numel() + yw.numel()) + 16 * (8192 + 1) + 4 * 8192
    with torch.no_grad():
        out["config4_b8192n512_masked_dense_forward"] = entry(
            timed(lambda i: nat.forward_rows(xm, ym, p512, p512b, 2.0, flags, plan512), n), forward_kernel_name(512, "cutoff", batch=8192), dense_bytes,
            l3_resident=True, mean_kept_support=rs["kept"])
        out["config4_b8192n512_csr_forward"] = entry(
            timed(lambda i: wasserstein_1d_csr(xw, xp_, xo, yw, yp_, yo, rs["max_n"], rs["max_m"], **kw), n), "sot_forward_kernel<CSR>",
            csr_bytes, l3_resident=True, mean_kept_support=rs["kept"], retired=True,
            note="NOT a product path: the CSR form left the public surface in round 4 (DESIGN.md §8); timed only so the decision stays checkable")
    del xm, ym, xw, xp_, yw, yp_

    # (4) BASELINE config 5: 256 harmonic clips -> STFT x2 (n_fft 2048, hop 256, flattop; 16 frames) -> SOT paper mode
    #     forward + backward into the estimate's audio (4096 rows x 1025 bins)
    gen = torch.Generator(device=dev).manual_seed(0)
    target = spectra.harmonic_batch(256, generator=gen, device=dev)
    estimates = [spectra.harmonic_batch(256, generator=gen, device=dev).requires_grad_(True) for _ in range(2)]
    mod5 = Wasserstein1D(**MODES["cutoff"]).to(dev)

    seed5 = torch.ones((), device=dev)   # the gradient seed loss.backward() would otherwise create with a fill kernel per step (4 us of GPU time)

    def train_step(i):
        e = estimates[i % 2]
        e.grad = None
        spectra.training_step_slice(mod5, target, e).backward(seed5)

    ms5 = timed(train_step, n)
    # bytes the slice must move: both clips' audio in, the estimate's audio gradient out (spectra stay on chip in the ideal)
    out["config5_train_step_256clips"] = entry(ms5, "stft_mag_forward_pair (+ the estimate's complex spectrum) + sot_backward_full_kernel<128, 9, 2, ..., 1025, false, true, 4> + mean + stft_mag_backward_spec + overlap-add",
                                               3 * 256 * 4096 * 4, steps_per_s=1e3 / ms5, rows=4096, bins=1025)

    # (5) the synthesiser in front of it: 256 clips x 16 frames x 8 partials of frame-rate controls -> 4096
    #     samples (sot_synth_forward / _backward: no sample-rate array in HBM), alone and with the config-5 slice behind it
    amp_frames = torch.rand(256, 16, 8, device=dev, generator=gen).requires_grad_(True)
    f0_frames = (40 + 1900 * torch.rand(256, 16, 1, device=dev, generator=gen)).requires_grad_(True)
    ctl_bytes = 4 * (256 * 16 * 9) * 2 + 4 * 256 * 4096 * 2      # controls in, their gradients out, audio out and its gradient in
    with torch.no_grad():
        ms_sf = timed(lambda i: spectra.sinusoidal_synth(amp_frames, f0_frames, 4096, 16000, harmonic=True), n)
    out["synth_forward_256clips"] = entry(ms_sf, "oscillator_tile_kernel<0, true> + scan + oscillator_tile_kernel<1, true>", 4 * 256 * (16 * 9 + 4096))
    grad_audio = torch.randn(256, 4096, device=dev, generator=gen)

    def synth_step(i):
        amp_frames.grad = f0_frames.grad = None
        spectra.sinusoidal_synth(amp_frames, f0_frames, 4096, 16000, harmonic=True).backward(grad_audio)

    ms_sb = timed(synth_step, n)
    out["synth_forward_backward_256clips"] = entry(ms_sb, "synth forward + tap tables + oscillator_tile_kernel<3, true> + scan + frames reduce", ctl_bytes)

    def synth_train_step(i):
        amp_frames.grad = f0_frames.grad = None
        audio = spectra.sinusoidal_synth(amp_frames, f0_frames, 4096, 16000, harmonic=True)
        spectra.training_step_slice(mod5, target, audio).backward(seed5)

    ms_st = timed(synth_train_step, n)
    out["config5_train_step_with_synth_256clips"] = entry(ms_st, "synth + stft pair + sot training form + stft backward + synth backward", ctl_bytes,
                                                          steps_per_s=1e3 / ms_st)

    # (6) the multi-kernel steps above are launched from Python one kernel at a time: on a loaded host they measure the host.  The same
    #     steps replayed from ONE HIP graph (what a training loop that captures its step does) show the GPU time.
    def replayed(step_fn):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step_fn(0)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step_fn(0)
        return timed(lambda i: graph.replay(), n)

    for key, fn, kern, nbytes in (("config5_train_step_256clips", train_step, "the same kernels, one HIP graph", 3 * 256 * 4096 * 4),
                                  ("synth_forward_backward_256clips", synth_step, "the same kernels, one HIP graph", ctl_bytes),
                                  ("config5_train_step_with_synth_256clips", synth_train_step, "the same kernels, one HIP graph", ctl_bytes)):
        try:
            out[key + "_graph_replay"] = entry(replayed(fn), kern, nbytes)
        except Exception as exc:  # noqa: BLE001 -- a capture that fails must not take the bench line with it
            out[key + "_graph_replay"] = {"error": repr(exc)[:200]}
    out.update(rccl_world1_probe())
    return out


def paper_loss_workloads(dev, nat, timed, n):
    """The loss block a user of the reference actually runs per step (trainer.py:183-245 with the paper's YAML,
    paper-experiments/SOT-2048/*/train_config.yaml:73-102): fresh x_pos / y_pos, two TorchSTFT transforms (n_fft 2048, hop 256, flattop),
    MixOfLosses([MSSLoss(6 scales, L1, mag_weight 1), Wasserstein1D(paper kwargs)], [0.05, 1]), sum of the means, backward() into x_hat --
    at the paper's batch (64 clips of 4096 samples) and at config 5's (256), eager and replayed from one HIP graph; next to it MSSLoss
    alone, the SOT slice alone, and the reference's own op sequence (torch.stft / ATen ops) on the same GPU and inputs."""
    from sot_amd import spectra
    from sot_amd import _torch_path as tpath
    from sot_amd.losses import MixOfLosses, MSSLoss, Wasserstein1D
    out = {}
    sizes = (2048, 1024, 512, 256, 128, 64)
    mss = MSSLoss(fft_sizes=sizes, loss_type="L1", mag_weight=1, logmag_weight=0).to(dev)
    sot = Wasserstein1D(**MODES["cutoff"], require_sort=True).to(dev)
    mix = MixOfLosses([mss, sot], [0.05, 1]).to(dev)
    freqs_dev = torch.fft.rfftfreq(2048, d=1.0 / 16000.0).to(dev)
    seed = torch.ones((), device=dev)

    def replayed(step_fn):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step_fn(0)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step_fn(0)
        return timed(lambda i: graph.replay(), n)

    def torch_mss(t_audio, v_audio):   # losses.py:365-425 on torch ops (torch.stft = rocFFT)
        loss = 0.0
        for size in sizes:
            hop = int(size * 0.25)
            t = spectra.stft_magnitude_torch(t_audio, size, hop, None)
            v = spectra.stft_magnitude_torch(v_audio, size, hop, None)
            loss = loss + torch.mean(torch.abs(t - v))
        return loss

    def torch_step(x, e, pos):     # the same block on the reference's ops: torch.stft + losses.py:129-313 as ATen calls
        x_pos = pos / pos.max()
        y_pos = x_pos.clone()
        sx = spectra.stft_magnitude_torch(x, 2048, 256, "flattop")
        sy = spectra.stft_magnitude_torch(e, 2048, 256, "flattop")
        w = tpath.module_forward(sx, sy, x_pos, y_pos, p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True,
                                 require_sort=True, hinge_on=False)
        return (torch_mss(x, e) * 0.05).mean() + (w * 1).mean()

    for clips in (64, 256):
        gen = torch.Generator(device=dev).manual_seed(1000 + clips)
        x = spectra.harmonic_batch(clips, generator=gen, device=dev)
        hats = [spectra.harmonic_batch(clips, generator=gen, device=dev).requires_grad_(True) for _ in range(2)]
        io_bytes = 3 * clips * 4096 * 4   # both clips' audio in, the estimate's gradient out: what the block must move

        def full_step(i, fresh_host_positions=True, fused=None):   # fused=None: what a caller of trainer_loss_step gets (the one-node form)
            e = hats[i % 2]
            e.grad = None
            spectra.trainer_loss_step(mix, x, e, 2048, 256, "flattop", 16000.0, positions=None if fresh_host_positions else freqs_dev,
                                      fused=fused).backward(seed)

        def mss_step(i):
            e = hats[i % 2]
            e.grad = None
            mss(x, e).backward(seed)

        def sot_step(i):
            e = hats[i % 2]
            e.grad = None
            spectra.training_step_slice(sot, x, e).backward(seed)

        def ref_step(i):
            e = hats[i % 2]
            e.grad = None
            torch_step(x, e, freqs_dev).backward(seed)

        def ref_mss_step(i):
            e = hats[i % 2]
            e.grad = None
            torch_mss(x, e).backward(seed)

        def entry(ms, what, **kw):
            return {"ms": ms, "what": what, "algorithmic_bytes": io_bytes, "frac": io_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "clips": clips, **kw}

        tag = f"{clips}clips"
        out[f"paper_loss_step_{tag}"] = entry(timed(full_step, n), "trainer.py:183-245 as spectra.trainer_loss_step runs it by default (positions=None: the transform's bin frequencies, kept on the device after the first call): the mix of MSSLoss and Wasserstein1D as ONE host call / autograd node (round 6; loss and gradient bit-identical to the module-by-module composition), eager, launched from Python")
        out[f"paper_loss_step_{tag}_device_positions"] = entry(timed(lambda i: full_step(i, False), n), "the same with the caller's own device tensor of bin frequencies (positions=...)")
        out[f"paper_loss_step_{tag}_module_by_module"] = entry(timed(lambda i: full_step(i, False, False), n), "the same step composed module by module as the reference's trainer does (fused=False: rounds 4-5's form), device positions, eager")
        out[f"mssloss_forward_backward_{tag}"] = entry(timed(mss_step, n), "MSSLoss(6 scales, L1, mag_weight 1) forward + backward into the estimate, eager")
        out[f"sot_slice_forward_backward_{tag}"] = entry(timed(sot_step, n), "STFT pair + Wasserstein1D (paper mode) forward + backward, eager (= config 5's slice)")
        for key, fn in ((f"paper_loss_step_{tag}", lambda i: full_step(i, False)), (f"paper_loss_step_{tag}_module_by_module", lambda i: full_step(i, False, False)),
                        (f"mssloss_forward_backward_{tag}", mss_step),
                        (f"sot_slice_forward_backward_{tag}", sot_step)):
            try:
                out[key + "_graph_replay"] = entry(replayed(fn), "the same kernels replayed from ONE HIP graph (GPU time of the block)")
            except Exception as exc:  # noqa: BLE001
                out[key + "_graph_replay"] = {"error": repr(exc)[:200]}
        try:
            out[f"paper_loss_step_{tag}_reference_ops"] = entry(timed(ref_step, max(3, n // 5)), "the reference's op sequence on this GPU: torch.stft (rocFFT) x 14 + ATen ops of losses.py, eager")
            out[f"mssloss_forward_backward_{tag}_reference_ops"] = entry(timed(ref_mss_step, max(3, n // 5)), "MSSLoss on torch ops (torch.stft x 12 + abs / mean), eager")
        except Exception as exc:  # noqa: BLE001
            out[f"paper_loss_step_{tag}_reference_ops"] = {"error": repr(exc)[:200]}
        del x, hats
    return out


def rccl_world1_probe():
    """The N > 1 step (local kernels -> ONE RCCL all-reduce of the fp64 partial sum, two alternating streams) run by ONE rank in a
    fresh child process tree (python -m torch.distributed.run, SOT_BENCH_FORCE_DIST=1): the code path the 8-GPU run takes, exercised
    on every bench run so that it never runs unattended for the first time.  Child processes are the permitted way to start a second
    GPU program from one that has initialised the GPU (no exec)."""
    import socket
    import subprocess
    try:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ, SOT_BENCH_FORCE_DIST="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "8")
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        for k in list(env):   # a profiler around this bench (rocprofv3 preloads its tool library) must not follow into the child tree
            if k == "LD_PRELOAD" or k.startswith(("ROCP_", "ROCPROF", "ROCPROFILER_", "HSA_TOOLS_")):
                env.pop(k)
        cmd = launcher_command(1, ["--gpus", "1", "--steps", "200", "--warmup", "20", "--prewarm", "200", "--full", "--no-extras", "--no-cpu-baseline"], port)
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            return {"rccl_world1": {"error": f"rc={r.returncode}: " + (r.stderr or "")[-300:]}}
        rec = json.loads(line[-1])
        return {"rccl_world1_ms_per_step": rec["ms_per_step"], "rccl_world1": {"collective": rec["config"]["collective"], "streams": rec["config"]["streams"],
                "ms_per_step_without_collective": rec["extras"].get("ms_per_step_without_collective"),
                "host_enqueue_ms_per_step": rec["extras"].get("host_enqueue_ms_per_step"), "loss_set0": rec["config"]["loss_set0"]}}
    except Exception as exc:  # noqa: BLE001 -- a probe must not take the bench line with it
        return {"rccl_world1": {"error": repr(exc)[:300]}}


def cpu_baseline(mode, n, rows, seed, budget_s=25.0):
    """The reference's CPU PyTorch path (op-for-op restatement) on this host's cores, bounded sample.
    ATen's intra-op scaling on this problem saturates well below a big host's core count, so a few thread
    counts are tried (within `budget_s`) and the best is reported with the count actually used.  The SAME inputs as the GPU's set 0
    (seed 1234, all `rows` rows of the workload when the budget allows: `rows_timed`); a `paper_mode` sibling times the paper's own
    mode (p = 2, square_dist, dont_normalize, limit_quantile_range) on the same rows at the best thread count, and `per_row_scaling`
    gives the time of half the rows relative to all of them (0.5 = linear in the row count)."""
    from oracle import torch_restatement as tr   # the ONLY use of oracle/ in this file: the timed CPU baseline
    from sot_amd.bench_inputs import spectrum_pairs
    ncpu = os.cpu_count() or 1
    x, y = spectrum_pairs("uniform", rows, n, n, seed)
    pos = torch.linspace(0, 1, n)

    def kwargs_of(m):
        c = MODES[m]
        return dict(p=c.get("p", 1), square_dist=c.get("square_dist", False), dont_normalize=c.get("dont_normalize", False),
                    limit_quantile_range=c.get("limit_quantile_range", False))

    def best_of(xr, yr, kw, threads, calls=2):
        torch.set_num_threads(threads)
        best, val = float("inf"), 0.0
        with torch.no_grad():
            tr.sot_loss(xr, yr, pos, pos.clone(), **kw)  # warm-up
            for _ in range(calls):
                t0 = time.perf_counter()
                val = tr.sot_loss(xr, yr, pos, pos.clone(), **kw)
                best = min(best, time.perf_counter() - t0)
        return best, float(val)

    kw = kwargs_of(mode)
    best, best_threads, val, tried = float("inf"), 1, 0.0, []
    t_end = time.perf_counter() + budget_s
    for threads in sorted({min(ncpu, t) for t in (8, 16, 32, 64, ncpu)}):
        if time.perf_counter() > t_end:
            break
        dt, v = best_of(x, y, kw, threads)
        if dt < best:
            best, best_threads, val = dt, threads, v
        tried.append(threads)
    rec = {"value": rows / best, "unit": f"rows/s ({rows}-row sample)", "cores": best_threads, "kind": "port", "rows_timed": rows,
           "sample": f"{rows} rows x N={n}, mode {mode}: best call of oracle/torch_restatement.sot_loss over thread counts "
                     f"{tried} on a {ncpu}-cpu host (torch {torch.__version__} CPU)", "scalar": float(val)}
    try:
        half = max(1, rows // 2)
        dt_half, _ = best_of(x[:half], y[:half], kw, best_threads)
        rec["per_row_scaling"] = {"rows": half, "seconds": dt_half, "relative_to_all_rows": dt_half / best}
        if mode != "cutoff":
            dt_p, v_p = best_of(x, y, kwargs_of("cutoff"), best_threads)
            rec["paper_mode"] = {"value": rows / dt_p, "unit": f"rows/s ({rows}-row sample)", "cores": best_threads, "rows_timed": rows,
                                 "mode": MODES["cutoff"], "scalar": v_p}
    except Exception as exc:  # noqa: BLE001 -- the siblings must not take the baseline with them
        rec["paper_mode"] = {"error": repr(exc)[:200]}
    return rec


# Launches of the timed region whose dominant kernel is timed: the library attaches a HIP start / stop event pair to the kernel
# dispatch itself (sot_profile_next_launch -> hipExtLaunchKernelGGL: what rocprofv3's kernel trace measures; an event pair
# recorded on the stream AROUND the call adds 2-3 us of stream time to a 30 us kernel and delays the step).  The library keeps
# 64 such pairs, so every max(4, ceil(K / 64))-th step of the timed region is timed.
PROFILE_SLOTS = 64


def flatten_for_scalar_readers(rec, B, N):
    """Scalar copies of the nested figures (round-5 review: the driver's record of this line keeps scalars of `config`, `roofline`,
    `cpu_baseline` and of the top level, and drops nested objects -- so the pipeline north_star names, the paper's step at the paper's
    batch and the per-row path never reached it).  Same numbers as the nested entries, nothing new is measured here; a figure that was
    not measured in this run (N > 1, --no-extras, another row length) is None."""
    roof, ext = rec["roofline"], rec.get("extras", {})

    def ms_of(key):
        e = ext.get(key)
        return e.get("ms") if isinstance(e, dict) else None

    for key in ("paper_mode", "merge_p1", "training_form"):
        side = roof.get(key) if isinstance(roof.get(key), dict) else {}
        roof[f"{key}_kernel_ms"] = side.get("kernel_ms")
        roof[f"{key}_frac"] = side.get("frac")
        roof[f"{key}_stream_ms_per_call"] = side.get("stream_ms_per_call")
    rows_pr = min(B, 4096)
    flat = {
        "paper_step_64clips_graph_ms": ms_of("paper_loss_step_64clips_graph_replay"),
        "paper_step_64clips_eager_ms": ms_of("paper_loss_step_64clips"),
        "paper_step_256clips_graph_ms": ms_of("paper_loss_step_256clips_graph_replay"),
        "paper_step_64clips_module_by_module_graph_ms": ms_of("paper_loss_step_64clips_module_by_module_graph_replay"),
        "mss_64clips_graph_ms": ms_of("mssloss_forward_backward_64clips_graph_replay"),
        "mss_256clips_graph_ms": ms_of("mssloss_forward_backward_256clips_graph_replay"),
        "sot_slice_64clips_graph_ms": ms_of("sot_slice_forward_backward_64clips_graph_replay"),
        "per_row_forward_ms": ms_of(f"b{rows_pr}n{N}_per_row_positions_forward"),
        "per_row_backward_ms": ms_of(f"b{rows_pr}n{N}_per_row_backward"),
        "per_row_sorted_rows_forward_ms": ms_of(f"b{rows_pr}n{N}_per_row_sorted_positions_forward"),
        "per_row_position_grad_ms": ms_of(f"b{rows_pr}n{N}_per_row_position_gradients"),
        "segmented_sort_ms": ms_of(f"b{rows_pr}n{N}_segmented_sort"),
        "module_step_1024x1025_user_graph_ms": ms_of("b1024n1025_cutoff_step_user_graph"),
        "rccl_world1_ms_per_step": ext.get("rccl_world1_ms_per_step"),
    }
    rec.update(flat)
    roof.update({k: v for k, v in flat.items() if k != "rccl_world1_ms_per_step"})   # a second copy inside an object the reader keeps
    cb = rec.get("cpu_baseline")
    if isinstance(cb, dict):
        pm = cb.get("paper_mode") if isinstance(cb.get("paper_mode"), dict) else {}
        cb["paper_mode_rows_per_s"] = pm.get("value")
        cb["paper_mode_scalar"] = pm.get("scalar")


DUMP_LIMIT_BYTES = 64 * 2**20


def write_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: every array as out_dir/<name>.npy in float32 / float64.  When the arrays together exceed `limit`, every 1-D
    array larger than its share is cut to a fixed, seeded sample of its elements (the same indices in every run of the same shape)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.array(v, dtype=np.float64 if v.dtype == np.float64 else np.float32, order="C") for k, v in arrays.items()}   # 0-d stays 0-d
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > limit and a.ndim == 1 and a.nbytes > limit // len(arrays):
            keep = (limit // len(arrays)) // a.itemsize
            a = a[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def event_stride(steps):
    # never more than every 4th step: a timed dispatch is preceded / followed by its event packets (+ ~8 us when EVERY step is timed)
    return int(os.environ.get("SOT_BENCH_EVENT_STRIDE", str(max(4, -(-steps // PROFILE_SLOTS)))))


def main():
    args = parse()
    if args.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if args.steps < 1:
        sys.exit("bench.py: --steps must be >= 1")
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(launch_ranks(args, sys.argv[1:]))
    # stdout carries exactly ONE line (rank 0's JSON): native libraries print there too (RCCL's version banner at
    # communicator creation), so file descriptor 1 is pointed at stderr for the run and the line goes to the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        sys.stderr.write(f"bench.py: WORLD_SIZE={world} does not match --gpus {args.gpus}\n")
        sys.exit(4)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # SOT_BENCH_FORCE_DIST=1 exercises the RCCL branch even with one rank (used to test it on a 1-GPU box)
    dist_on = world > 1 or (os.environ.get("SOT_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))  # nccl == RCCL on ROCm
        ones = torch.ones(1, dtype=torch.float64, device=torch.device("cuda", local_rank))
        dist.all_reduce(ones)   # every rank contributes 1.0: the sum is the number of ranks RCCL connected (checked before anything is timed)
        rccl_seen = {"rccl_world_size": dist.get_world_size(), "rccl_allreduce_ones": float(ones)}
        assert rccl_seen["rccl_allreduce_ones"] == float(world), rccl_seen
    else:
        rccl_seen = {"rccl_world_size": 1, "rccl_allreduce_ones": None}   # no process group in a one-GPU run (extras.rccl_world1 exercises the path)
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP path has no CPU fallback)"
    dev = torch.device("cuda", local_rank if dist_on else 0)
    torch.cuda.set_device(dev)

    from sot_amd import _native as nat
    from sot_amd.losses import Wasserstein1D
    from sot_amd.bench_inputs import spectrum_pairs

    nat.load(build_if_missing=False)  # must be the prebuilt in-tree library
    B, N = args.rows, args.nfft
    mod = Wasserstein1D(**MODES[args.mode]).to(dev)
    pos_x = torch.linspace(0, 1, N, device=dev)
    pos_y = pos_x.clone()

    # set 0: the BASELINE recipe (CPU generator, seed 1234 + rank, x drawn before y); others: device RNG
    if args.scaling == "strong":   # config 3's global batch = blocks of 8192 rows seeded 1234 + block; this rank owns rows [rank B, rank B + B)
        x0, y0 = global_batch_rows(rank * B, B, N)
    else:
        x0, y0 = spectrum_pairs("uniform", B, N, N, 1234 + rank)
    sets = [(x0.to(dev), y0.to(dev))]
    g = torch.Generator(device=dev).manual_seed(99 + rank)
    for _ in range(args.sets - 1):
        sets.append((torch.rand(B, N, device=dev, generator=g), torch.rand(B, N, device=dev, generator=g)))

    # The rotating inputs are fixed tensors: their marshalled form (contiguous [B, N] views, flag word, position plan) is
    # computed once; a step then is exactly the FFI calls Wasserstein1D.forward makes (no GPU work is skipped).
    marshalled = [mod._marshal(x, y, pos_x, pos_y, {}) for x, y in sets]
    n_sets = len(sets)

    # Steps are independent.  With N > 1 (or --lanes 2) they are issued on TWO alternating HIP streams: one step's batch-mean
    # kernel and its RCCL all-reduce then overlap the next step's forward kernel instead of leaving the GPU idle for the
    # collective's latency (measured with one rank through RCCL in round 1: 61.7 us/step with everything on one stream, 44-47 us
    # like this).  All work, collectives included, completes inside the timed region (device-wide synchronize at its end).  On
    # one GPU the default is ONE stream: consecutive forward kernels then never share the GPU and rocprofv3's per-kernel
    # durations agree with the kernel-attached ones (with two streams a timed kernel may share the GPU with the other stream's).
    graph_mode = bool(args.graph_steps)   # --graph-steps: single stream, the whole step replayed from a HIP graph (opt-in)
    n_lanes = args.lanes if args.lanes else (2 if dist_on else 1)
    if graph_mode:
        n_lanes = 1
    EVENT_STRIDE = event_stride(args.steps)
    default_stream = torch.cuda.current_stream()
    lanes = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    ring = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(4)]   # local / global fp64 sums (N > 1)
    rowbuf = [torch.empty(B, dtype=torch.float32, device=dev) for _ in range(4)]  # row losses; slot i % 4 stays on one lane
    meanbuf = [torch.empty((), dtype=torch.float32, device=dev) for _ in range(4)]
    inv_global_rows = 1.0 / float(world * B)   # weak scaling: every rank owns exactly B rows

    # The step's native call with its arguments marshalled once per (input set, output slot) pair (nat.prepared_loss_call): the timed
    # loop then enters the C function directly -- the same call Wasserstein1D.forward makes (sot_w1d_loss: row kernel + fixed-order
    # reduction), minus the per-call struct fill.  With N > 1 this keeps the host (issuing kernel, reduction and all-reduce for
    # every step) ahead of the GPU: 36 us of host time per step before, against 33 us of kernel time.
    prepared = {}

    def native_step(i, slot):
        key = (i % len(sets), slot)
        call = prepared.get(key)
        if call is None:
            x2, y2, xp, yp, flags, plan, _ = marshalled[key[0]]
            call = prepared[key] = nat.prepared_loss_call(x2, y2, xp, yp, float(mod.p), flags, plan, rowbuf[slot], meanbuf[slot],
                                                          sum_out=ring[slot] if dist_on else None)
        return call()

    def step(i, profile=None):
        with torch.no_grad():
            slot = i % len(ring)
            if n_lanes != 1:
                torch.cuda.set_stream(lanes[i & 1])
            if profile is not None:
                nat.profile_next_launch(profile)   # start / stop events attached to the next row-kernel dispatch
            if not dist_on:
                # the FFI call Wasserstein1D.forward makes (sot_w1d_loss: the row kernel, then the fixed-order mean kernel), into
                # preallocated outputs
                return native_step(i, slot)
            # N > 1: local kernels (one FFI crossing: row kernel + fixed-order reduction, the fp64 partial sum into ring[slot]) -> ONE
            # all-reduce(SUM) of that sum over RCCL -> global mean
            native_step(i, slot)
            dist.all_reduce(ring[slot], op=dist.ReduceOp.SUM)   # in place: the slot then holds the global sum
            return ring[slot]   # the mean is ring[slot] * inv_global_rows (applied where the value is read)

    def enter_lanes():
        for ln in lanes:
            ln.wait_stream(default_stream)

    def leave_lanes():
        torch.cuda.synchronize()
        torch.cuda.set_stream(default_stream)

    def barrier():
        if dist_on:
            import torch.distributed as dist
            dist.barrier()

    enter_lanes()
    for i in range(args.prewarm + args.warmup):
        # the first launches also create the library's timing event pairs (one per slot), outside the timed region
        out = step(i, i if i < PROFILE_SLOTS else None)
    for sl in range(min(args.prewarm + args.warmup, PROFILE_SLOTS), PROFILE_SLOTS):
        step(sl, sl)   # a short warm-up did not reach every slot: no event pair is created inside the timed region
    first_t = step(0)  # parity value on set 0 (global mean when N > 1)
    torch.cuda.synchronize()  # every stream
    first = float(first_t) * (inv_global_rows if dist_on else 1.0)
    timed_slots = []

    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graphs = None
    if args.graph_steps:  # one captured step per rotating input set, replayed in the same order
        graphs = []
        for k in range(len(sets)):
            gph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gph):
                out = step(k)
            graphs.append(gph)
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
    for i in range(args.steps):
        if graphs is not None:
            graphs[i % len(graphs)].replay()
        else:
            if i % EVENT_STRIDE == 0 and len(timed_slots) < PROFILE_SLOTS:
                timed_slots.append(len(timed_slots))
                out = step(i, timed_slots[-1])
            else:
                out = step(i)
    host_enqueue = time.perf_counter() - t0   # when the host is done issuing work (diagnostic: is the loop host-bound?)
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist_on:
        import torch.distributed as dist
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt)
    del out
    if args.dump_outputs and rank == 0:
        # the buffers the last timed step wrote (slot of step K - 1; a replayed graph holds the slot of the step it captured), copied
        # before anything else reuses them
        last = args.steps - 1
        slot = (last % len(graphs) if graphs is not None else last) % len(ring)
        dump = {"loss": (ring[slot] * inv_global_rows) if dist_on else meanbuf[slot], "row_losses": rowbuf[slot]}
        write_outputs(args.dump_outputs, {k: v.detach().cpu().numpy() for k, v in dump.items()})
    leave_lanes()  # back to the default stream for the secondary measurements

    if graphs is not None and args.full:  # a replay carries no kernel-attached events: time the dominant kernel eagerly after the timed region
        timed_slots = list(range(min(args.steps, 50)))
        for i in timed_slots:
            step(i, i)
        torch.cuda.synchronize()
    kern_ms = sum(nat.profile_elapsed_ms(sl) for sl in timed_slots) / len(timed_slots) if timed_slots else None

    def attached_ms(call, count=32):
        """Average duration of the FIRST kernel `call(i)` launches (a compile-time-length row kernel), from HIP events attached to
        the dispatch: the figure rocprofv3's kernel trace reports for it."""
        for i in range(400):   # the first launches of a kernel run slower (code load, clock ramp): like the headline's 400 untimed steps (60 until round 6:
            call(i)            # the same kernels then read 5-30 % above their steady state on some boxes -- profiles/r6_same_box_ab.txt)
        slots = list(range(min(count, PROFILE_SLOTS)))
        for i in slots:
            nat.profile_next_launch(i)
            call(i)
        torch.cuda.synchronize()
        return sum(nat.profile_elapsed_ms(i) for i in slots) / len(slots)

    # The pipeline north_star names (merge of the two CDFs = sort + searchsorted) on the SAME workload, in the paper's mode, and the
    # training form (loss + d/dy in one pass): kernel-attached times and their roofline fractions next to the headline kernel's.
    side = {}
    if args.full and not dist_on and FULL_ROW_GEOMETRY.get(N) is not None:
        cutm = Wasserstein1D(**MODES["cutoff"]).to(dev)
        cm = [cutm._marshal(x, y, pos_x, pos_y, {}) for x, y in sets]

        def paper_forward(i):
            x2, y2, xp, yp, flags, plan, _ = cm[i % len(cm)]
            nat.forward_rows(x2, y2, xp, yp, 2.0, flags, plan, rowbuf[i % 4])

        def merge_p1_forward(i):
            x2, y2, xp, yp, flags, plan, _ = marshalled[i % len(marshalled)]
            nat.forward_rows(x2, y2, xp, yp, 1.0, flags | nat.FLAG_NO_AREA, plan, rowbuf[i % 4])

        def training_form(i):
            x2, y2, xp, yp, flags, plan, _ = cm[i % len(cm)]
            nat.loss_and_grad(x2, y2, xp, yp, 2.0, flags, plan)

        with torch.no_grad():
            for key, call, kern, nbytes in (
                    ("paper_mode", paper_forward, forward_kernel_name(N, "cutoff", batch=B), B * (8 * N + 4)),
                    ("merge_p1", merge_p1_forward, forward_kernel_name(N, "p1", same_grid=False, batch=B), B * (8 * N + 4)),
                    ("training_form", training_form, forward_kernel_name(N, "cutoff", backward=True, batch=B), B * (12 * N + 4))):
                try:
                    ms = attached_ms(call)
                    side[key] = {"kernel": kern, "kernel_ms": ms, "algorithmic_bytes_per_launch": nbytes,
                                 "achieved": nbytes / (ms * 1e-3) / 1e9, "frac": nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
                    # the same launches back to back between two stream events (per launch: the kernel + its launch gap, plus the
                    # batch-mean kernel for the training form): a dispatch with attached events ends with a system-scope release,
                    # which for the training form (64 MB of gradients) flushes what a following kernel would not wait for
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for i in range(100):
                        call(i)
                    e1.record()
                    torch.cuda.synchronize()
                    side[key]["stream_ms_per_call"] = e0.elapsed_time(e1) / 100
                except Exception as exc:  # noqa: BLE001
                    side[key] = {"error": repr(exc)[:200]}
        del cm

    def timed(fn, n):  # secondary measurements (outside the contract's timed region), HIP events on the launch stream
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    extras = {"host_enqueue_ms_per_step": 1e3 * host_enqueue / args.steps, "kernel_timing": f"kernel-attached HIP events on {len(timed_slots)} "
              f"launches of the timed region (every {EVENT_STRIDE}th step)"}
    if args.full and not dist_on and n_lanes == 1 and not graph_mode:
        # the same steps pipelined over two HIP streams (what --lanes 2 times, and what N > 1 does to hide the collective): a step's
        # launch gap, pipeline fill / drain and mean kernel then overlap its neighbour's row kernel.  Not the default on one GPU:
        # overlapped kernels share the chip, so their individual durations (kernel_ms, rocprofv3) stop describing the kernel.
        k2 = max(40, min(args.steps, 200))
        torch.cuda.synchronize()
        for ln in lanes:
            ln.wait_stream(default_stream)
        t2 = time.perf_counter()
        with torch.no_grad():
            for i in range(k2):
                x2, y2, xp, yp, flags, plan, _ = marshalled[i % len(marshalled)]
                with torch.cuda.stream(lanes[i & 1]):
                    nat.reduce_mean(nat.forward_rows(x2, y2, xp, yp, float(mod.p), flags, plan, rowbuf[i % 4]))
        torch.cuda.synchronize()
        extras["two_streams_ms_per_step"] = 1e3 * (time.perf_counter() - t2) / k2
        extras["two_streams_rows_per_s"] = B / (extras["two_streams_ms_per_step"] * 1e-3)
    if args.full:
        with torch.no_grad():   # the same kernel between two events recorded on the stream around the call (round 1's method)
            x2, y2, xp, yp, flags, plan, _ = marshalled[0]
            pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
            for k, (ea, eb) in enumerate(pairs):
                x2, y2, xp, yp, flags, plan, _ = marshalled[k % len(marshalled)]
                ea.record()
                nat.forward_rows(x2, y2, xp, yp, float(mod.p), flags, plan, rowbuf[0])
                eb.record()
                nat.reduce_mean(rowbuf[0])
            torch.cuda.synchronize()
            extras["kernel_ms_between_stream_events"] = sum(ea.elapsed_time(eb) for ea, eb in pairs) / len(pairs)
    n_extra = max(10, min(args.steps, 50))
    if args.full and dist_on:  # BASELINE config 3: report the step with and without the collective
        def local_only(i):
            with torch.no_grad():
                x2, y2, xp, yp, flags, plan, _ = marshalled[i % len(sets)]
                nat.reduce_mean(nat.forward_rows(x2, y2, xp, yp, float(mod.p), flags, plan, rowbuf[i % 4]), sum_out=ring[i % len(ring)])
        extras["ms_per_step_without_collective"] = timed(local_only, n_extra)
    elif args.full and not args.no_extras:
        del sets[4:], marshalled[4:]   # four rotating sets (512 MiB) still exceed the Infinity Cache
        extras.update(other_workloads(dev, nat, sets, pos_x, pos_y, timed, n_extra))
        extras.update(paper_loss_workloads(dev, nat, timed, n_extra))
    bytes_per_row = 4 * (N + N) + 4  # fwd, shared positions
    achieved = bytes_per_row * B / (kern_ms * 1e-3) / 1e9 if kern_ms else None

    if rank == 0:
        parity = None
        try:
            man = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))
            if args.full and (B, N) == (8192, 2048) and world == 1:  # the stored scalar is that of seed 1234 alone
                want = man["_config2_b8192n2048_seed1234"][f"uniform_{args.mode}"]
                parity = abs(first - want) / abs(want)
        except Exception:
            parity = None
        traffic, traffic_source = None, None
        try:  # HBM bytes per launch of THIS kernel on THIS workload from the committed rocprofv3 PMC passes (profiles/), if present
            import glob
            for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json")), reverse=True):
                pj = json.load(open(path))
                if pj.get("workload") == f"B={B},N={N},{args.mode}" and pj.get("kernel") == forward_kernel_name(N, args.mode, batch=B):
                    traffic = pj["hbm_bytes_per_launch"]
                    traffic_source = (f"{os.path.relpath(path, ROOT)}: rocprofv3 --pmc passes (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE) of this "
                                      "command in an earlier run, committed; NOT measured in this run")
                    break
        except Exception:
            traffic = None
        for key in ("paper_mode", "training_form"):   # the same committed PMC passes hold these kernels' traffic
            try:
                import glob
                for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_hbm_traffic_{key}.json")), reverse=True):
                    pj = json.load(open(path))
                    if key in side and pj.get("kernel") == side[key].get("kernel") and pj.get("workload", "").startswith(f"B={B},N={N},"):
                        side[key]["traffic"] = pj["hbm_bytes_per_launch"]
                        side[key]["traffic_source"] = f"{os.path.relpath(path, ROOT)} (committed PMC passes; not measured in this run)"
                        break
            except Exception:
                pass
        rec = {
            "metric": "sot_loss_evals_per_sec", "value": world * B * args.steps / elapsed, "unit": "rows/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"SOT-2048 config: B={B} rows/GPU x N_fft={N} fp32 spectrum pairs, forward, mode {args.mode} "
                                   f"({json.dumps(MODES[args.mode])}), shared linspace positions, {n_sets} rotating input sets "
                                   f"({n_sets * 2 * B * N * 4 / 2**20:.0f} MiB > 256 MiB L3)",
                       "rows_per_gpu": B, "n_fft": N, "mode": args.mode, "prewarm_steps": args.prewarm, "global_rows": world * B,
                       "streams": n_lanes,
                       "collective": "none" if not dist_on else "one RCCL all-reduce(SUM) of the fp64 partial sum per step" + (" (HIP-graph replay)" if args.graph_steps else ""),
                       "parity_rel_err_vs_reference_scalar": parity, "loss_set0": first, **rccl_seen},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS if achieved is not None else None, "traffic": traffic, "traffic_source": traffic_source,
                         "kernel": forward_kernel_name(N, args.mode, batch=B), "kernel_ms": kern_ms, "algorithmic_bytes_per_launch": bytes_per_row * B,
                         "headline_is": ("merge-free p=1 kernel (both measures on one sorted grid: no sort, no search, no merge); the merge pipeline "
                                         "north_star describes: see roofline.merge_p1 / roofline.paper_mode / roofline.training_form")
                                        if (args.mode == "p1") else "merge pipeline (sort/cumsum/merge-path search/walk)",
                         **side},
            "extras": extras,
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            rec["cpu_baseline"] = cpu_baseline(args.mode, N, min(args.cpu_rows, B), 1234)
        flatten_for_scalar_readers(rec, B, N)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(rec) + "\n").encode())
    barrier()
    if dist_on:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
