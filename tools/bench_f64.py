"""float64 rows, timed on the GPU: what the float64 kernels (sot_w1d_forward_f64 / sot_w1d_backward_f64 behind Wasserstein1D) cost next to the
route such tensors took before them -- the torch-op composition (_torch_path.py) on the same float64 GPU tensors -- and, as context, next
to the float32 HIP call on the same values.

Two shapes (8192 x 2048, 1024 x 1025), two modes (p = 1; the paper's mode: p = 2, square_dist, dont_normalize, limit_quantile_range), two
calls (the forward; forward + backward w.r.t. y).  Per cell three routes, all through the public module, in ONE process, alternating within
every round:
    composition   the module with losses.F64_ROUTE = False (the torch-op composition on float64 GPU tensors: the route before the kernels)
    f64           the module on the float64 kernels
    f32           the float32 module on x.float(), y.float() (context: what float32 costs on the same values)
Stream time: device events around blocks of back-to-back calls, `--warmup` calls discarded, `--calls` calls timed in `--rounds` blocks per
route.  The paper's mode runs on the recipe rows of tests/f64_cases.py (order-insensitive under the cutoff), p = 1 on generic rows; the
values of the three routes are compared first.  Per cell the f64 route's share of the HBM peak is reported on 16 (n + m) + 8 bytes per row
(forward: the two float64 rows and the row loss; shared positions stay in LDS) and 24 (n + m) + 8 ... per row for forward + backward w.r.t. y
(the rows twice, one gradient row).

    python tools/bench_f64.py [--calls 500] [--warmup 50] [--rounds 10] [--out profiles/f64_rows.json]   -> one JSON line
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12    # bytes / s, MI355X
SHAPES = ((8192, 2048), (1024, 1025))
MODES = (("p1", dict(p=1)), ("paper", dict(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True)))


def block_us(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_f64.py measures on the GPU"
    import f64_cases as fc
    from sot_amd import losses
    from sot_amd._native import load
    load(build_if_missing=False)
    dev = torch.device("cuda:0")
    per_block = max(1, args.calls // args.rounds)
    result = {"device": torch.cuda.get_device_name(0), "calls": per_block * args.rounds, "warmup": args.warmup, "rounds": args.rounds,
              "unit": "us per call (device events)", "hbm_peak_bytes_per_s": HBM_PEAK, "cells": {}}
    for B, n in SHAPES:
        for mode_name, kw in MODES:
            if "limit_quantile_range" in kw:
                x, y = fc.cutoff_rows(B, n, n, True, seed=1)
            else:
                x, y = fc.plain_rows(B, n, n, seed=1)
            x64, y64 = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
            pos64 = torch.linspace(0, 1, n, dtype=torch.float64, device=dev)
            x32, y32, pos32 = x64.float(), y64.float(), pos64.float()
            mod = losses.Wasserstein1D(**kw).to(dev)

            def run(route, backward):
                xa, ya, pa = (x32, y32, pos32) if route == "f32" else (x64, y64, pos64)
                losses.F64_ROUTE = route != "composition"
                if not backward:
                    with torch.no_grad():
                        return mod(xa, ya, x_pos=pa, y_pos=pa)
                yg = ya.detach().requires_grad_(True)
                out = mod(xa, yg, x_pos=pa, y_pos=pa)
                out.backward()
                return out.detach(), yg.grad

            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")   # the composition says once that it is not the HIP path
                values = {r: run(r, True) for r in ("composition", "f64", "f32")}
            torch.cuda.synchronize()
            v_c, v_k, v_s = (float(values[r][0]) for r in ("composition", "f64", "f32"))
            g_c, g_k = values["composition"][1], values["f64"][1]
            cell = {"value_composition": v_c, "value_f64": v_k, "value_f32": v_s,
                    "value_rel_diff_f64_vs_composition": abs(v_k - v_c) / abs(v_c),
                    "grad_max_diff_f64_vs_composition": float((g_k - g_c).abs().max()), "grad_max": float(g_c.abs().max())}
            for call, backward in (("forward", False), ("forward_backward_y", True)):
                routes = ("composition", "f64", "f32")
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    for r in routes:
                        block_us(lambda: run(r, backward), args.warmup)
                    total = dict.fromkeys(routes, 0.0)
                    for _ in range(args.rounds):
                        for r in routes:
                            total[r] += block_us(lambda: run(r, backward), per_block)
                us = {r: total[r] / (per_block * args.rounds) for r in routes}
                nbytes = B * ((24 if backward else 16) * 2 * n + 8)
                cell[call] = {"composition_us": us["composition"], "f64_us": us["f64"], "f32_us": us["f32"],
                              "speedup_over_composition": us["composition"] / us["f64"], "f64_over_f32": us["f64"] / us["f32"],
                              "f64_bytes": nbytes, "f64_share_of_hbm_peak": nbytes / (us["f64"] * 1e-6) / HBM_PEAK}
            losses.F64_ROUTE = True
            result["cells"][f"b{B}n{n}_{mode_name}"] = cell
            del x64, y64, x32, y32, values, g_c, g_k
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
