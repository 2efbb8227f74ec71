"""bfloat16 training, timed on the GPU: what the typed backward and training form (sot_w1d_backward_bf16 / sot_w1d_loss_and_grad_bf16: 16-bit
row loads and 16-bit gradient stores in the kernel) cost next to the float32 calls and next to what a bfloat16 caller had to do before them.

Two shapes (8192 x 2048, 8192 x 512) x two modes (paper mode; p = 1) x two forms (the y-only training form: row losses, mean and grad_y;
the both-gradient backward under per-row cotangents), per case:
    a   the float32 call on float32 rows, float32 gradients
    b   two sot_rows_bf16_to_f32, the float32 call on the images, sot_rows_f32_to_bf16 per gradient -- a bfloat16 caller without the typed call
    c   the typed call on the bfloat16 rows, bfloat16 gradients
All in one process, alternating within every round, device events around `--iters` back-to-back calls, the warm-up round discarded.  Every
variant walks round robin over `sets` distinct input sets, enough of them that also the bfloat16 copies exceed the 256 MiB L3 one and a half
times: rows come from HBM in every variant.  The calls are the C entry points themselves on preallocated buffers with a position plan (ctypes
calls only), so the figures are stream time per call: kernel(s) plus launch gaps.  Outputs are compared first: c and b must equal a's
gradients rounded to nearest even, bit for bit, and a's losses.

    python tools/bench_bf16_train.py [--iters 1000] [--rounds 7] [--out profiles/bf16_training.json]   -> one JSON line
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RS = 8
PAPER = 1 | 2 | 4 | 8
BF16 = torch.bfloat16
CASES = [(f"b8192n{n}_{mode}_{form}", 8192, n, p, flags, form) for n in (2048, 512) for mode, p, flags in (("paper", 2.0, PAPER), ("p1", 1.0, RS))
         for form in ("training_form", "backward_both")]


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sets", type=int, default=0, help="input sets per case (0: as many as put 384 MiB of bfloat16 rows in rotation, at least 6)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bf16_train.py measures on the GPU"
    from sot_amd import _native as nat
    lib = nat.load(build_if_missing=False)
    dev = torch.device("cuda:0")
    idx = 0
    raw = torch._C._cuda_getCurrentRawStream
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "unit": "us per call (device events)", "cases": {}}
    for tag, B, n, p, flags, form in CASES:
        both = form == "backward_both"
        g = torch.Generator(device=dev).manual_seed(5)
        sets = args.sets or max(6, -(-(384 << 20) // (B * 4 * n)))
        x16s = [torch.rand(B, n, generator=g, device=dev).to(BF16) for _ in range(sets)]
        y16s = [torch.rand(B, n, generator=g, device=dev).to(BF16) for _ in range(sets)]
        x32s, y32s = [t.float() for t in x16s], [t.float() for t in y16s]            # the same values in both types
        pos = torch.linspace(0, 1, n, device=dev)
        plan = nat.PositionPlan(pos, pos)
        cot = torch.rand(B, generator=g, device=dev) + 0.25
        rows = {k: torch.empty(B, device=dev) for k in "abc"}
        mean = {k: torch.empty((), device=dev) for k in "abc"}
        gx32 = {k: torch.empty(B, n, device=dev) for k in "ab"}
        gy32 = {k: torch.empty(B, n, device=dev) for k in "ab"}
        gx16 = {k: torch.empty(B, n, dtype=BF16, device=dev) for k in "bc"}
        gy16 = {k: torch.empty(B, n, dtype=BF16, device=dev) for k in "bc"}
        xw, yw = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)        # b's float32 images

        def f32_call(xs, ys, key):
            pr = nat.make_problem(xs, ys, pos, pos, p, flags, plan)
            ref, keep = ctypes.byref(pr), (pr, xs, ys)
            r, m, gx, gy, c = rows[key].data_ptr(), mean[key].data_ptr(), gx32[key].data_ptr(), gy32[key].data_ptr(), cot.data_ptr()

            def go():
                if both:
                    rc = lib.sot_w1d_backward(ref, c, 1, 1.0, gx, gy, None, 0, raw(idx))
                else:
                    rc = lib.sot_w1d_loss_and_grad(ref, r, float(B), m, None, 1.0 / B, gy, None, None, 0, raw(idx))
                assert rc == 0, (rc, keep[0].n)
            return go

        def typed_call(xs, ys):
            pr = nat.make_problem(xs, ys, pos, pos, p, flags, plan)
            assert lib.sot_w1d_bf16_native(ctypes.byref(pr)) == 1
            ref, keep = ctypes.byref(pr), (pr, xs, ys)
            r, m, gx, gy, c = rows["c"].data_ptr(), mean["c"].data_ptr(), gx16["c"].data_ptr(), gy16["c"].data_ptr(), cot.data_ptr()

            def go():
                if both:
                    rc = lib.sot_w1d_backward_bf16(ref, c, 1, 1.0, gx, gy, None, None, 0, raw(idx))
                else:
                    rc = lib.sot_w1d_loss_and_grad_bf16(ref, r, float(B), m, None, 1.0 / B, gy, None, None, 0, raw(idx))
                assert rc == 0, (rc, keep[0].n)
            return go

        def widen_call_narrow(x16, y16):
            inner = f32_call(xw, yw, "b")
            xs, ys, xd, yd = x16.data_ptr(), y16.data_ptr(), xw.data_ptr(), yw.data_ptr()
            gxs, gys, gxd, gyd = gx32["b"].data_ptr(), gy32["b"].data_ptr(), gx16["b"].data_ptr(), gy16["b"].data_ptr()

            def go():
                s = raw(idx)
                assert lib.sot_rows_bf16_to_f32(xs, B, n, n, xd, n, s) == 0 and lib.sot_rows_bf16_to_f32(ys, B, n, n, yd, n, s) == 0
                inner()
                if both:
                    assert lib.sot_rows_f32_to_bf16(gxs, B, n, n, gxd, n, s) == 0
                assert lib.sot_rows_f32_to_bf16(gys, B, n, n, gyd, n, s) == 0
            return go

        def rotating(calls):
            state = [0]

            def go():
                calls[state[0] % sets]()
                state[0] += 1
            return go

        variants = {"a_float32": rotating([f32_call(x32s[k], y32s[k], "a") for k in range(sets)]),
                    "b_widen_float32_narrow": rotating([widen_call_narrow(x16s[k], y16s[k]) for k in range(sets)]),
                    "c_typed_bf16": rotating([typed_call(x16s[k], y16s[k]) for k in range(sets)])}
        for fn in variants.values():      # set 0 through every variant: the outputs must be the same bits
            fn()
        torch.cuda.synchronize()
        want_gy, want_gx = gy32["a"].to(BF16), gx32["a"].to(BF16)
        same = {"c_grad_y_is_rne_of_a": bool(torch.equal(gy16["c"].view(torch.int16), want_gy.view(torch.int16))),
                "b_grad_y_is_rne_of_a": bool(torch.equal(gy16["b"].view(torch.int16), want_gy.view(torch.int16)))}
        if both:
            same["c_grad_x_is_rne_of_a"] = bool(torch.equal(gx16["c"].view(torch.int16), want_gx.view(torch.int16)))
        else:
            same["c_losses_equal_a_bits"] = bool(torch.equal(rows["c"], rows["a"]) and torch.equal(mean["c"], mean["a"]))
        assert all(same.values()), (tag, same)
        times = {k: [] for k in variants}
        for rnd in range(args.rounds + 1):
            for k, fn in variants.items():
                t = timed(fn, args.iters)
                if rnd > 0:                                  # round 0 is the warm-up
                    times[k].append(t)
        entry = {"rows": B, "bins": n, "p": p, "flags": flags, "form": form, "bits": same, "input_sets": sets,
                 "rotating_bytes_float32": sets * B * 8 * n, "rotating_bytes_bf16": sets * B * 4 * n}
        for k, v in times.items():
            entry[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v), "rounds_us": v}
        spread = max(entry[k]["spread_us"] for k in ("b_widen_float32_narrow", "c_typed_bf16"))
        entry["c_below_b_by_us"] = entry["b_widen_float32_narrow"]["median_us"] - entry["c_typed_bf16"]["median_us"]
        entry["gate_c_below_b_by_more_than_round_to_round_spread"] = entry["c_below_b_by_us"] > spread
        entry["c_over_a"] = entry["c_typed_bf16"]["median_us"] / entry["a_float32"]["median_us"]
        entry["narrowing_and_widening_us"] = entry["b_widen_float32_narrow"]["median_us"] - entry["a_float32"]["median_us"]
        result["cases"][tag] = entry
        del x16s, y16s, x32s, y32s
        torch.cuda.empty_cache()
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
