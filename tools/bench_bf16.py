"""bfloat16 spectra, timed on the GPU: what the typed forward (sot_w1d_loss_bf16 / sot_w1d_forward_bf16: 16-bit row loads in the kernel) costs
next to the float32 call and next to what a bfloat16 caller had to do before it -- x.float(), y.float(), then the float32 call.

Three shapes (8192 x 2048 p = 1 forward + mean, the headline; 8192 x 2048 paper-mode forward; 8192 x 512 p = 1 forward + mean), per shape:
    a         the float32 call on float32 inputs
    a_parent  the same call into ANOTHER build of the library (--parent-lib: the parent commit's libsot_hip.so), same process, same buffers
    b         x16.float(), y16.float() (two torch kernels, two temporaries from the caching allocator), then a on them
    c         the typed call on the bfloat16 inputs
All in one process, alternating within every round, device events around `--iters` back-to-back calls, the warm-up round discarded.
Every variant walks round robin over `sets` distinct input sets, enough of them that also the bfloat16 copies exceed the 256 MiB L3 one and
a half times (as bench.py's rotating sets do for float32): rows come from HBM in every variant.  `--sets 1` keeps one L3-resident set.  The
calls are the C entry points themselves on preallocated outputs with a position plan (one ctypes call per iteration, as bench.py's timed
loop), so the figures are stream time per call: kernel(s) plus launch gaps, no Python marshalling.  Outputs are compared first: c must
equal a on the upcast inputs bit for bit, a_parent must equal a.

    python tools/bench_bf16.py [--parent-lib PATH] [--iters 2000] [--rounds 7] [--out profiles/bf16_forward.json]   -> one JSON line
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

RS, SAME = 8, 64
PAPER = 1 | 2 | 4 | 8
SHAPES = (("b8192n2048_p1_forward_mean", 8192, 2048, 1.0, RS, True),
          ("b8192n2048_paper_forward", 8192, 2048, 2.0, PAPER, False),
          ("b8192n512_p1_forward_mean", 8192, 512, 1.0, RS, True))


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
    ap.add_argument("--parent-lib", default=None, help="libsot_hip.so of the parent commit (row a_parent)")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sets", type=int, default=0, help="input sets per shape (0: as many as put 384 MiB of bfloat16 rows in rotation, at least 6)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bf16.py measures on the GPU"
    from sot_amd import _native as nat
    lib = nat.load(build_if_missing=False)
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("sot_w1d_loss", "sot_w1d_forward"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = nat.EXPORTS[name]
        parent.sot_abi_version.restype = ctypes.c_int
    dev = torch.device("cuda:0")
    idx = 0
    raw = torch._C._cuda_getCurrentRawStream
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "unit": "us per call (device events)",
              "parent_lib_abi": parent.sot_abi_version() if parent is not None else None, "shapes": {}}
    for tag, B, n, p, flags, with_mean in SHAPES:
        g = torch.Generator(device=dev).manual_seed(5)
        sets = args.sets or max(6, -(-(384 << 20) // (B * 4 * n)))
        x16s = [torch.rand(B, n, generator=g, device=dev).to(torch.bfloat16) for _ in range(sets)]
        y16s = [torch.rand(B, n, generator=g, device=dev).to(torch.bfloat16) for _ in range(sets)]
        x32s, y32s = [t.float() for t in x16s], [t.float() for t in y16s]            # the same values in both types
        pos = torch.linspace(0, 1, n, device=dev)
        plan = nat.PositionPlan(pos, pos)
        rows = {k: torch.empty(B, device=dev) for k in "abcp"}
        mean = {k: torch.empty((), device=dev) for k in "abcp"}

        def call(handle, typed, xs, ys, key):
            pr = nat.make_problem(xs, ys, pos, pos, p, flags, plan)
            ref = ctypes.byref(pr)
            fn = getattr(handle, ("sot_w1d_loss" if with_mean else "sot_w1d_forward") + ("_bf16" if typed else ""))
            r, m = rows[key].data_ptr(), mean[key].data_ptr()
            keep = (pr, xs, ys)

            def go():
                rc = fn(ref, r, float(B), 0, 0.0, m, None, None, None, 0, raw(idx)) if with_mean else fn(ref, r, None, 0, raw(idx))
                assert rc == 0, (rc, keep[0].n)
            return go

        def rotating(calls):
            state = [0]

            def go():
                calls[state[0] % sets]()
                state[0] += 1
            go.reset = lambda: state.__setitem__(0, 0)
            return go

        def widen_then_call(x16, y16):
            def go():
                xf, yf = x16.float(), y16.float()
                call(lib, False, xf, yf, "b")()
            return go

        a = rotating([call(lib, False, x32s[k], y32s[k], "a") for k in range(sets)])
        c = rotating([call(lib, True, x16s[k], y16s[k], "c") for k in range(sets)])
        a_parent = rotating([call(parent, False, x32s[k], y32s[k], "p") for k in range(sets)]) if parent is not None else None
        b = rotating([widen_then_call(x16s[k], y16s[k]) for k in range(sets)])

        variants = {"a_float32": a, "b_float_then_float32": b, "c_typed_bf16": c}
        if a_parent is not None:
            variants["a_parent_float32"] = a_parent
        for fn in variants.values():      # set 0 through every variant: the outputs must be the same bits
            fn()
        torch.cuda.synchronize()
        same = {"c_equals_a_bits": bool(torch.equal(rows["c"], rows["a"]) and (not with_mean or torch.equal(mean["c"], mean["a"]))),
                "b_equals_a_bits": bool(torch.equal(rows["b"], rows["a"])),
                "a_parent_equals_a_bits": bool(torch.equal(rows["p"], rows["a"])) if a_parent is not None else None}
        assert same["c_equals_a_bits"] and same["b_equals_a_bits"] and same["a_parent_equals_a_bits"] in (True, None), same
        times = {k: [] for k in variants}
        for rnd in range(args.rounds + 1):
            for k, fn in variants.items():
                t = timed(fn, args.iters)
                if rnd > 0:                                  # round 0 is the warm-up
                    times[k].append(t)
        entry = {"rows": B, "bins": n, "p": p, "flags": flags, "with_mean": with_mean, "bits": same, "input_sets": sets,
                 "rotating_bytes_float32": sets * B * 8 * n, "rotating_bytes_bf16": sets * B * 4 * n,
                 "bytes_float32": B * (8 * n + 4), "bytes_bf16": B * (4 * n + 4)}
        for k, v in times.items():
            entry[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v), "rounds_us": v}
        entry["c_below_b_by_us"] = entry["b_float_then_float32"]["median_us"] - entry["c_typed_bf16"]["median_us"]
        entry["gate_c_below_b_by_more_than_spread_of_b"] = entry["c_below_b_by_us"] > entry["b_float_then_float32"]["spread_us"]
        entry["c_over_a"] = entry["c_typed_bf16"]["median_us"] / entry["a_float32"]["median_us"]
        result["shapes"][tag] = entry
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
