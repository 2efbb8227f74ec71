"""Mixed supports (a dense spectrum on the shared STFT bin grid against K partials with per-row frequencies), timed on the GPU: the native
route (sot_w1d_mixed_*) next to the materialising route (losses.MIXED_ROUTE = False: the grid expanded to [B, n], both sides down the
per-row route) in ONE process, alternating rounds, device events on the stream around `--iters` calls after a warm-up.  Two workloads per
shape and mode: the forward (batch mean, no gradient) and forward + backward with gradients for the partials' amplitudes AND frequencies.
`forward` / `forward_backward` are CALL times, eager from Python -- everything a user's call enqueues, host marshalling included where
the device waits for it; `*_graph` are the same calls captured into a HIP graph and replayed: the GPU time of the block without the
host.  Neither is a kernel time.  Outputs of the two routes are compared on the timed inputs before anything is timed.

    python tools/bench_mixed.py [--iters 50] [--rounds 7] [--out profiles/f7_mixed_supports.json]      -> one JSON line (and the file)
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4096, 1025, 8), (4096, 1025, 64), (16384, 257, 8))   # rows, grid bins n, partials K
MODES = {"p1": dict(p=1), "paper": dict(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True)}


def row_bytes(n, K):
    """HBM bytes per row from the shapes alone.  Native: weights of both sides, the K positions, the loss.  Materialising: weights and
    positions at 4 bytes per point on both sides, the expanded grid row written and read back, the uint16 sort permutations written and
    read back."""
    return {"native": 4 * n + 8 * K + 4, "materialising": 8 * (n + K) + 8 * n + 4 * (n + K) + 4}


def inputs(B, n, K, dev):
    gen = torch.Generator(device=dev).manual_seed(17)
    x = torch.rand(B, n, device=dev, generator=gen)
    grid = torch.linspace(0, 1, n, device=dev)
    amps = torch.rand(B, K, device=dev, generator=gen)
    f0 = 0.004 + 0.03 * torch.rand(B, 1, device=dev, generator=gen)
    freqs = f0 * torch.arange(1, K + 1, device=dev)            # harmonic partials; the highest of K = 64 pass Nyquist (1.0)
    return x, grid, amps, freqs.contiguous()


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / iters      # us per call


def graph_of(fn, dev):
    """`fn` captured into a graph on a side stream after a warm-up there (the pattern of tests/test_mixed_supports_gpu.py)"""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def compare(run_new, run_old, rounds, iters):
    t_new, t_old = [], []
    for _ in range(rounds):
        t_new.append(timed(run_new, iters))
        t_old.append(timed(run_old, iters))
    return {"native": statistics.median(t_new), "native_rounds": t_new, "materialising": statistics.median(t_old), "materialising_rounds": t_old,
            "speedup": statistics.median(t_old) / statistics.median(t_new), "faster_beyond_spread": max(t_new) < min(t_old)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixed.py measures on the GPU"
    from sot_amd import losses
    dev = torch.device("cuda:0")
    result = {"iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "unit": "us, device events around `iters` calls / replays; medians over alternating rounds", "cases": {}}

    class route:
        def __init__(self, native):
            self.native = native

        def __enter__(self):
            losses.MIXED_ROUTE = self.native

        def __exit__(self, *exc):
            losses.MIXED_ROUTE = True

    for (B, n, K), (mode, ctor) in ((s, m) for s in SHAPES for m in MODES.items()):
        mod = losses.Wasserstein1D(**ctor).to(dev)
        x, grid, amps, freqs = inputs(B, n, K, dev)
        ya, yf = amps.clone().requires_grad_(True), freqs.clone().requires_grad_(True)

        def forward():
            with torch.no_grad():
                return mod(x, amps, x_pos=grid, y_pos=freqs)

        def train():
            ya.grad = yf.grad = None
            loss = mod(x, ya, x_pos=grid, y_pos=yf)
            loss.backward()
            return loss.detach()

        # the two routes on the timed inputs: loss, amplitude and frequency gradients
        outs = {}
        for native in (True, False):
            with route(native):
                f = forward()
                t = train()
                outs[native] = (f.clone(), t.clone(), ya.grad.clone(), yf.grad.clone())
        torch.cuda.synchronize()
        scale = lambda t: float(t.abs().max()) + 1e-30   # noqa: E731
        agree = {name: float((a - b).abs().max()) / scale(b) for name, a, b in zip(("forward", "loss", "grad_amplitudes", "grad_frequencies"), outs[True], outs[False])}

        case = {"rows": B, "n": n, "K": K, "mode": mode, "bytes_per_row": row_bytes(n, K), "max_difference_over_max_magnitude": agree}
        for name, fn in (("forward", forward), ("forward_backward", train)):
            for native in (True, False):      # warm-up of both
                with route(native):
                    for _ in range(10):
                        fn()
            torch.cuda.synchronize()

            def eager(native, fn=fn):
                def run():
                    with route(native):
                        fn()
                return run
            case[name] = {"unit": "us per call, eager", **compare(eager(True), eager(False), args.rounds, args.iters)}
            graphs = {}
            for native in (True, False):
                with route(native):
                    graphs[native] = graph_of(fn, dev)
            torch.cuda.synchronize()
            case[name + "_graph"] = {"unit": "us per replay of the captured call", **compare(graphs[True].replay, graphs[False].replay, args.rounds, args.iters)}
            del graphs
        result["cases"][f"{B}x{n}_K{K}_{mode}"] = case
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
