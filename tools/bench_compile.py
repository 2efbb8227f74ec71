"""Diagnostic (not part of bench.py): the paper's 64-clip loss step (4096 samples @ 16 kHz, STFT 2048 / 256 flattop,
MixOfLosses([MSSLoss six scales, Wasserstein1D p = 2 with cutoff], [0.05, 1]), backward into the estimate) as the reference trainer's
UNCHANGED module-by-module loop in three forms -- eager, torch.compile(mode="reduce-overhead"), a hand-captured HIP graph -- and the
one-node `trainer_loss_step` eager and under compile.  Host wall clock around `--steps` steps ending in a device synchronise, the forms
interleaved round by round in one process; prints one JSON line (median, min, max of the per-step microseconds over the rounds).

    python tools/bench_compile.py [--clips 64] [--steps 1000] [--rounds 7] [--forms a,b,...] [--package-root DIR] [--out FILE]

--package-root: import `sot_amd` from another checkout (e.g. the parent commit, for an eager-against-eager comparison in the same run)."""
import argparse
import json
import os
import statistics
import sys
import time

FORMS = ("eager_loop", "compiled_loop", "graph_loop", "eager_fused", "compiled_fused")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from sot_amd import spectra
    from sot_amd.losses import MixOfLosses, MSSLoss, Wasserstein1D

    assert torch.cuda.is_available(), "bench_compile.py measures on the GPU"
    dev = torch.device("cuda:0")
    forms = [f for f in args.forms.split(",") if f]
    assert all(f in FORMS for f in forms), forms
    mix = MixOfLosses([MSSLoss(fft_sizes=(2048, 1024, 512, 256, 128, 64), loss_type="L1", mag_weight=1, logmag_weight=0),
                       Wasserstein1D(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True, require_sort=True)], [0.05, 1]).to(dev)
    x = spectra.harmonic_batch(args.clips, seed=0, device=dev)
    x_hat = spectra.harmonic_batch(args.clips, seed=1, device=dev).requires_grad_(True)
    freqs = torch.fft.rfftfreq(2048, d=1.0 / 16000.0).to(dev)

    def loop(x, x_hat):   # trainer.py:192-236 as it stands: fresh positions, two transforms, each loss times its weight, sum of the means
        x_pos = freqs / freqs.max()
        y_pos = x_pos.clone()
        spec_x, spec_x_hat = spectra.stft_magnitude(x, 2048, 256), spectra.stft_magnitude(x_hat, 2048, 256)
        total = 0
        for loss_fn, weight in zip(mix.losses, mix.weights):
            a, b = (x, x_hat) if loss_fn.__class__.__name__ == "MSSLoss" else (spec_x, spec_x_hat)
            total = total + (loss_fn(a, b, x_pos=x_pos, y_pos=y_pos) * weight).mean()
        return total

    def fused(x, x_hat):
        return spectra.trainer_loss_step(mix, x, x_hat)

    def stepper(fn, mark=False):
        def step():
            x_hat.grad = None
            if mark:
                torch.compiler.cudagraph_mark_step_begin()
            fn(x, x_hat).backward()
        return step

    steppers, values, grad_of = {}, {}, {}
    for form in forms:
        if form == "eager_loop":
            steppers[form] = stepper(loop)
        elif form == "eager_fused":
            steppers[form] = stepper(fused)
        elif form in ("compiled_loop", "compiled_fused"):
            steppers[form] = stepper(torch.compile(loop if form == "compiled_loop" else fused, mode="reduce-overhead", fullgraph=True), mark=True)
        else:   # the hand capture of INTEGRATION.md: warm-up on a side stream, one capture of forward + backward, replay
            eager = stepper(loop)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    eager()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            x_hat.grad = None
            with torch.cuda.graph(graph):
                loop(x, x_hat).backward()
            static_grad = x_hat.grad   # lives in the graph's pool: every replay writes it
            steppers[form], grad_of[form] = graph.replay, (lambda g=static_grad: g)
    for form, step in steppers.items():   # warm-up: compilation, graph recording, plans, tables, allocator blocks
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        grad = grad_of.get(form, lambda: x_hat.grad)()
        values[form] = float(grad.double().abs().sum())   # the forms compute one gradient: a checksum per form goes into the record

    times = {form: [] for form in forms}
    for _ in range(args.rounds):
        for form in forms:   # interleaved: every round visits every form
            step = steppers[form]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            times[form].append((time.perf_counter() - t0) / args.steps * 1e6)
    record = {"tool": "tools/bench_compile.py", "clips": args.clips, "steps_per_window": args.steps, "rounds": args.rounds, "unit": "us per step",
              "torch": torch.__version__, "device": torch.cuda.get_device_name(0),
              "forms": {form: {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2),
                               "grad_abs_sum": values[form]} for form, t in times.items()}}
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
