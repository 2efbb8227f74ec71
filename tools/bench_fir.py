"""The HIP FIR filter (sot_fir_same_*, behind spectra.fft_convolve) against the reference's FFT route on torch ops
(spectra._fft_convolve_torch: two pads, two rfft of 8192, a complex product, irfft, fold, crop) on the same GPU, for the synthesiser's
roll-off (128 shared taps): forward, forward + backward to the audio, and forward + backward of sinusoidal_synth(apply_roll_off=True),
each eager and replayed from a captured graph.  The arms of one measurement alternate round by round in one process; per arm the
median and the minimum over the rounds are printed, in microseconds per call.

usage: python tools/bench_fir.py [--rounds 9] [--iters 200] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from sot_amd import spectra


def window_us(fn, iters):
    """Microseconds per call over `iters` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def graphed(fn):
    """fn captured once on a side stream; returns the replay callable."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def compare(label, arms, rounds, iters, lines):
    """arms: {name: callable}; alternates them for `rounds` rounds."""
    for fn in arms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            times[name].append(window_us(fn, iters))
    text = "  ".join(f"{name} median {statistics.median(t):8.2f} min {min(t):8.2f}" for name, t in times.items())
    lines.append(f"{label:<46s} {text}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fir.py measures on the GPU"
    dev = torch.device("cuda:0")
    taps = spectra.roll_off_taps(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, {args.rounds} alternating rounds of {args.iters} calls; "
             "hip = sot_fir_same_* kernels, torch = the FFT route on torch ops"]
    gen = torch.Generator(device=dev).manual_seed(1)
    for batch in (64, 256):
        samples = 4096
        audio = (torch.randn(batch, samples, device=dev, generator=gen) * 0.3).requires_grad_(True)
        up = torch.randn(batch, samples, device=dev, generator=gen)
        shared = taps[None, :].expand(batch, -1)
        amps = (torch.rand(batch, 16, 8, device=dev, generator=gen) * 0.6 + 0.1).requires_grad_(True)
        f0 = (torch.rand(batch, 16, 1, device=dev, generator=gen) * 900 + 100).requires_grad_(True)

        def fwd_hip():
            with torch.no_grad():
                return spectra.fft_convolve(audio, shared)

        def fwd_torch():
            with torch.no_grad():
                return spectra._fft_convolve_torch(audio, shared)

        def both(route):
            def run():
                audio.grad = None
                route(audio, shared).backward(up)
            return run

        def synth(rolled_by_hip):
            def run():
                amps.grad = f0.grad = None
                if rolled_by_hip:
                    out = spectra.sinusoidal_synth(amps, f0, samples, 16000, harmonic=True, apply_roll_off=True)
                else:
                    out = spectra._fft_convolve_torch(spectra.sinusoidal_synth(amps, f0, samples, 16000, harmonic=True), shared)
                out.backward(up)
            return run

        shape = f"[{batch} x {samples}, 128 taps]"
        for mode, wrap in (("eager", lambda f: f), ("graph", graphed)):
            compare(f"{shape} forward, {mode}", {"hip": wrap(fwd_hip), "torch": wrap(fwd_torch)}, args.rounds, args.iters, lines)
            compare(f"{shape} forward + backward to audio, {mode}",
                    {"hip": wrap(both(spectra.fft_convolve)), "torch": wrap(both(spectra._fft_convolve_torch))}, args.rounds, args.iters, lines)
            compare(f"{shape} synth + roll-off, fwd + bwd, {mode}", {"hip": wrap(synth(True)), "torch": wrap(synth(False))},
                    args.rounds, args.iters, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
