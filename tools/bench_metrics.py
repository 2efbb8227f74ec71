"""Evaluation metrics of a validation step, timed on the GPU: metrics.signal_metrics with the paper's switches (mse, log_spectral_distance,
mss) on the HIP route, next to the reference's op sequence on torch ops (torch.stft = rocFFT, abs, where / log / log10, mean) on the same GPU
tensors -- what a user who evaluates with the reference's metrics.py runs.  Both in one process, alternating, device events on the stream
around `--iters` calls after a warm-up; the launch counts come from one profiled call of each.

    python tools/bench_metrics.py [--clips 64 256] [--iters 50] [--rounds 5]      -> one JSON line
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAPER = {"mse": True, "log_spectral_distance": True, "mss": True}


def reference_ops(x, x_hat):
    """metrics.py:168-193 on torch ops (compute_mag features.py:191-237, mean_difference losses.py:7-36, safe_log / safe_log10 utils.py:145-157)"""
    from sot_amd import spectra

    def mag(a, size):
        hop = size // 4
        a = spectra.end_padded(a, size, hop)
        return torch.stft(a, n_fft=size, hop_length=hop, win_length=size, window=torch.hann_window(size, device=a.device), center=False,
                          normalized=True, return_complex=True).abs()

    def slog(m, fn):
        e = torch.tensor(1e-5, device=m.device)
        return fn(torch.where(m <= e, e, m))

    out = {"mse": torch.mean((x - x_hat) ** 2)}
    t, v = mag(x, 1024), mag(x_hat, 1024)
    out["log_spectral_distance"] = 0.0 + 1.0 * torch.mean((10 * slog(t ** 2, torch.log10) - 10 * slog(v ** 2, torch.log10)) ** 2)
    loss = 0.0
    for size in (2048, 1024, 512, 256, 128, 64):
        t, v = mag(x, size), mag(x_hat, size)
        loss = loss + 1 * torch.mean(torch.abs(t - v))
        loss = loss + 1 * torch.mean(torch.abs(slog(t, torch.log) - slog(v, torch.log)))
    out["mss"] = loss
    return out


def launches(fn):
    """device kernels of one call, from torch's profiler; None when the profiler does not see them"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as exc:  # noqa: BLE001
        print(f"bench_metrics: no launch count ({exc})", file=sys.stderr)
        return None


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
    ap.add_argument("--clips", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics.py measures on the GPU"
    from sot_amd import metrics, spectra
    dev = torch.device("cuda:0")
    result = {"samples": args.samples, "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "cases": {}}
    for clips in args.clips:
        x = spectra.harmonic_batch(clips, args.samples, seed=11, device=dev)
        x_hat = spectra.harmonic_batch(clips, args.samples, seed=12, device=dev)
        hip = lambda: metrics.signal_metrics(x, x_hat, PAPER)      # noqa: E731
        ref = lambda: reference_ops(x, x_hat)                      # noqa: E731
        with torch.inference_mode():
            a, b = hip(), ref()
            torch.cuda.synchronize()
            agree = {k: abs(float(a[k]) - float(b[k])) / abs(float(b[k])) for k in PAPER}
            for _ in range(10):      # warm-up of both
                hip()
                ref()
            torch.cuda.synchronize()
            t_hip, t_ref = [], []
            for _ in range(args.rounds):
                t_hip.append(timed(hip, args.iters))
                t_ref.append(timed(ref, args.iters))
            n_hip, n_ref = launches(hip), launches(ref)
        result["cases"][f"{clips}clips"] = {"hip_us": statistics.median(t_hip), "hip_us_rounds": t_hip, "reference_ops_us": statistics.median(t_ref),
                                            "reference_ops_us_rounds": t_ref, "hip_launches": n_hip, "reference_ops_launches": n_ref,
                                            "relative_difference": agree, "values": {k: float(a[k]) for k in PAPER}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
