"""Writes tests/golden/eval_metrics.npz: what the reference's evaluation metrics (metrics.mse, metrics.ms_spectral_distance with the
parameters of its log-spectral distance, of its multi-scale metric and of one mixed case, metrics.wasserstein_distance) return on the CPU
for the harmonic clips of tests/golden/stft_chain.npz, for tests/test_eval_metrics.py and tests/test_eval_metrics_gpu.py.  Numbers only.
Needs the reference checkout (found through the shim of oracle/make_golden.py); never imported by a test or by the package.

    python tools/make_golden_metrics.py [--pins FILE.npz]

--pins: arrays named pin_* to store next to the reference's numbers -- MSSLoss WITH gradient (loss bits, sha256 of the gradient bytes) as
the HIP engine computed them before the metric mode was added; without the option the pins of the existing fixture are kept.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import import_reference, OUT  # noqa: E402

CLIPS = {"a": ("mss_audio_x", "mss_audio_y"), "b": ("wt_audio_x", "wt_audio_y")}     # 2 x 4096 and 3 x 3000 samples
LSD = dict(fft_sizes=[1024], mag_weight=0, logmag_weight=0, log_spectral_distance_weight=1.0, loss_type="L2")
MSS = dict(fft_sizes=[2048, 1024, 512, 256, 128, 64], mag_weight=1, logmag_weight=1, loss_type="L1")
MIXED = dict(fft_sizes=[512, 128], mag_weight=1.0, logmag_weight=0.5, log_spectral_distance_weight=0.25, loss_type="L2")
LSD4096 = dict(LSD, fft_sizes=[4096])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pins", default=None)
    args = ap.parse_args()
    import_reference()
    for name in ("mir_eval", "mir_eval.melody"):        # metrics.py imports it at module level; nothing here calls it
        sys.modules[name] = types.ModuleType(name)
    sys.modules["mir_eval"].melody = sys.modules["mir_eval.melody"]
    import metrics  # type: ignore  (the reference's, on sys.path after import_reference)

    path = os.path.join(OUT, "eval_metrics.npz")
    out = {}
    if args.pins:
        out.update({k: v for k, v in np.load(args.pins).items() if k.startswith("pin_")})
    elif os.path.exists(path):
        out.update({k: v for k, v in np.load(path).items() if k.startswith("pin_")})
    chain = np.load(os.path.join(OUT, "stft_chain.npz"))
    for tag, (kx, ky) in CLIPS.items():
        x, y = torch.from_numpy(chain[kx]), torch.from_numpy(chain[ky])
        out[f"{tag}_mse"] = metrics.mse(x, y).numpy()
        out[f"{tag}_mse_sorted"] = metrics.mse(x, y, sort=True).numpy()
        for name, kw in (("lsd", LSD), ("mss", MSS), ("mixed", MIXED), ("lsd4096", LSD4096)):
            out[f"{tag}_{name}"] = metrics.ms_spectral_distance(x, y, **kw).numpy()
        out[f"{tag}_w1"] = metrics.wasserstein_distance(x, y).numpy()
        out[f"{tag}_w2"] = metrics.wasserstein_distance(x, y, p=2).numpy()
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes;", {k: (v.tolist() if v.size < 4 else v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
