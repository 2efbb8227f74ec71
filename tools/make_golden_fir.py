"""Writes tests/golden/fir_rolloff.npz: what the reference's FIR design and filtering functions (ddsp.slope_frequency_response,
frequency_impulse_response, fft_convolve, frequency_filter; synths.Sinusoidal(apply_roll_off=True)) return on the CPU, for
tests/test_fir_filter.py and tests/test_fir_filter_gpu.py.  Data only.  Needs the reference checkout (found through the shim of
oracle/make_golden.py); never imported by a test or by the package.

    python tools/make_golden_fir.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import import_reference, OUT  # noqa: E402


def main():
    _, _, synths = import_reference()
    import ddsp  # type: ignore  (the reference's, on sys.path after import_reference)

    g = torch.Generator().manual_seed(20260)
    out = {}

    # the synthesiser's roll-off: int64 decay, as synths.py:122-123 passes it
    mag = ddsp.slope_frequency_response(torch.tensor(6), n_freqs=65, f_ref=500)[0]
    out["rolloff_mag"] = mag.numpy()                                                    # [1, 65]
    out["rolloff_taps"] = ddsp.frequency_impulse_response(mag)[0].numpy()               # [128]

    # a float decay tensor [2, 3, 1]
    decay = torch.rand(2, 3, 1, generator=g) * 9 + 1
    out["slope_decay"] = decay.numpy()
    out["slope_mag"] = ddsp.slope_frequency_response(decay, n_freqs=17, f_ref=300.0).numpy()   # [2, 3, 17]

    # taps of random magnitudes for the three window cases
    rmag = torch.rand(2, 33, generator=g)
    out["rand_mag"] = rmag.numpy()
    for w in (0, 33, 32):
        out[f"rand_taps_w{w}"] = ddsp.frequency_impulse_response(rmag, window_size=w).numpy()

    # synthesiser audio with and without the roll-off
    amps = torch.rand(2, 16, 8, generator=g) * 0.6 + 0.1
    f0 = torch.rand(2, 16, 1, generator=g) * 900 + 100
    out["amps"], out["f0"] = amps.numpy(), f0.numpy()
    for roll in (False, True):
        synth = synths.Sinusoidal(n_samples=4096, sample_rate=16000, amp_scale_fn=None, freq_scale_fn=None, harmonic=True,
                                  apply_roll_off=roll)
        ctl = synth.get_controls(amps, f0)
        out["audio_filtered" if roll else "audio"] = synth.get_signal(ctl["amplitudes"], ctl["frequencies"]).numpy()

    # gradients of (frequency_filter(audio, mag) * up).sum() w.r.t. audio and magnitudes
    audio = torch.from_numpy(out["audio"]).clone().requires_grad_(True)
    gmag = (torch.rand(2, 65, generator=g) * 0.9 + 0.1).requires_grad_(True)
    up = torch.randn(2, 4096, generator=g)
    y = ddsp.frequency_filter(audio, gmag)
    (y * up).sum().backward()
    out["grad_mag_in"], out["grad_up"] = gmag.detach().numpy(), up.numpy()
    out["grad_out"] = y.detach().numpy()
    out["grad_audio"], out["grad_mag"] = audio.grad.numpy(), gmag.grad.numpy()

    # a small case of fft_convolve
    x = torch.randn(2, 61, generator=g)
    h = torch.randn(2, 9, generator=g)
    out["small_x"], out["small_h"] = x.numpy(), h.numpy()
    out["small_same"] = ddsp.fft_convolve(x, h).numpy()
    out["small_same_delay0"] = ddsp.fft_convolve(x, h, delay_compensation=0).numpy()
    out["small_valid"] = ddsp.fft_convolve(x, h, padding="valid").numpy()

    path = os.path.join(OUT, "fir_rolloff.npz")
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
