"""The reference's evaluation metrics (`metrics.py`), with its names and signatures: `mse`, `ms_spectral_distance` (the log-spectral distance
and the multi-scale spectral metric are two calls of it), `wasserstein_distance` and `compute_metrics`, everything under
`torch.inference_mode()` as there.

Routing, the package's custom:
  * float32 GPU audio [batch, samples] of one shape, every FFT size in the fused engine's set (64 ... 2048): the HIP route.  One launch of
    the fused multi-scale engine in its metric mode (csrc/sot_mss.hip: sot_spec_metrics) evaluates up to four `ms_spectral_distance`
    configurations over the union of their sizes -- no spectrogram leaves the chip, and a size that two configurations share (the 1024-point
    spectra of LSD and MSS) is fetched and transformed once.  `signal_metrics` uses that for LSD + MSS; `mse` is sot_spec_distance_forward
    on the raw audio;
  * GPU tensors outside that set (n_fft 4096, other dtypes, differing shapes): the same arithmetic on `spectra.stft_magnitude` + torch ops,
    said once;
  * CPU tensors: the reference's op sequence on torch ops.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .losses import MeanDifference, mean_difference, warn_once
from .spectra import wasserstein_distance  # noqa: F401  (metrics.py:144-149; re-exported under the reference's module name)

LSD_PARAMETERS = dict(fft_sizes=[1024], mag_weight=0, logmag_weight=0, log_spectral_distance_weight=1.0, loss_type="L2")   # metrics.py:172-180
MSS_PARAMETERS = dict(fft_sizes=[2048, 1024, 512, 256, 128, 64], mag_weight=1, logmag_weight=1, loss_type="L1")            # metrics.py:184-191
MIR_EVAL_KEYS = {"raw_pitch_accuracy": "raw", "raw_chroma_accuracy": "chroma", "octave_difference": "octave_difference"}   # metrics.py:200-210
MAX_GROUPS, MAX_SIZES = 4, 8    # include/sot_hip.h: sot_spec_metrics


def _safe_log(x, eps=1e-5):
    e = torch.tensor(eps, device=x.device)        # utils.py:145-151
    return torch.log(torch.where(x <= e, e, x))


def safe_log10(x, eps=1e-5):
    e = torch.tensor(eps, device=x.device)        # utils.py:154-157
    return torch.log10(torch.where(x <= e, e, x))


def _magnitude(audio, size):
    """features.compute_mag(size=size) (features.py:191-237): [batch, n_fft/2 + 1, frames].  CPU tensors: torch.stft on the end-padded
    signal, the reference's own ops; GPU tensors: spectra.stft_magnitude (the HIP STFT kernels up to n_fft 4096)."""
    from . import spectra
    hop = int(size * (1.0 - 0.75))
    if audio.is_cuda:
        return spectra.stft_magnitude(audio, size, hop, None).permute(0, 2, 1)
    padded = spectra.end_padded(audio.float(), size, hop)
    spec = torch.stft(padded, n_fft=size, hop_length=hop, win_length=size, window=torch.hann_window(size, device=audio.device), center=False,
                      normalized=True, return_complex=True)
    return spec.abs().float()


def _group_torch(target_audio, audio, group, per_clip):
    """metrics.py:61-87 on torch ops; per_clip: the means run over each clip's own spectrogram."""
    sizes, mag_w, log_w, lsd_w, kind = group
    dims = [1, 2] if per_clip else None
    loss = 0.0
    for size in sizes:
        t, v = _magnitude(target_audio, size), _magnitude(audio, size)
        if mag_w > 0:
            loss += mag_w * mean_difference(t, v, kind, dims=dims)
        if log_w > 0:
            loss += log_w * mean_difference(_safe_log(t), _safe_log(v), kind, dims=dims)
        if lsd_w > 0:
            loss += lsd_w * mean_difference(10 * safe_log10(t ** 2), 10 * safe_log10(v ** 2), kind, dims=dims)
    return loss


def _hip_route(target_audio, audio, groups) -> bool:
    sizes = {s for g in groups for s in g[0]}
    return (torch.is_tensor(target_audio) and torch.is_tensor(audio) and target_audio.is_cuda and audio.is_cuda and
            target_audio.dtype == torch.float32 and audio.dtype == torch.float32 and audio.ndim == 2 and target_audio.shape == audio.shape and
            audio.shape[0] > 0 and audio.shape[1] > 0 and len(groups) <= MAX_GROUPS and 0 < len(sizes) <= MAX_SIZES and
            all(s in nat.MSS_FUSED_SIZES for s in sizes) and all(0 < len(g[0]) <= MAX_SIZES for g in groups) and
            all(g[1] > 0 or g[2] > 0 or g[3] > 0 for g in groups))


def _spectral_groups(target_audio, audio, groups, per_clip=False):
    """Several ms_spectral_distance configurations of the same two signals -> one value each.  groups: (fft_sizes, mag_weight, logmag_weight,
    log_spectral_distance_weight, "L1" | "L2") tuples.  On the HIP route ONE sot_spec_metrics call serves all of them."""
    groups = [(tuple(int(s) for s in g[0]), float(g[1]), float(g[2]), float(g[3]), str(g[4]).upper()) for g in groups]
    for g in groups:
        if g[4] not in ("L1", "L2"):
            raise ValueError('Loss type ({}), must be "L1", "L2" '.format(g[4]))   # losses.py:36
    if _hip_route(target_audio, audio, groups):
        from . import spectra
        union = tuple(sorted({s for g in groups for s in g[0]}, reverse=True))
        windows = spectra._cached_windows(None, union, audio.device)      # window=None -> hann (features.py:200-201)
        out = nat.spec_metrics(target_audio, audio, union, windows, [(g[0], g[1], g[2], g[3], g[4] == "L2") for g in groups], 1e-5, per_clip)
        return [out[i] for i in range(len(groups))]
    if torch.is_tensor(audio) and audio.is_cuda:
        warn_once(("metrics", tuple(g[0] for g in groups), str(audio.dtype), str(getattr(target_audio, "dtype", None)), audio.ndim),
                  "metrics.ms_spectral_distance: this call runs spectra.stft_magnitude + torch ops instead of the fused HIP engine (it takes float32 "
                  "[batch, samples] audio of one shape, FFT sizes 64 ... 2048, at most 8 sizes and 4 configurations)")
    return [_group_torch(target_audio, audio, g, per_clip) for g in groups]


@torch.inference_mode()
def ms_spectral_distance(target_audio, audio, fft_sizes, mag_weight=1.0, logmag_weight=1.0, log_spectral_distance_weight=0, loss_type="L1",
                         per_clip=False):
    """metrics.py:51-87: over the FFT sizes, `mag_weight * D(|T|, |V|) + logmag_weight * D(safe_log |T|, safe_log |V|) +
    log_spectral_distance_weight * D(10 log10 |T|^2, 10 log10 |V|^2)` with D the mean absolute ("L1") or squared ("L2") difference and both
    logarithms clamped below eps = 1e-5.  per_clip (not in the reference): one value per clip, [batch] -- a test set is averaged clip by clip;
    the mean of batch means is biased by a short last batch."""
    if not (mag_weight > 0 or logmag_weight > 0 or log_spectral_distance_weight > 0) or len(fft_sizes) == 0:
        return 0.0      # metrics.py:66: the loop adds nothing
    return _spectral_groups(target_audio, audio, [(fft_sizes, mag_weight, logmag_weight, log_spectral_distance_weight, loss_type)], per_clip)[0]


@torch.inference_mode()
def mse(x, x_hat, sort=False):
    """metrics.py:11-13: mean((x - x_hat)^2) over every element, after sorting both along the last axis with sort=True."""
    if (torch.is_tensor(x) and torch.is_tensor(x_hat) and x.is_cuda and x_hat.is_cuda and x.dtype == torch.float32 and x_hat.dtype == torch.float32
            and x.shape == x_hat.shape and x.numel() > 0):
        if sort:
            x, x_hat = torch.sort(x, dim=-1)[0], torch.sort(x_hat, dim=-1)[0]
        return nat.spec_distance_forward(x, x_hat, 1.0, 0.0, 1e-5, l2=True)     # D = (.)^2 on the raw samples: fixed-order fp64 sums
    return MeanDifference("L2")(x, x_hat, sort=sort)


@torch.inference_mode()
def signal_metrics(x, x_hat, evaluation_metrics):
    """The metrics of metrics.py:168-217 that compare the two audio signals: `mse`, `log_spectral_distance`, `mss`, `1-wasserstein`,
    `2-wasserstein`, each when `evaluation_metrics` switches it on.  LSD and MSS come from ONE sot_spec_metrics call of two groups."""
    out = {}
    if evaluation_metrics.get("mse", False):
        out["mse"] = mse(x, x_hat)
    names = [n for n in ("log_spectral_distance", "mss") if evaluation_metrics.get(n)]
    if names:
        params = {"log_spectral_distance": LSD_PARAMETERS, "mss": MSS_PARAMETERS}
        groups = [(params[n]["fft_sizes"], params[n]["mag_weight"], params[n]["logmag_weight"], params[n].get("log_spectral_distance_weight", 0),
                   params[n]["loss_type"]) for n in names]
        for name, value in zip(names, _spectral_groups(x, x_hat, groups)):
            out[name] = value
    if evaluation_metrics.get("1-wasserstein", False):
        out["1-wasserstein"] = wasserstein_distance(x, x_hat)
    if evaluation_metrics.get("2-wasserstein", False):
        out["2-wasserstein"] = wasserstein_distance(x, x_hat, p=2)
    return out


def mean_octave_difference(ref_voicing, ref_cent, est_voicing, est_cent):
    """metrics.py:90-141: signed count of whole octaves (after half a semitone of slack) between the two pitch tracks in cents, averaged
    over the voiced reference frames; frames where either track is 0 do not count."""
    import numpy as np
    if ref_voicing.size == 0 or est_cent.size == 0 or ref_cent.size == 0:
        return 0.0
    both = np.logical_and(est_cent != 0, ref_cent != 0)
    if both.sum() == 0:
        return 0.0
    diff = (ref_cent - est_cent)[both]
    sign = np.sign(diff)
    octaves = np.floor(np.abs(diff + 50 * sign) / 1200)
    return np.sum(ref_voicing[both] * octaves * sign) / np.sum(ref_voicing)


def _mir_melody(key):
    try:
        import mir_eval.melody as melody
    except ImportError as exc:
        raise ImportError(f"compute_metrics: evaluation metric '{key}' needs the mir_eval package, which is not installed") from exc
    return melody


@torch.inference_mode()
def pitch_accuracy_fn(pred_pitch, true_pitch, type="raw", key=None):
    """metrics.py:16-48: mir_eval's raw pitch / raw chroma accuracy (or mean_octave_difference) of two pitch tensors in Hz, every frame
    voiced.  mir_eval is imported here, when a metric that needs it is asked for."""
    import numpy as np
    if type not in ("raw", "chroma", "octave_difference"):
        raise ValueError("type must be raw or chroma")
    melody = _mir_melody(key or type)
    if true_pitch.ndim == 3:
        true_pitch = true_pitch.reshape(-1, true_pitch.shape[-1])
        pred_pitch = pred_pitch.reshape(-1, pred_pitch.shape[-1])
    true_cent = melody.hz2cents(true_pitch.detach().cpu().flatten().numpy())
    pred_cent = melody.hz2cents(pred_pitch.detach().cpu().flatten().numpy())
    voicing = np.ones_like(true_cent)
    fn = {"raw": melody.raw_pitch_accuracy, "chroma": melody.raw_chroma_accuracy, "octave_difference": mean_octave_difference}[type]
    return torch.tensor(fn(voicing, true_cent, voicing, pred_cent))


@torch.inference_mode()
def compute_metrics(trainer, step_name, **outputs):
    """metrics.py:152-219: the dictionary of evaluation metrics that `trainer.evaluation_metrics` switches on, from a step's outputs.  The
    signal metrics go through signal_metrics (HIP kernels on GPU audio); the pitch metrics are a few hundred numbers on torch ops."""
    x, x_hat = outputs["x"], outputs["x_hat"]
    pitch_hz, true_pitch_hz = outputs["pitch_hz"], outputs["true_pitch_hz"]
    for required in ("pitch", "true_pitch", "true_weights"):     # metrics.py:156-160 reads them whether or not a metric uses them
        outputs[required]
    wanted = trainer.evaluation_metrics
    metrics_dict = signal_metrics(x, x_hat, {k: wanted.get(k, False) for k in ("mse", "log_spectral_distance", "mss")})
    if wanted.get("pitch_mse", False):
        pitch_mse = MeanDifference("L2")(outputs["frequency_unit"], outputs["true_frequency_unit"], sort=True)
        metrics_dict["pitch_mse"] = pitch_mse
        metrics_dict["pitch_mse_db"] = 10 * safe_log10(pitch_mse)
    for key, kind in MIR_EVAL_KEYS.items():
        if wanted.get(key, False):
            metrics_dict[key] = pitch_accuracy_fn(pitch_hz, true_pitch_hz, type=kind, key=key)
    metrics_dict.update(signal_metrics(x, x_hat, {k: wanted.get(k, False) for k in ("1-wasserstein", "2-wasserstein")}))
    return metrics_dict
