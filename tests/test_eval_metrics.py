"""CPU tests of sot_amd.metrics (the reference's metrics.py): on CPU tensors the module runs the reference's op sequence on the same ATen, so
every value agrees with tests/golden/eval_metrics.npz (tools/make_golden_metrics.py: the reference's own numbers for the harmonic clips of
stft_chain.npz) to 1e-6 relative; per-clip values average to the batch value; compute_metrics has the reference's keys and imports mir_eval
only when a metric needs it."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LSD = dict(fft_sizes=[1024], mag_weight=0, logmag_weight=0, log_spectral_distance_weight=1.0, loss_type="L2")
MSS = dict(fft_sizes=[2048, 1024, 512, 256, 128, 64], mag_weight=1, logmag_weight=1, loss_type="L1")
MIXED = dict(fft_sizes=[512, 128], mag_weight=1.0, logmag_weight=0.5, log_spectral_distance_weight=0.25, loss_type="L2")
CASES = {"lsd": LSD, "mss": MSS, "mixed": MIXED, "lsd4096": dict(LSD, fft_sizes=[4096])}
CLIPS = {"a": ("mss_audio_x", "mss_audio_y"), "b": ("wt_audio_x", "wt_audio_y")}
# the paper's evaluation_metrics (train_config.yaml of every paper experiment)
PAPER_METRICS = dict(diff_activated_partials=True, log_spectral_distance=True, mse=True, mss=True, octave_difference=True, raw_chroma_accuracy=True,
                     raw_pitch_accuracy=True)


def _clips(tag):
    chain = np.load(os.path.join(GOLDEN, "stft_chain.npz"))
    return torch.from_numpy(chain[CLIPS[tag][0]]), torch.from_numpy(chain[CLIPS[tag][1]])


def _close(got, want, rel=1e-6):
    got, want = float(got), float(want)
    assert abs(got - want) <= rel * abs(want), (got, want)


@pytest.mark.parametrize("tag", sorted(CLIPS))
def test_cpu_values_equal_the_reference(tag):
    from sot_amd import metrics
    gold = np.load(os.path.join(GOLDEN, "eval_metrics.npz"))
    x, y = _clips(tag)
    _close(metrics.mse(x, y), gold[f"{tag}_mse"])
    _close(metrics.mse(x, y, sort=True), gold[f"{tag}_mse_sorted"])
    for name, kw in CASES.items():
        got = metrics.ms_spectral_distance(x, y, **kw)
        assert got.dtype == torch.float32 and got.ndim == 0
        _close(got, gold[f"{tag}_{name}"])
    _close(metrics.wasserstein_distance(x, y), gold[f"{tag}_w1"])
    _close(metrics.wasserstein_distance(x, y, p=2), gold[f"{tag}_w2"])
    got = metrics.signal_metrics(x, y, {"mse": True, "log_spectral_distance": True, "mss": True, "1-wasserstein": True, "2-wasserstein": True})
    assert list(got) == ["mse", "log_spectral_distance", "mss", "1-wasserstein", "2-wasserstein"]
    for key, name in (("mse", "mse"), ("log_spectral_distance", "lsd"), ("mss", "mss"), ("1-wasserstein", "w1"), ("2-wasserstein", "w2")):
        _close(got[key], gold[f"{tag}_{name}"])


@pytest.mark.parametrize("name", ["lsd", "mss", "mixed"])
def test_per_clip_values_average_to_the_batch_value(name):
    from sot_amd import metrics
    x, y = _clips("b")
    whole = metrics.ms_spectral_distance(x, y, **CASES[name])
    clips = metrics.ms_spectral_distance(x, y, per_clip=True, **CASES[name])
    assert clips.shape == (3,)
    _close(clips.double().mean(), whole, rel=2e-6)       # equal clip lengths: the mean of the clips' means is the mean (two float32 roundings)
    for b in range(3):                                   # and each is the batch value of the clip alone
        _close(clips[b], metrics.ms_spectral_distance(x[b:b + 1], y[b:b + 1], **CASES[name]), rel=2e-6)


def test_zero_weights_and_bad_loss_type():
    from sot_amd import metrics
    x, y = _clips("a")
    assert metrics.ms_spectral_distance(x, y, [512], mag_weight=0, logmag_weight=0) == 0.0      # metrics.py:66: nothing is added
    with pytest.raises(ValueError):
        metrics.ms_spectral_distance(x, y, [512], loss_type="L3")


def _outputs(x, y):
    g = torch.Generator().manual_seed(5)
    hz = 100 + 900 * torch.rand(x.shape[0], 8, generator=g)
    unit = torch.rand(x.shape[0], 8, generator=g)
    return dict(x=x, x_hat=y, pitch=unit, pitch_hz=hz, true_pitch=unit.flip(1), true_pitch_hz=hz * 1.01, true_weights=torch.ones(x.shape[0], 8),
                frequency_unit=unit, true_frequency_unit=unit.flip(1))


def test_compute_metrics_has_the_reference_keys():
    from sot_amd import metrics
    x, y = _clips("a")
    gold = np.load(os.path.join(GOLDEN, "eval_metrics.npz"))
    wanted = {k: v for k, v in PAPER_METRICS.items() if k not in metrics.MIR_EVAL_KEYS}
    got = metrics.compute_metrics(types.SimpleNamespace(evaluation_metrics=wanted), "val", **_outputs(x, y))
    assert list(got) == ["mse", "log_spectral_distance", "mss"]                     # metrics.py:168-193, in its order
    for key, name in (("mse", "mse"), ("log_spectral_distance", "lsd"), ("mss", "mss")):
        _close(got[key], gold[f"a_{name}"])
    every = dict(wanted, pitch_mse=True, **{"1-wasserstein": True, "2-wasserstein": True})
    got = metrics.compute_metrics(types.SimpleNamespace(evaluation_metrics=every), "test", **_outputs(x, y))
    assert list(got) == ["mse", "log_spectral_distance", "mss", "pitch_mse", "pitch_mse_db", "1-wasserstein", "2-wasserstein"]
    out = _outputs(x, y)
    want = torch.mean((torch.sort(out["frequency_unit"], dim=-1)[0] - torch.sort(out["true_frequency_unit"], dim=-1)[0]) ** 2)
    _close(got["pitch_mse"], want)
    _close(got["pitch_mse_db"], 10 * torch.log10(torch.clamp(want, min=1e-5)))
    _close(got["1-wasserstein"], gold["a_w1"])
    with pytest.raises(KeyError):                                                   # metrics.py:154-160 reads these outputs unconditionally
        metrics.compute_metrics(types.SimpleNamespace(evaluation_metrics={}), "val", x=x, x_hat=y)


def test_mir_eval_is_imported_only_when_asked_for():
    import importlib.util
    from sot_amd import metrics
    assert importlib.util.find_spec("mir_eval") is None, "this test describes a machine without mir_eval"
    x, y = _clips("a")
    for key in metrics.MIR_EVAL_KEYS:
        with pytest.raises(ImportError, match=key):
            metrics.compute_metrics(types.SimpleNamespace(evaluation_metrics={key: True}), "val", **_outputs(x, y))
    with pytest.raises(ImportError, match="raw_pitch_accuracy"):
        metrics.compute_metrics(types.SimpleNamespace(evaluation_metrics=PAPER_METRICS), "val", **_outputs(x, y))


def test_mean_octave_difference():
    from sot_amd import metrics
    ref = np.array([1200.0, 2400.0, 0.0, 3600.0, 4800.0])
    est = np.array([2400.0, 2430.0, 1200.0, 1190.0, 4800.0])
    ones = np.ones(5)
    # -1 octave, 0 (30 cents), skipped (reference 0), +2 octaves (2410 + 50 cents), 0: (-1 + 2) / 5 voiced frames
    assert metrics.mean_octave_difference(ones, ref, ones, est) == pytest.approx(0.2)
    assert metrics.mean_octave_difference(ones, np.zeros(5), ones, est) == 0.0
    assert metrics.mean_octave_difference(np.ones(0), np.ones(0), np.ones(0), np.ones(0)) == 0.0


def test_module_source_and_binding():
    import re
    from sot_amd import _native as nat, metrics
    assert "oracle" not in inspect.getsource(metrics)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sot_hip.h")).read()
    assert int(re.search(r"#define SOT_ABI_VERSION (\d+)", header).group(1)) == nat.ABI_VERSION >= 16
    assert "sot_spec_metrics(" in header and "sot_spec_metrics_workspace_bytes(" in header
    assert {"sot_spec_metrics", "sot_spec_metrics_workspace_bytes"} <= set(nat.EXPORTS)
    assert int(re.search(r"#define SOT_METRIC_MAX_GROUPS (\d+)", header).group(1)) == nat.METRIC_MAX_GROUPS == metrics.MAX_GROUPS
    assert metrics.wasserstein_distance is __import__("sot_amd").spectra.wasserstein_distance


def test_c_abi_argument_errors_on_the_host():
    """decided before anything is enqueued: no GPU is needed to see the status codes"""
    import ctypes
    from sot_amd import _native as nat
    lib = nat.load(build_if_missing=False)

    def call(sizes, groups, batch=2):
        n = len(sizes)
        arr = (ctypes.c_int * n)(*sizes)
        wins = (ctypes.c_void_p * n)(*[4096] * n)            # never dereferenced: an error is returned first
        grp = (nat.SotMetricGroup * max(1, len(groups)))()
        for i, (gs, mag, log, lsd, l2) in enumerate(groups):
            grp[i].n_sizes = len(gs)
            for j, s in enumerate(gs):
                grp[i].fft_sizes[j] = s
            grp[i].mag_weight, grp[i].logmag_weight, grp[i].lsd_weight, grp[i].l2 = mag, log, lsd, l2
        return lib.sot_spec_metrics(None, 4096, None, 4096, batch, 4096, ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(wins, ctypes.c_void_p), n,
                                    ctypes.cast(grp, ctypes.c_void_p), len(groups), 1e-5, 0, None, None, 0, None)

    one = ((1024,), 1.0, 0.0, 0.0, 0)
    assert call([1024], [one] * 5) == nat.SOT_ERR_BAD_SHAPE
    assert call([2048, 1024, 512, 256, 128, 64, 2048, 1024, 512], [one]) == nat.SOT_ERR_BAD_SHAPE
    assert call([4096], [((4096,), 1.0, 0.0, 0.0, 0)]) == nat.SOT_ERR_UNSUPPORTED_SIZE
    assert call([1024], [((1024,), 0.0, 0.0, -1.0, 1)]) == nat.SOT_ERR_BAD_SHAPE
    assert call([1024, 1024], [one]) == nat.SOT_ERR_BAD_SHAPE                       # a size twice in the union
    assert call([1024], [((512,), 1.0, 0.0, 0.0, 0)]) == nat.SOT_ERR_BAD_SHAPE      # a group's size outside the union
    assert call([1024], [one], batch=0) == nat.SOT_OK                               # nothing to do, nothing is touched
    assert call([1024], [one]) == nat.SOT_ERR_NULL_POINTER
    assert lib.sot_spec_metrics_workspace_bytes(64, 4096, (ctypes.c_int * 6)(2048, 1024, 512, 256, 128, 64), 6, 2) == 8 * 2 * 64 * 48
    assert lib.sot_spec_metrics_workspace_bytes(64, 4096, (ctypes.c_int * 1)(4096), 1, 1) == 0


def test_tables_cached_under_inference_mode_are_ordinary_tensors():
    """the metrics run under torch.inference_mode(); a window they are first to ask for must still serve a differentiated step later"""
    from sot_amd import spectra
    with torch.inference_mode():
        win = spectra._cached_window(None, 96, torch.device("cpu"))
    assert not win.is_inference()
    assert spectra._cached_window(None, 96, torch.device("cpu")) is win
