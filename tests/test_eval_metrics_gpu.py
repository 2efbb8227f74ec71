"""-m gpu: the evaluation metrics on the HIP route (sot_amd.metrics -> sot_spec_metrics, the metric mode of the fused multi-scale engine in
csrc/sot_mss.hip; `mse` on sot_spec_distance_forward).

  * bit pin: a group without LSD weight is the loss engine's arithmetic in the loss engine's order -- torch.equal to sot_mss_loss_and_grad /
    MSSLoss; MSSLoss WITH gradient has the bits it had before the metric mode existed (eval_metrics.npz: pin_*, captured on that build);
  * accuracy of the LSD term and of the mixed group against the reference's op sequence in float64 on the CPU:
        e_new <= 4 max(e_ref, e_stft) + 1e-6 |f64|,
    e_ref the error of the reference's own float32 result, e_stft the error of the float64 distance arithmetic applied to the magnitudes of the
    HIP STFT kernels (spectra.stft_magnitude: the float32 transform's error without the new arithmetic); 4 is what
    test_random_mss_cases_against_float64 grants a float32 chain, the additive term covers the last float32 rounding;
  * every frame / range boundary of the six scales, both grid forms, strided rows, clamped and identical signals;
  * two groups in one pass equal the two single-group calls bit for bit; MSE; the fallbacks say so once; C-ABI status codes.

Observed on MI355X (e_new / e_ref / e_stft, relative to |f64|): DESIGN.md section 6."""
import ctypes
import hashlib
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (2048, 1024, 512, 256, 128, 64)
LSD = dict(fft_sizes=[1024], mag_weight=0, logmag_weight=0, log_spectral_distance_weight=1.0, loss_type="L2")
MSS = dict(fft_sizes=list(SIZES), mag_weight=1, logmag_weight=1, loss_type="L1")
MIXED = dict(fft_sizes=[512, 128], mag_weight=1.0, logmag_weight=0.5, log_spectral_distance_weight=0.25, loss_type="L2")
CLIPS = {"a": ("mss_audio_x", "mss_audio_y"), "b": ("wt_audio_x", "wt_audio_y")}
PINS = {"l1mag": dict(mag_weight=1.0, logmag_weight=0.0), "l1both": dict(mag_weight=1.0, logmag_weight=1.0),
        "l2": dict(mag_weight=0.7, logmag_weight=0.3, loss_type="L2")}
EPS = float(np.float32(1e-5))      # the float32 value the reference's `torch.tensor(eps)` holds (utils.py:148, 155)


def _gold():
    return np.load(os.path.join(GOLDEN, "eval_metrics.npz"))


def _fixture_clips(tag):
    chain = np.load(os.path.join(GOLDEN, "stft_chain.npz"))
    return torch.from_numpy(chain[CLIPS[tag][0]]), torch.from_numpy(chain[CLIPS[tag][1]])


_CLIP_CACHE = {}


def _clips(batch, samples, seed=0):
    """harmonic clips and a detuned estimate (the generator of test_mss_fused.py)"""
    key = (batch, samples, seed)
    if key not in _CLIP_CACHE:
        g = torch.Generator().manual_seed(1000 * seed + samples + batch)
        t = torch.arange(samples) / 16000.0
        f0 = 60 + 900 * torch.rand(batch, 1, generator=g)
        x = sum((0.5 / k) * torch.sin(2 * np.pi * k * f0 * t + k) for k in range(1, 6)) + 0.02 * torch.randn(batch, samples, generator=g)
        f1 = f0 * (1 + 0.05 * torch.randn(batch, 1, generator=g))
        y = sum((0.45 / k) * torch.sin(2 * np.pi * k * f1 * t + 0.3 * k) for k in range(1, 6)) + 0.02 * torch.randn(batch, samples, generator=g)
        _CLIP_CACHE[key] = (x.float(), y.float())
    return _CLIP_CACHE[key]


def _group(kw):
    return (tuple(kw["fft_sizes"]), float(kw["mag_weight"]), float(kw["logmag_weight"]), float(kw.get("log_spectral_distance_weight", 0)),
            kw["loss_type"].upper() == "L2")


def _mag64_cpu(audio, size):
    """features.compute_mag in float64 on the CPU (the hann window's float32 values, as the reference builds it)"""
    from sot_amd import spectra
    hop = size // 4
    a = spectra.end_padded(audio.double(), size, hop)
    win = torch.hann_window(size).double()
    return torch.stft(a, n_fft=size, hop_length=hop, win_length=size, window=win, center=False, normalized=True, return_complex=True).abs()


def _mag_hip_stft(audio, size):
    """the magnitudes of the HIP STFT kernels (csrc/sot_stft.hip), as float64 values: [batch, frames, bins]"""
    from gpu_util import device
    from sot_amd import spectra
    with torch.no_grad():
        return spectra.stft_magnitude(audio.to(device()), size, size // 4, None).cpu().double()


def _distance64(mag, x, y, kw, per_clip=False):
    """metrics.py:61-87 in float64 on the magnitudes `mag` supplies"""
    sizes, mag_w, log_w, lsd_w, l2 = _group(kw)
    total = 0.0
    for size in sizes:
        t, v = mag(x, size), mag(y, size)

        def mean(d):
            d = d ** 2 if l2 else d.abs()
            return d.mean(dim=(1, 2)) if per_clip else d.mean()

        clamp = lambda m: torch.where(m <= EPS, torch.full_like(m, EPS), m)      # noqa: E731
        if mag_w > 0:
            total = total + mag_w * mean(t - v)
        if log_w > 0:
            total = total + log_w * mean(torch.log(clamp(t)) - torch.log(clamp(v)))
        if lsd_w > 0:
            total = total + lsd_w * mean(10 * torch.log10(clamp(t ** 2)) - 10 * torch.log10(clamp(v ** 2)))
    return total


def _accuracy(label, got, ref32, x, y, kw, per_clip=False):
    """the criterion of the module docstring; prints the three errors relative to |f64|"""
    want = _distance64(_mag64_cpu, x, y, kw, per_clip)
    stft = _distance64(_mag_hip_stft, x, y, kw, per_clip)
    got, ref32 = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref32).detach().cpu().double()
    want, stft = torch.as_tensor(want).double(), torch.as_tensor(stft).double()
    e_new, e_ref, e_stft = (got - want).abs(), (ref32 - want).abs(), (stft - want).abs()
    scale = want.abs().clamp_min(1e-300)
    print(f"ACCURACY {label}: f64={want.flatten()[0].item():.9g} e_new={(e_new / scale).max().item():.3e} e_ref={(e_ref / scale).max().item():.3e} "
          f"e_stft={(e_stft / scale).max().item():.3e}")
    assert torch.isfinite(got).all()
    bound = 4 * torch.maximum(e_ref, e_stft) + 1e-6 * want.abs()
    assert bool((e_new <= bound).all()), (label, e_new.tolist(), e_ref.tolist(), e_stft.tolist(), want.tolist())


def _windows(sizes):
    from gpu_util import device
    from sot_amd import spectra
    return [spectra._cached_window(None, s, device()) for s in sizes]


# ---- 1. bit pin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PINS))
@pytest.mark.parametrize("per_clip", [False, True])
def test_group_without_lsd_has_the_bits_of_the_loss_engine(name, per_clip):
    from gpu_util import device, native
    from sot_amd import metrics
    from sot_amd.losses import MSSLoss
    nat = native()
    kw = PINS[name]
    x, y = (t.to(device()) for t in _fixture_clips("a"))
    got = metrics.ms_spectral_distance(x, y, list(SIZES), kw["mag_weight"], kw["logmag_weight"], 0, kw.get("loss_type", "L1"), per_clip=per_clip)
    engine, _ = nat.mss_loss_and_grad(x, y, SIZES, _windows(SIZES), kw["mag_weight"], kw["logmag_weight"], 1e-5, kw.get("loss_type") == "L2", per_clip,
                                      want_grad=False)
    assert got.dtype == torch.float32 and got.shape == engine.shape and torch.equal(got, engine)
    with torch.no_grad():
        assert torch.equal(got, MSSLoss(**kw)(x, y, **({"dims": (1, 2)} if per_clip else {})))
    # the training instantiations were not touched: MSSLoss WITH gradient has the bits of the build before the metric mode
    gold = _gold()
    tag = f"pin_{name}_{'clip' if per_clip else 'all'}"
    yd = y.clone().requires_grad_(True)
    loss = MSSLoss(**kw)(x, yd, **({"dims": (1, 2)} if per_clip else {}))
    loss.sum().backward()
    assert np.array_equal(loss.detach().cpu().numpy(), gold[tag + "_loss"])
    assert hashlib.sha256(yd.grad.cpu().numpy().tobytes()).digest() == gold[tag + "_grad_sha256"].tobytes()


# ---- 2. accuracy of the LSD term and of the mixed group -----------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(CLIPS))
@pytest.mark.parametrize("name,kw", [("lsd", LSD), ("mixed", MIXED)])
def test_accuracy_against_float64(tag, name, kw):
    from gpu_util import device, native
    from sot_amd import metrics
    native()
    x, y = _fixture_clips(tag)
    got = metrics.ms_spectral_distance(x.to(device()), y.to(device()), **kw)
    assert got.dtype == torch.float32 and got.ndim == 0
    _accuracy(f"{name}/{tag}", got, torch.from_numpy(_gold()[f"{tag}_{name}"]), x, y, kw)


# ---- 3. shapes -----------------------------------------------------------------------------------------------------------------------
def _check_shape(x, y, xd=None, yd=None, label=""):
    """One launch of three groups (LSD, MSS, mixed) on a shape: the MSS group has the loss engine's bits, the LSD and the mixed group meet the
    accuracy criterion (e_ref: the module's CPU route, the reference's op sequence in float32); per-clip values are those of the clip alone."""
    from gpu_util import device, native
    from sot_amd import metrics
    nat = native()
    xd = x.to(device()) if xd is None else xd
    yd = y.to(device()) if yd is None else yd
    groups = [_group(LSD), _group(MSS), _group(MIXED)]
    wins = _windows(SIZES)
    out = nat.spec_metrics(xd, yd, SIZES, wins, groups)
    clip = nat.spec_metrics(xd, yd, SIZES, wins, groups, per_clip=True)
    assert out.shape == (3,) and clip.shape == (3, x.shape[0])
    engine, _ = nat.mss_loss_and_grad(xd, yd, SIZES, wins, 1.0, 1.0, want_grad=False)
    engine_clip, _ = nat.mss_loss_and_grad(xd, yd, SIZES, wins, 1.0, 1.0, per_clip=True, want_grad=False)
    assert torch.equal(out[1], engine) and torch.equal(clip[1], engine_clip)
    last = x.shape[0] - 1
    alone = nat.spec_metrics(xd[last:], yd[last:], SIZES, wins, groups, per_clip=True)
    assert torch.equal(alone[:, 0], clip[:, last])
    assert torch.equal(nat.spec_metrics(xd, yd, SIZES, wins, groups), out)          # deterministic
    for i, (name, kw) in enumerate((("lsd", LSD), ("mss", MSS), ("mixed", MIXED))):
        if name == "mss":
            continue
        ref32 = metrics.ms_spectral_distance(x, y, **kw)
        _accuracy(f"{name}/{label}", out[i], ref32, x, y, kw)
        ref32_clip = metrics.ms_spectral_distance(x, y, per_clip=True, **kw)
        _accuracy(f"{name}/{label}/per_clip", clip[i], ref32_clip, x, y, kw, per_clip=True)
    return out, clip


@pytest.mark.parametrize("samples", [1, 63, 64, 65, 255, 300, 1023, 1024, 1025, 4096, 4097, 5000])
def test_frame_and_range_boundaries(samples):
    x, y = _clips(3, samples)
    _check_shape(x, y, label=f"3x{samples}")


@pytest.mark.parametrize("batch", [1, 64, 96])
def test_batches_and_both_grid_forms(batch):
    """96 clips x 48 tasks = 4608 > 16 x 256 wave slots: the smallest batch in 16-wave workgroups"""
    x, y = _clips(batch, 4096)
    _check_shape(x, y, label=f"{batch}x4096")


def test_strided_rows():
    from gpu_util import device
    x, y = _clips(3, 1500)
    wide_x, wide_y = torch.zeros(3, 1801, device=device()), torch.full((3, 2003), 7.0, device=device())
    wide_x[:, :1500], wide_y[:, 1:1501] = x.to(device()), y.to(device())
    xs, ys = wide_x[:, :1500][:, ::1], wide_y[:, 1:1501][:, ::1]          # row strides 1801 / 2003 > samples; the second at an odd offset
    assert xs.stride(0) == 1801 and ys.stride(0) == 2003 and not ys.is_contiguous()
    strided, strided_clip = _check_shape(x, y, xs, ys, label="strided 3x1500")
    dense, dense_clip = _check_shape(x, y, label="dense 3x1500")
    assert torch.equal(strided, dense) and torch.equal(strided_clip, dense_clip)


def test_all_zero_target_and_identical_signals():
    from gpu_util import device, native
    from sot_amd import metrics
    native()
    x, y = _clips(3, 4096)
    zero = torch.zeros_like(x)
    out, clip = _check_shape(zero, y, label="zero target 3x4096")      # every target bin at the clamp: finite, and as accurate as elsewhere
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(clip).all()) and float(out[0]) > 0
    yd = y.to(device())
    got = metrics.signal_metrics(yd, yd.clone(), {"mse": True, "log_spectral_distance": True, "mss": True})
    assert all(float(v) == 0.0 for v in got.values()), got
    same = native().spec_metrics(yd, yd.clone(), SIZES, _windows(SIZES), [_group(LSD), _group(MSS), _group(MIXED)], per_clip=True)
    assert float(same.abs().max()) == 0.0


# ---- 4. one pass, two groups -----------------------------------------------------------------------------------------------------------
def test_two_groups_in_one_pass_equal_the_single_calls():
    from gpu_util import device, native
    from sot_amd import metrics
    native()
    for x, y in (_fixture_clips("a"), _clips(5, 5000)):
        xd, yd = x.to(device()), y.to(device())
        both = metrics.signal_metrics(xd, yd, {"log_spectral_distance": True, "mss": True})
        assert list(both) == ["log_spectral_distance", "mss"]
        assert torch.equal(both["log_spectral_distance"], metrics.ms_spectral_distance(xd, yd, **LSD))      # the shared 1024-point scale
        assert torch.equal(both["mss"], metrics.ms_spectral_distance(xd, yd, **MSS))                        # changes neither value
        # whatever the order of the groups and of the union
        nat = native()
        a = nat.spec_metrics(xd, yd, SIZES, _windows(SIZES), [_group(MSS), _group(LSD)])
        rev = tuple(reversed(SIZES))
        b = nat.spec_metrics(xd, yd, rev, _windows(rev), [_group(LSD), _group(MSS)])
        assert torch.equal(a[0], both["mss"]) and torch.equal(a[1], both["log_spectral_distance"])
        assert torch.equal(b[0], both["log_spectral_distance"]) and torch.equal(b[1], both["mss"])


# ---- 5. MSE ----------------------------------------------------------------------------------------------------------------------------
def test_mse():
    from gpu_util import device, native
    from sot_amd import metrics
    native()
    for x, y in (_fixture_clips("a"), _fixture_clips("b"), _clips(64, 4096)):
        xd, yd = x.to(device()), y.to(device())
        got = metrics.mse(xd, yd)
        want = float(((x.double() - y.double()) ** 2).mean())
        assert got.dtype == torch.float32 and got.ndim == 0 and abs(float(got) - want) <= 1e-6 * want
        srt = metrics.mse(xd, yd, sort=True)
        assert torch.equal(srt, metrics.mse(torch.sort(xd, dim=-1)[0], torch.sort(yd, dim=-1)[0]))
        want = float(((torch.sort(x.double(), dim=-1)[0] - torch.sort(y.double(), dim=-1)[0]) ** 2).mean())
        assert abs(float(srt) - want) <= 1e-6 * want
    gold = _gold()
    x, y = (t.to(device()) for t in _fixture_clips("a"))
    assert abs(float(metrics.mse(x, y)) - float(gold["a_mse"])) <= 2e-6 * float(gold["a_mse"])


# ---- 6. fallbacks ----------------------------------------------------------------------------------------------------------------------
def test_fallbacks_return_the_composition_and_say_so_once():
    from gpu_util import device, native
    from sot_amd import metrics
    native()
    gold = _gold()
    x, y = (t.to(device()) for t in _fixture_clips("a"))
    for args, want in (((x, y, [4096], 0, 0, 1.0, "L2"), gold["a_lsd4096"]),                           # a size outside the fused engine's set
                       ((x.double(), y.double(), [1024], 0, 0, 1.0, "L2"), gold["a_lsd"])):         # float64 GPU audio
        with pytest.warns(UserWarning, match="instead of the fused HIP engine"):
            got = metrics.ms_spectral_distance(*args)
        assert abs(float(got) - float(want)) <= 2e-5 * float(want), (float(got), float(want))
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            again = metrics.ms_spectral_distance(*args)                                               # said once
        assert not [w for w in seen if "fused HIP engine" in str(w.message)] and float(again) == float(got)


# ---- 7. C-ABI errors -------------------------------------------------------------------------------------------------------------------
def test_c_abi_errors_launch_nothing():
    from gpu_util import device, native
    nat = native()
    lib = nat.load(build_if_missing=False)
    dev = device()
    x, y = (t.to(dev) for t in _fixture_clips("a"))
    out = torch.full((4, 2), -7.0, device=dev)
    ws = torch.full((1 << 16,), -7.0, dtype=torch.float64, device=dev)

    def call(sizes, groups, batch=2):
        n = len(sizes)
        arr = (ctypes.c_int * n)(*sizes)
        wins = [torch.hann_window(max(64, min(s, 4096)), device=dev) for s in sizes]
        wptr = (ctypes.c_void_p * n)(*[w.data_ptr() for w in wins])
        grp = (nat.SotMetricGroup * max(1, len(groups)))()
        for i, (gs, mag, log, lsd, l2) in enumerate(groups):
            grp[i].n_sizes = len(gs)
            for j, s in enumerate(gs):
                grp[i].fft_sizes[j] = s
            grp[i].mag_weight, grp[i].logmag_weight, grp[i].lsd_weight, grp[i].l2 = mag, log, lsd, l2
        rc = lib.sot_spec_metrics(x.data_ptr(), 4096, y.data_ptr(), 4096, batch, 4096, ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(wptr, ctypes.c_void_p), n,
                                  ctypes.cast(grp, ctypes.c_void_p), len(groups), 1e-5, 0, out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                  nat.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc

    one = ((1024,), 1.0, 0.0, 0.0, 0)
    assert call([1024], [one] * 5) == nat.SOT_ERR_BAD_SHAPE
    assert call([2048, 1024, 512, 256, 128, 64, 2048, 1024, 512], [one]) == nat.SOT_ERR_BAD_SHAPE
    assert call([4096], [((4096,), 1.0, 0.0, 0.0, 0)]) == nat.SOT_ERR_UNSUPPORTED_SIZE
    assert call([1024], [((1024,), 0.0, 0.0, 0.0, 1)]) == nat.SOT_ERR_BAD_SHAPE
    assert call([1024], [one], batch=0) == nat.SOT_OK
    assert float(out.min()) == -7.0 == float(out.max()) and float(ws.min()) == -7.0 == float(ws.max())      # nothing was launched
    assert call([1024], [one]) == nat.SOT_OK                                                                  # and the valid call writes out[0] alone
    assert float(out[0, 0]) > 0 and float(out.flatten()[1:].max()) == -7.0
    with pytest.raises(nat.SotError) as err:
        nat.spec_metrics(x, y, (4096,), [torch.hann_window(4096, device=dev)], [((4096,), 1.0, 0.0, 0.0, False)])
    assert err.value.status == nat.SOT_ERR_UNSUPPORTED_SIZE


# ---- 8. the metrics leave nothing behind that a training step cannot use ---------------------------------------------------------------
def test_training_step_after_an_evaluation_shares_the_cached_windows():
    """the metrics run under torch.inference_mode() and may be the first to ask for a window: the cached table must be an ordinary tensor, or
    the differentiated STFT / MSSLoss of the next training step could not save it for backward"""
    from gpu_util import device, native
    from sot_amd import metrics, spectra
    from sot_amd.losses import MSSLoss
    native()
    dev = device()
    x, y = (t.to(dev) for t in _fixture_clips("a"))
    sizes = [1024, 256]
    metrics.ms_spectral_distance(x, y, sizes, 1.0, 1.0, 1.0, "L2")
    metrics.wasserstein_distance(x, y, n_fft=256)
    for size in sizes:
        assert not spectra._cached_window(None, size, dev).is_inference()
    yd = y.clone().requires_grad_(True)
    (spectra.stft_magnitude(yd, 256, 64, None).sum() + MSSLoss(fft_sizes=sizes, mag_weight=1.0)(x, yd)).backward()
    assert bool(torch.isfinite(yd.grad).all()) and float(yd.grad.abs().max()) > 0
