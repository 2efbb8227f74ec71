"""GPU checks of the HIP FIR kernels (csrc/sot_fir.hip behind sot_fir_same_forward / sot_fir_same_backward) and of the functions of
sot_amd.spectra that run them: fft_convolve, frequency_filter, sinusoidal_synth(apply_roll_off=True).

References: the integer direct sum in int64 (exact test), the float64 direct sum of the same float32 inputs (bounded test) -- both in
tests/fir_model.py -- and the reference's own results (tests/golden/fir_rolloff.npz, tools/make_golden_fir.py).  u = 2^-24 below.
  * forward and audio gradient: an L-term float32 fmaf chain, |err| <= (L + 1) u (|h| * |x|)[t] elementwise;
  * tap gradient per clip: exact fp64 products added in fp64, rounded once: |err| <= 2 u |truth| + T 2^-52 (|g| * |x|)[k];
  * tap gradient of a SHARED filter: the per-clip float32 results added in fp64 and rounded once more (sot_column_sum):
    |err| <= sum_b (per-clip bound)_b + u |truth| (the bound above has no term for cancellation between clips);
  * magnitude gradient (the tap gradient through the design's torch ops, a linear map J of 128 taps x 65 magnitudes evaluated as a
    128-point float32 FFT, at most log2(128) + 2 = 9 roundings along any path): |err| <= |J|^T (tap bound) + 9 u |J|^T |gh|.
"""
import os
import warnings

import numpy as np
import pytest
import torch

import fir_model
from conftest import GOLDEN
from gpu_util import device, native

U = 2.0 ** -24
TAPS = (3, 4, 9, 128, 129, 512)


def _tile():
    return native().FIR_TILE


def _lengths():
    t = _tile()
    return (1, 2, 61, 127, 128, 129, 300, t - 1, t, t + 1, 2 * t + 5)


def _starts(taps):
    return sorted({fir_model.default_start(taps), 0, taps - 2})


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.int32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), np.ascontiguousarray(want, np.float32).view(np.int32))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "fir_rolloff.npz")))


def _audio_layouts(values, dev, rng):
    """The same [B, T] values as a contiguous tensor and as a column slice of a wider tensor (row stride T + 7, first sample three floats
    into the row) whose other columns hold non-zero values: a kernel that reads past a row's ends instead of zero-filling shows."""
    B, T = values.shape
    wide = rng.integers(1, 9, size=(B, T + 7)).astype(np.float32)
    wide[:, 3:3 + T] = values
    return torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(dev), torch.from_numpy(wide).to(dev)[:, 3:3 + T]


@pytest.mark.gpu
@pytest.mark.parametrize("taps", TAPS)
def test_integer_data_is_exact(taps):
    """Integer audio and taps in [-8, 8]: every float32 partial sum is an integer below 2^24 (at most 512 * 64 = 32768; tap gradient at
    most 64 * 2053), so forward, audio gradient and tap gradient must EQUAL the int64 convolution -- for every length around the tile,
    batch, crop start, per-clip and shared taps, contiguous and strided rows."""
    nat, dev = native(), device()
    rng = np.random.default_rng(100 + taps)
    for T in _lengths():
        for B in (1, 3):
            x = rng.integers(-8, 9, size=(B, T))
            g = rng.integers(-8, 9, size=(B, T))
            g_dev = torch.from_numpy(g.astype(np.float32)).to(dev)
            for shared in (False, True):
                h = rng.integers(-8, 9, size=(taps,) if shared else (B, taps))
                h_dev = torch.from_numpy(h.astype(np.float32)).to(dev)
                for start in _starts(taps):
                    want = fir_model.forward(x, h, start)
                    want_gx = fir_model.grad_audio(g, h, start)
                    want_gh = fir_model.grad_taps(g, x, taps, start)
                    if shared:
                        want_gh = want_gh.sum(axis=0)
                    for x_dev in _audio_layouts(x, dev, rng):
                        where = f"T={T} L={taps} B={B} start={start} shared={shared} stride={x_dev.stride(0)}"
                        assert _same_bits(nat.fir_same_forward(x_dev, h_dev, start), want), where
                        gx, gh = nat.fir_same_backward(g_dev, x_dev, h_dev, start, need_audio=True, need_taps=True)
                        assert _same_bits(gx, want_gx), where
                        assert tuple(gh.shape) == tuple(h.shape) and _same_bits(gh, want_gh), where


BOUNDED = [(300, 9, 3, False), (300, 128, 1, True), (1025, 129, 3, True), (2053, 512, 2, False), (4096, 128, 3, False), (4096, 128, 3, True),
           (61, 3, 3, False), (129, 4, 1, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("T, taps, B, shared", BOUNDED)
def test_float_data_within_the_rounding_bound(T, taps, B, shared):
    """randn * 0.3 audio and randn taps through fft_convolve and autograd against the float64 direct sum of the same float32 inputs,
    held elementwise to the bounds of the module docstring."""
    from sot_amd import spectra
    native()
    dev = device()
    gen = torch.Generator().manual_seed(7 * T + taps)
    x = (torch.randn(B, T, generator=gen) * 0.3)
    h = torch.randn(taps if shared else (B, taps), generator=gen)
    g = torch.randn(B, T, generator=gen)
    start = fir_model.default_start(taps)
    xd = x.to(dev).requires_grad_(True)
    hd = h.to(dev).requires_grad_(True)
    out = spectra.fft_convolve(xd, hd[None, :].expand(B, -1) if shared else hd)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_FirSame")
    out.backward(g.to(dev))
    x64, h64, g64 = x.double().numpy(), h.double().numpy(), g.double().numpy()
    ax, ah, ag = np.abs(x64), np.abs(h64), np.abs(g64)

    truth = fir_model.forward(x64, h64, start)
    bound = (taps + 1) * U * fir_model.forward(ax, ah, start)
    err = np.abs(out.detach().cpu().numpy() - truth)
    print(f"forward: worst fraction of the bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()

    truth = fir_model.grad_audio(g64, h64, start)
    bound = (taps + 1) * U * fir_model.grad_audio(ag, ah, start)
    err = np.abs(xd.grad.cpu().numpy() - truth)
    print(f"audio gradient: worst fraction of the bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()

    per_clip = fir_model.grad_taps(g64, x64, taps, start)
    bound = 2 * U * np.abs(per_clip) + T * 2.0 ** -52 * fir_model.grad_taps(ag, ax, taps, start)
    truth = per_clip
    if shared:
        truth = per_clip.sum(axis=0)
        bound = bound.sum(axis=0) + U * np.abs(truth)
    err = np.abs(hd.grad.cpu().numpy() - truth)
    print(f"tap gradient: worst fraction of the bound {np.max(err / bound):.3f}")
    assert tuple(hd.grad.shape) == tuple(h.shape) and (err <= bound).all()


@pytest.mark.gpu
def test_reference_fixture_within_twice_the_bounds(gold):
    """frequency_filter on the GPU against the reference's CPU results for the same audio, magnitudes and upstream gradient: output, audio
    gradient and magnitude gradient within TWICE the bounds of the module docstring (the reference's FFT route and the kernels are each
    within one bound of the float64 truth); the synthesiser with apply_roll_off against the reference's filtered audio likewise, for the
    filter step (fed the reference's own unfiltered audio)."""
    from sot_amd import spectra
    native()
    dev = device()
    T, L, start = 4096, 128, 62
    audio = torch.from_numpy(gold["audio"]).to(dev).requires_grad_(True)
    mag = torch.from_numpy(gold["grad_mag_in"]).to(dev).requires_grad_(True)
    out = spectra.frequency_filter(audio, mag)
    out.backward(torch.from_numpy(gold["grad_up"]).to(dev))
    taps = spectra.frequency_impulse_response(torch.from_numpy(gold["grad_mag_in"])).double().numpy()
    x64, g64 = gold["audio"].astype(np.float64), gold["grad_up"].astype(np.float64)

    bound = (L + 1) * U * fir_model.forward(np.abs(x64), np.abs(taps), start)
    frac = np.max(np.abs(out.detach().cpu().numpy() - gold["grad_out"]) / bound)
    print(f"filtered audio vs reference: {frac:.3f} of the bound")
    assert frac <= 2

    bound = (L + 1) * U * fir_model.grad_audio(np.abs(g64), np.abs(taps), start)
    frac = np.max(np.abs(audio.grad.cpu().numpy() - gold["grad_audio"]) / bound)
    print(f"audio gradient vs reference: {frac:.3f} of the bound")
    assert frac <= 2

    gh = fir_model.grad_taps(g64, x64, L, start)
    tap_bound = 2 * U * np.abs(gh) + T * 2.0 ** -52 * fir_model.grad_taps(np.abs(g64), np.abs(x64), L, start)
    J = np.abs(spectra.frequency_impulse_response(torch.eye(65)).double().numpy())     # |d taps[k] / d magnitude[f]|, [65, 128]
    bound = tap_bound @ J.T + 9 * U * (np.abs(gh) @ J.T)
    frac = np.max(np.abs(mag.grad.cpu().numpy() - gold["grad_mag"]) / bound)
    print(f"magnitude gradient vs reference: {frac:.3f} of the bound")
    assert frac <= 2

    rolled = spectra.frequency_filter(torch.from_numpy(gold["audio"]).to(dev), spectra.roll_off_magnitudes(dev).expand(2, -1))
    roll = gold["rolloff_taps"].astype(np.float64)
    bound = (L + 1) * U * fir_model.forward(np.abs(x64), np.abs(roll), start)
    frac = np.max(np.abs(rolled.cpu().numpy() - gold["audio_filtered"]) / bound)
    print(f"roll-off of the reference's audio vs reference: {frac:.3f} of the bound")
    assert frac <= 2
    # the whole synthesiser: the HIP oscillator bank's audio is not the CPU's bit for bit, so this one is a plain tolerance
    synth = spectra.sinusoidal_synth(torch.from_numpy(gold["amps"]).to(dev), torch.from_numpy(gold["f0"]).to(dev), 4096, 16000, harmonic=True,
                                     apply_roll_off=True)
    assert np.abs(synth.cpu().numpy() - gold["audio_filtered"]).max() <= 1e-3 * np.abs(gold["audio_filtered"]).max()


@pytest.mark.gpu
def test_rows_are_independent_and_calls_deterministic():
    nat, dev = native(), device()
    T, L = 2 * _tile() + 5, 129
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(3, T, generator=gen).to(dev)
    h = torch.randn(3, L, generator=gen).to(dev)
    g = torch.randn(3, T, generator=gen).to(dev)
    start = fir_model.default_start(L)
    out = nat.fir_same_forward(x, h, start)
    gx, gh = nat.fir_same_backward(g, x, h, start, need_audio=True, need_taps=True)
    out2 = nat.fir_same_forward(x, h, start)
    gx2, gh2 = nat.fir_same_backward(g, x, h, start, need_audio=True, need_taps=True)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and torch.equal(gh, gh2)                     # a second call: the same bits
    alone = nat.fir_same_forward(x[1:2].clone(), h[1:2].clone(), start)
    gx1, gh1 = nat.fir_same_backward(g[1:2].clone(), x[1:2].clone(), h[1:2].clone(), start, need_audio=True, need_taps=True)
    assert torch.equal(out[1:2], alone) and torch.equal(gx[1:2], gx1) and torch.equal(gh[1:2], gh1)      # row 1 alone: the same bits
    # ... and where a tile ends does not matter either: the same samples at another offset inside a longer row of zeros
    padded = torch.zeros(1, T + 300, device=dev)
    padded[:, 300:] = x[1:2]
    shifted = nat.fir_same_forward(padded, h[1:2].clone(), start)
    keep = T - (L - 1)                                            # outputs that do not see the end of the shorter row
    assert torch.equal(shifted[:, 300:300 + keep], out[1:2, :keep])


@pytest.mark.gpu
def test_graph_replay_matches_eager():
    """Forward and backward (audio and tap gradients) captured into a graph on a side stream and replayed on new data: the eager bits."""
    from sot_amd import spectra
    native()
    dev = device()
    B, T, L = 3, 2 * _tile() + 5, 128
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(B, T, device=dev, generator=gen).requires_grad_(True)
    h = torch.randn(B, L, device=dev, generator=gen).requires_grad_(True)
    g = torch.randn(B, T, device=dev, generator=gen)

    def step():
        x.grad = h.grad = None
        out = spectra.fft_convolve(x, h)
        out.backward(g)
        return out.detach()

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    x.grad = h.grad = None
    with torch.cuda.graph(graph):
        captured = step()
    nx, nh, ng = (torch.randn(t.shape, device=dev, generator=gen) for t in (x, h, g))
    with torch.no_grad():
        x.copy_(nx)
        h.copy_(nh)
        g.copy_(ng)
    graph.replay()
    torch.cuda.synchronize()
    xe, he = nx.clone().requires_grad_(True), nh.clone().requires_grad_(True)
    eager = spectra.fft_convolve(xe, he)
    eager.backward(ng)
    assert torch.equal(captured, eager.detach()) and torch.equal(x.grad, xe.grad) and torch.equal(h.grad, he.grad)


def _controls(dev, batch=3, seed=2):
    gen = torch.Generator().manual_seed(seed)
    amps = (torch.rand(batch, 16, 8, generator=gen) * 0.6 + 0.1).to(dev)
    f0 = (torch.rand(batch, 16, 1, generator=gen) * 900 + 100).to(dev)
    return amps, f0


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_synthesiser_roll_off_is_the_filter_applied_to_its_audio(fused):
    from sot_amd import spectra
    native()
    dev = device()
    amps, f0 = _controls(dev)
    before = spectra.FUSED_SYNTH
    spectra.FUSED_SYNTH = fused
    try:
        rolled = spectra.sinusoidal_synth(amps, f0, 4096, 16000, harmonic=True, apply_roll_off=True)
        plain = spectra.sinusoidal_synth(amps, f0, 4096, 16000, harmonic=True)
    finally:
        spectra.FUSED_SYNTH = before
    assert torch.equal(rolled, spectra.frequency_filter(plain, spectra.roll_off_magnitudes(dev).expand(3, -1)))
    assert not torch.equal(rolled, plain)
    assert spectra.roll_off_taps(dev) is spectra.roll_off_taps(dev) and tuple(spectra.roll_off_taps(dev).shape) == (128,)


@pytest.mark.gpu
def test_control_gradients_through_roll_off_and_mss_equal_the_manual_chain():
    """synth -> roll-off -> MSSLoss under autograd gives the control gradients of the chain done by hand: MSS audio gradient -> FIR
    backward (sot_fir_same_backward with the shared taps) -> synthesiser backward.  Bit for bit."""
    from sot_amd import spectra
    from sot_amd.losses import MSSLoss
    nat, dev = native(), device()
    amps, f0 = _controls(dev)
    target = spectra.sinusoidal_synth(*_controls(dev, seed=3), 4096, 16000, harmonic=True, apply_roll_off=True)
    mss = MSSLoss(mag_weight=1, logmag_weight=1).to(dev)

    a1, f1 = amps.clone().requires_grad_(True), f0.clone().requires_grad_(True)
    loss = mss(target, spectra.sinusoidal_synth(a1, f1, 4096, 16000, harmonic=True, apply_roll_off=True))
    loss.backward()

    a2, f2 = amps.clone().requires_grad_(True), f0.clone().requires_grad_(True)
    plain = spectra.sinusoidal_synth(a2, f2, 4096, 16000, harmonic=True)
    taps = spectra.roll_off_taps(dev)
    rolled = nat.fir_same_forward(plain.detach(), taps, 62).requires_grad_(True)
    loss2 = mss(target, rolled)
    loss2.backward()
    grad_plain, none = nat.fir_same_backward(rolled.grad, plain.detach(), taps, 62, need_audio=True, need_taps=False)
    assert none is None
    plain.backward(grad_plain)
    assert torch.equal(loss.detach(), loss2.detach())
    assert torch.equal(a1.grad, a2.grad) and torch.equal(f1.grad, f2.grad)
    assert a1.grad.abs().max() > 0 and f1.grad.abs().max() > 0


OUTSIDE = {
    "valid": dict(taps=(2, 9), kwargs=dict(padding="valid")),
    "cross_fade": dict(taps=(2, 2, 9), kwargs=dict(cross_fade=True)),
    "two_frames": dict(taps=(2, 2, 9), kwargs={}),
    "two_taps": dict(taps=(2, 2), kwargs={}),
    "513_taps": dict(taps=(2, 513), kwargs={}),
    "float64": dict(taps=(2, 9), kwargs={}, dtype=torch.float64),
    "start_past_the_taps": dict(taps=(2, 9), kwargs=dict(delay_compensation=8)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(OUTSIDE))
def test_calls_outside_the_kernel_domain_run_the_fft_route_and_say_so_once(case):
    from sot_amd import losses, spectra
    native()
    dev = device()
    spec = OUTSIDE[case]
    gen = torch.Generator().manual_seed(13)
    dtype = spec.get("dtype", torch.float32)
    x = torch.randn(2, 600, generator=gen).to(dev, dtype)
    h = torch.randn(spec["taps"], generator=gen).to(dev, dtype)
    for key in [k for k in losses._warned if isinstance(k, tuple) and k and k[0] == "fft_convolve"]:
        losses._warned.discard(key)
    with pytest.warns(UserWarning, match="outside what the HIP FIR kernels take"):
        got = spectra.fft_convolve(x, h, **spec["kwargs"])
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*HIP FIR kernels.*")
        again = spectra.fft_convolve(x, h, **spec["kwargs"])          # once: the second call is silent
    want = spectra._fft_convolve_torch(x, h, **spec["kwargs"])
    assert got.device == x.device and got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want) and torch.equal(again, want)


@pytest.mark.gpu
def test_c_entry_points_report_the_documented_status():
    nat, dev = native(), device()
    lib = nat.load()
    B, T, L = 2, 300, 9
    x = torch.zeros(B, T, device=dev)
    h = torch.zeros(B, L, device=dev)
    y = torch.empty(B, T, device=dev)
    gh = torch.empty(B, L, device=dev)
    g = torch.zeros(B, T, device=dev)
    ws = torch.empty(int(lib.sot_fir_workspace_bytes(B, T, L)), dtype=torch.uint8, device=dev)
    assert ws.numel() == 8 * B * ((T + 511) // 512) * L
    X, H, Y, G, GH, WS = x.data_ptr(), h.data_ptr(), y.data_ptr(), g.data_ptr(), gh.data_ptr(), ws.data_ptr()
    st = nat.stream_ptr(dev)

    def fwd(audio=X, stride=T, taps=H, tstride=L, batch=B, samples=T, n=L, start=3, out=Y):
        return lib.sot_fir_same_forward(audio, stride, taps, tstride, batch, samples, n, start, out, st)

    def bwd(g=G, audio=X, stride=T, taps=H, tstride=L, batch=B, samples=T, n=L, start=3, ga=Y, gt=GH, w=WS, wb=None):
        return lib.sot_fir_same_backward(g, audio, stride, taps, tstride, batch, samples, n, start, ga, gt, w, ws.numel() if wb is None else wb, st)

    assert fwd() == nat.SOT_OK and bwd() == nat.SOT_OK
    assert fwd(batch=0) == nat.SOT_OK and bwd(batch=0) == nat.SOT_OK and bwd(ga=None, gt=None) == nat.SOT_OK
    assert fwd(tstride=0) == nat.SOT_OK and bwd(audio=None, gt=None, w=None, wb=0) == nat.SOT_OK and bwd(taps=None, ga=None) == nat.SOT_OK
    for kw in (dict(audio=None), dict(taps=None), dict(out=None)):
        assert fwd(**kw) == nat.SOT_ERR_NULL_POINTER, kw
    for kw in (dict(g=None), dict(taps=None), dict(audio=None), dict(w=None)):
        assert bwd(**kw) == nat.SOT_ERR_NULL_POINTER, kw
    for kw in (dict(batch=-1), dict(samples=0), dict(n=0), dict(stride=T - 1), dict(tstride=L - 1)):
        assert fwd(**kw) == nat.SOT_ERR_BAD_SHAPE, kw
        assert bwd(**kw) == nat.SOT_ERR_BAD_SHAPE, kw
    for kw in (dict(n=2, start=0), dict(n=513), dict(start=-1), dict(start=L - 1), dict(samples=(1 << 20) + 1, stride=(1 << 20) + 1)):
        assert fwd(**kw) == nat.SOT_ERR_UNSUPPORTED_SIZE, kw
        assert bwd(**kw) == nat.SOT_ERR_UNSUPPORTED_SIZE, kw
    assert bwd(wb=ws.numel() - 1) == nat.SOT_ERR_WORKSPACE
    for args in ((B, T, 2), (B, T, 513), (B, 0, L), (B, (1 << 20) + 1, L), (0, T, L)):
        assert lib.sot_fir_workspace_bytes(*args) == 0, args
    torch.cuda.synchronize()
    with pytest.raises(nat.SotError):
        nat.fir_same_forward(x, torch.zeros(B, 513, device=dev), 3)
