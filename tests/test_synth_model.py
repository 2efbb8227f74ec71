"""tests/synth_model.py (the float64 model the synthesiser's GPU tests compare against) checked on the CPU: against the reference's own
outputs and autograd gradients (tests/golden/stft_chain.npz o1_* / o2_*, synth_generator.npz) and against the package's CPU route
(torch ops, pinned bit for bit to the reference).  Phases and envelopes: identical bits.  Audio and gradients: within the model's
per-element float32 bounds (the CPU's float32 sin / cos are held to the same U_SIN as the device's)."""
import os

import numpy as np
import pytest
import torch

import synth_model as sm
from conftest import GOLDEN
from sot_amd import spectra

SR = 16000


def _cpu_phases(freq):
    return torch.cumsum(torch.from_numpy(freq) * (2.0 * torch.pi) / float(SR), dim=1).numpy()


def _check_bank(freq, amp, up, audio, grad_freq, grad_amp):
    K = freq.shape[-1]
    m = sm.oscillator_bank(freq, amp, SR)
    assert np.array_equal(m.phase, _cpu_phases(freq))                      # ATen's double-accumulated cumsum: the same float32, bit for bit
    assert m.ties.mean() <= sm.TIE_SHARE
    b = sm.oscillator_bank_backward(freq, amp, SR, up, fwd=m)
    assert sm.ratio(audio - m.audio, sm.audio_bound(m, K)) <= 1.0
    assert sm.grad_amp_ratio(grad_amp, b) <= 1.0
    assert np.all(grad_amp[m.muted] == 0.0)
    return sm.ratio(grad_freq - b.grad_freq, sm.grad_freq_bound(b))


@pytest.mark.parametrize("tag", ("o1", "o2"))
def test_model_matches_the_references_oscillator_bank(tag):
    fx = np.load(os.path.join(GOLDEN, "stft_chain.npz"))
    r = _check_bank(fx[f"{tag}_freq"], fx[f"{tag}_amp"], fx[f"{tag}_up"], fx[f"{tag}_audio"], fx[f"{tag}_grad_freq"], fx[f"{tag}_grad_amp"])
    assert r <= 1.0, r


BANK_SHAPES = [(1, 5, 4), (2, 513, 5), (3, 4608, 4), (2, 197, 17), (1, 101, 65), (3, 144, 129), (1, 29, 257), (2, 72, 512)]


@pytest.mark.parametrize("batch,samples,k", BANK_SHAPES)
def test_model_matches_the_cpu_oscillator_bank(batch, samples, k):
    freq, amp, up = sm.bank_inputs(samples + k, batch, samples, k)
    assert (freq == sm.NYQ).any() and (freq == sm.BELOW_NYQ).any()
    f, a = torch.from_numpy(freq).requires_grad_(True), torch.from_numpy(amp).requires_grad_(True)
    audio = spectra.oscillator_bank(f, a, SR)
    (audio * torch.from_numpy(up)).sum().backward()
    r = _check_bank(freq, amp, up, audio.detach().numpy(), f.grad.numpy(), a.grad.numpy())
    assert r <= 1.0, r


def test_model_envelopes_match_the_references_resamplers():
    fx = np.load(os.path.join(GOLDEN, "synth_generator.npz"))
    hann = torch.hann_window(512).numpy()
    a, f = sm.envelopes(fx["amp_frames"], fx["freq_frames"], hann, 4096, SR, False)
    assert np.array_equal(f, fx["freq_bilinear_4096"])
    # amp_window_4096 is the plain resampler, without the Nyquist mask: frequencies of zero keep every amplitude
    a, _ = sm.envelopes(fx["amp_frames"], np.zeros_like(fx["freq_frames"]), hann, 4096, SR, False)
    assert np.array_equal(a, fx["amp_window_4096"])
    m = sm.synth(fx["amp_frames"], fx["f0_frames"], hann, 4096, SR, True)
    K = fx["amp_frames"].shape[-1]
    assert m.ties.mean() <= sm.TIE_SHARE
    assert sm.ratio(fx["synth_audio"] - m.audio, sm.audio_bound(m, K)) <= 1.0


SYNTH_SHAPES = [(1, 1, 2, 4, False), (2, 2, 3, 5, True), (3, 5, 256, 4, True), (2, 5, 64, 17, False), (1, 2, 33, 128, True),
                (2, 5, 8, 129, False), (1, 5, 17, 512, True), (2, 1, 4, 257, False)]


@pytest.mark.parametrize("batch,frames,hop,k,harmonic", SYNTH_SHAPES)
def test_model_matches_the_cpu_synthesiser(batch, frames, hop, k, harmonic):
    samples = frames * hop
    amp, freq = sm.control_inputs(7 * samples + k, batch, frames, k, harmonic)
    up = np.random.default_rng(k).standard_normal((batch, samples)).astype(np.float32)
    hann = torch.hann_window(2 * hop).numpy()
    m = sm.synth(amp, freq, hann, samples, SR, harmonic)
    ta, tf = torch.from_numpy(amp).requires_grad_(True), torch.from_numpy(freq).requires_grad_(True)
    full = tf * torch.linspace(1.0, float(k), k) if harmonic else tf
    masked = torch.where(full >= SR / 2.0, torch.zeros_like(ta), ta)
    assert np.array_equal(m.amp_env, spectra.upsample_window(masked, samples).detach().numpy())
    assert np.array_equal(m.freq_env, spectra.upsample_linear(full, samples).detach().numpy())
    assert np.array_equal(m.phase, _cpu_phases(m.freq_env))
    assert m.ties.mean() <= sm.TIE_SHARE
    audio = spectra.sinusoidal_synth(ta, tf, samples, SR, harmonic=harmonic)
    assert sm.ratio(audio.detach().numpy() - m.audio, sm.audio_bound(m, k)) <= 1.0
    (audio * torch.from_numpy(up)).sum().backward()
    b = sm.synth_backward(amp, freq, hann, samples, SR, harmonic, up, fwd=m)
    assert b.grad_amp.shape == ta.grad.shape and b.grad_freq.shape == tf.grad.shape
    ra = sm.ratio(ta.grad.numpy() - b.grad_amp, b.amp_bound)
    rf = sm.ratio(tf.grad.numpy() - b.grad_freq, b.freq_bound)
    assert ra <= 1.0 and rf <= 1.0, (ra, rf)
    assert np.all(ta.grad.numpy()[~b_live(amp, freq, k, harmonic)] == 0.0)


def b_live(amp, freq, k, harmonic):
    return sm.frame_frequencies(freq, k, harmonic) < np.float32(8000.0)


def test_single_rounding_sum_resolves_double_rounding():
    # 1 + 2^-24 + 2^-60: the float64 sum is the float32 midpoint 1 + 2^-24 (ties-to-even: 1.0), the exact sum is above it
    p, q = np.array([1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]), np.array([2.0 ** -60, -2.0 ** -60, -2.0 ** -60])
    got = sm._round_sum_to_f32(p, q)
    assert got.tolist() == [float(np.float32(1.0 + 2.0 ** -23)), 1.0, float(np.float32(1.0 + 2.0 ** -23))]


def test_phase_ties_flags_sums_next_to_a_rounding_boundary_only():
    mid = 1000.0 + 2.0 ** -15                                               # float32 spacing at 1000 is 2^-14: an exact midpoint
    sums = np.array([[mid, mid * (1 + 2.0 ** -51), mid * (1 + 2.0 ** -40), 1000.0]]).T[None]      # [1, 4, 1]
    mask, alt = sm.phase_ties(sums, samples=4)
    assert mask[0, :, 0].tolist() == [True, True, False, False]
    assert alt[0, 0, 0] != sums.astype(np.float32)[0, 0, 0] and abs(float(alt[0, 0, 0]) - mid) == 2.0 ** -15


def test_a_column_with_inexact_sums_reports_its_ties_and_their_slack():
    """A first omega of ~1e-20 rad next to omegas of ~3 rad: the float64 sums are no longer exact in every association, so the tie mask is live.
    The tied elements carry the neighbouring float32 phase, and audio and grad_amp evaluated AT that phase are accepted."""
    rng = np.random.default_rng(5)
    freq = (30.0 + 7900.0 * rng.random((1, 4000, 256))).astype(np.float32)
    freq[:, 0, :] = 1e-16
    amp = rng.random(freq.shape).astype(np.float32)
    up = rng.standard_normal((1, 4000)).astype(np.float32)
    assert not sm.sums_are_exact(sm.omegas(freq, SR)).any()
    m = sm.oscillator_bank(freq, amp, SR)
    assert 0 < m.ties.sum() < 1000               # ~ samples * 2^-28 of the million elements
    ulp = np.abs(m.alt_phase.astype(np.float64) - m.phase.astype(np.float64))[m.ties]
    assert np.all(ulp == np.spacing(np.minimum(np.abs(m.alt_phase), np.abs(m.phase))[m.ties]).astype(np.float64))
    b = sm.oscillator_bank_backward(freq, amp, SR, up, fwd=m)
    other = np.where(m.ties, m.alt_phase, m.phase).astype(np.float64)
    audio = (m.amp * np.sin(other)).sum(-1)
    rows = m.ties.any(-1)
    assert np.all(m.slack[rows] > 0) and np.all(m.slack[~rows] == 0)
    moved = np.abs(audio - m.audio)
    assert moved[rows].max() > 0 and np.all(moved <= m.slack * (1 + 1e-9) + 1e-15) and sm.ratio(moved, sm.audio_bound(m, 256)) <= 1.0
    grad_amp = np.where(m.muted, 0.0, up[:, :, None] * np.sin(other))
    assert sm.grad_amp_ratio(grad_amp, b) == 0.0 and sm.ratio(grad_amp - b.grad_amp, sm.grad_amp_bound(b)) > 1.0    # only the other phase explains it
    dphi = up[:, :, None] * m.amp * np.cos(other)
    grad_freq = sm._suffix(dphi) * b.scale
    assert sm.ratio(grad_freq - b.grad_freq, sm.grad_freq_bound(b)) <= 1.0
