"""The synthesiser kernels of csrc/sot_osc.hip at every tile geometry, against the float64 model of tests/synth_model.py with its
per-element bounds.  pick_segment gives a segment length S in {8, 16, 32, 64, 128, 256, 512} from the sinusoid count K; every S is
launched at both ends of its K band, with clips of S - 3 (one partial segment), S, S + 1 (two segments), 3 S + 5 (several, the clip
ending inside a run of 8) and 9 S samples (the scans over more than a few segments).  Frequencies sit at, one float32 below and, within
one run of 8 samples, across Nyquist."""
import numpy as np
import pytest
import torch

import synth_model as sm

SR = sm.SR
SEGMENTS = (8, 16, 32, 64, 128, 256, 512)
BANDS = [(4, 512), (5, 256), (8, 256), (9, 128), (16, 128), (17, 64), (64, 64), (65, 32), (128, 32), (129, 16), (256, 16), (257, 8), (512, 8)]
BANK_CASES = [(1 + (i + j) % 3, n, k, s) for i, (k, s) in enumerate(BANDS) for j, n in enumerate((s - 3, s, s + 1, 3 * s + 5))]
BANK_CASES += [(3, 9 * s, k, s) for k, s in BANDS]
HOPS_FRAMES = [(hop, frames) for hop in ("2", "3", "S/2", "S", "2S+1") for frames in (1, 2, 5)]


def _hop(name, s):
    return {"2": 2, "3": 3, "S/2": s // 2, "S": s, "2S+1": 2 * s + 1}[name]


def _segment_of(lib, batch, samples, k):
    """S as sot_oscillator_bank_workspace_bytes implies it: two arrays of batch x ceil(samples / S) x K doubles, asked at a multiple of 512."""
    whole = 512 * -(-samples // 512)
    return whole * batch * k * 16 // int(lib.sot_oscillator_bank_workspace_bytes(batch, whole, k))


def test_the_parameter_list_reaches_every_segment_length():
    from sot_amd import _native as nat
    lib = nat.load()
    seen = set()
    for batch, samples, k, s in BANK_CASES:
        assert _segment_of(lib, batch, samples, k) == s, (batch, samples, k)
        seen.add(s)
    for k, s in BANDS:
        for name, frames in HOPS_FRAMES:
            for batch in (1, 2, 3):
                assert _segment_of(lib, batch, _hop(name, s) * frames, k) == s
    assert seen == set(SEGMENTS)
    assert {n // s for _, n, _, s in BANK_CASES} >= {0, 1, 3, 9} and {-(-n // s) for _, n, _, s in BANK_CASES} >= {1, 2, 4, 9}


def test_segment_length_depends_on_the_sinusoid_count_alone():
    """pick_segment's third loop (halve S > 64 while (S / 8) K >= 512 and the grid is small) cannot run: S > 64 after the second loop
    means S K <= 2048, so (S / 8) K <= 256.  Enumerated: S is the same for every batch / clip length."""
    from sot_amd import _native as nat
    lib = nat.load()
    for k in range(1, 513):
        want = 512
        while want > 8 and want * k > 4096:
            want //= 2
        while want > 64 and want * k > 2048:
            want //= 2
        assert {_segment_of(lib, batch, samples, k) for batch in (1, 7, 256, 4096) for samples in (512, 4096, 1 << 20)} == {want}, k


def _model_inputs():
    """Every input the GPU tests below use (bank cases, then synthesiser cases), with the float64 model of its forward."""
    for case in BANK_CASES:
        yield case, sm.oscillator_bank(*_bank_input(*case)[:2], SR)
    for k, s in BANDS:
        for harmonic in (False, True):
            for amp, freq, hann, samples, _ in _synth_inputs(k, s, harmonic):
                yield (k, s, harmonic, samples), sm.synth(amp, freq, hann, samples, SR, harmonic)


def test_the_inputs_sit_on_no_phase_tie():
    """The precondition of the comparisons: at most TIE_SHARE of an input's elements may accept a neighbouring phase (synth_model.py)."""
    muted = total = 0
    for case, m in _model_inputs():
        assert m.ties.mean() <= sm.TIE_SHARE, (case, int(m.ties.sum()))
        muted, total = muted + int(m.muted.sum()), total + m.muted.size
    assert 0.05 <= muted / total <= 0.3


def _bank_input(batch, samples, k, s):
    return sm.bank_inputs(1000 * k + samples, batch, samples, k)


def _synth_inputs(k, s, harmonic):
    for i, (name, frames) in enumerate(HOPS_FRAMES):
        hop, batch = _hop(name, s), 1 + i % 3
        samples = hop * frames
        amp, freq = sm.control_inputs(100000 * int(harmonic) + 1000 * k + samples, batch, frames, k, harmonic)
        grad = np.random.default_rng(samples + k).standard_normal((batch, samples)).astype(np.float32)
        yield amp, freq, torch.hann_window(2 * hop).numpy(), samples, grad


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("batch,samples,k,s", BANK_CASES)
def test_oscillator_bank_against_the_float64_model(batch, samples, k, s):
    from gpu_util import native
    nat = native()
    freq, amp, grad = _bank_input(batch, samples, k, s)
    m = sm.oscillator_bank(freq, amp, SR)
    assert m.ties.mean() <= sm.TIE_SHARE
    b = sm.oscillator_bank_backward(freq, amp, SR, grad, fwd=m)
    f, a, g = _dev(freq), _dev(amp), _dev(grad)
    audio, ws = nat.oscillator_bank_forward(f, a, SR, return_workspace=True)
    r_audio = sm.ratio(audio.cpu().numpy() - m.audio, sm.audio_bound(m, k))
    gf, ga = nat.oscillator_bank_backward(f, a, SR, g, forward_workspace=ws)
    r_amp = sm.grad_amp_ratio(ga.cpu().numpy(), b)
    r_freq = sm.ratio(gf.cpu().numpy() - b.grad_freq, sm.grad_freq_bound(b))
    print(f"error / bound: audio {r_audio:.3f} grad_amp {r_amp:.3f} grad_freq {r_freq:.3f}")
    assert r_audio <= 1.0 and r_amp <= 1.0 and r_freq <= 1.0, (r_audio, r_amp, r_freq)
    assert m.muted.any() and np.all(ga.cpu().numpy()[m.muted] == 0.0)
    # segment phases rebuilt instead of reused, and either gradient alone: the same bits
    gf2, ga2 = nat.oscillator_bank_backward(f, a, SR, g)
    assert torch.equal(gf2, gf) and torch.equal(ga2, ga)
    gf3, none = nat.oscillator_bank_backward(f, a, SR, g, need_amp=False)
    assert none is None and torch.equal(gf3, gf)
    none, ga3 = nat.oscillator_bank_backward(f, a, SR, g, need_freq=False)
    assert none is None and torch.equal(ga3, ga)


@pytest.mark.gpu
@pytest.mark.parametrize("harmonic", (False, True))
@pytest.mark.parametrize("k,s", BANDS)
def test_one_piece_synthesiser_against_the_float64_model(k, s, harmonic):
    """sot_synth_forward / _backward with hop in {2, 3, S / 2, S, 2 S + 1} and 1, 2, 5 frames (clips of 2 ... 10 S + 5 samples)."""
    from gpu_util import native
    from sot_amd import spectra
    nat = native()
    worst = [0.0, 0.0, 0.0]
    for amp, freq, hann, samples, grad in _synth_inputs(k, s, harmonic):
        what = (k, harmonic, amp.shape, samples)
        m = sm.synth(amp, freq, hann, samples, SR, harmonic)
        assert m.ties.mean() <= sm.TIE_SHARE, what
        b = sm.synth_backward(amp, freq, hann, samples, SR, harmonic, grad, fwd=m)
        a, f, w, g = _dev(amp), _dev(freq), _dev(hann), _dev(grad)
        audio, ws = nat.synth_forward(a, f, w, samples, SR, harmonic, for_backward=True)
        r_audio = sm.ratio(audio.cpu().numpy() - m.audio, sm.audio_bound(m, k))
        try:
            ga, gf = nat.synth_backward(a, f, w, samples, SR, harmonic, g, forward_workspace=ws)
        except nat.SotError as err:
            # The 160 KB LDS check of sot_synth_backward: the module function must still deliver the gradient.  No valid shape reaches it today
            # (hop >= 2 and S K <= 4096 keep the kernel's LDS below ~100 KB), so this branch only runs if that limit or the tiling changes.
            assert err.status == nat.SOT_ERR_UNSUPPORTED_SIZE, what
            a1, f1 = a.clone().requires_grad_(True), f.clone().requires_grad_(True)
            (spectra.sinusoidal_synth(a1, f1, samples, SR, harmonic=harmonic) * g).sum().backward()
            ga, gf = a1.grad, f1.grad
        else:
            ga2, gf2 = nat.synth_backward(a, f, w, samples, SR, harmonic, g)                     # segment phases rebuilt
            assert torch.equal(ga2, ga) and torch.equal(gf2, gf), what
            ga3, none = nat.synth_backward(a, f, w, samples, SR, harmonic, g, need_freq=False)
            assert none is None and torch.equal(ga3, ga), what
            none, gf3 = nat.synth_backward(a, f, w, samples, SR, harmonic, g, need_amp=False)
            assert none is None and torch.equal(gf3, gf), what
        assert ga.shape == b.grad_amp.shape and gf.shape == b.grad_freq.shape
        r_amp = sm.ratio(ga.cpu().numpy() - b.grad_amp, b.amp_bound)
        r_freq = sm.ratio(gf.cpu().numpy() - b.grad_freq, b.freq_bound)
        assert r_audio <= 1.0 and r_amp <= 1.0 and r_freq <= 1.0, (what, r_audio, r_amp, r_freq)
        worst = [max(x, y) for x, y in zip(worst, (r_audio, r_amp, r_freq))]
    print("error / bound: audio %.3f grad_amp %.3f grad_freq %.3f" % tuple(worst))
