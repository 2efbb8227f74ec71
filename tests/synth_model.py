"""Float64 model of the synthesiser kernels (csrc/sot_osc.hip; include/sot_hip.h: sot_oscillator_bank_*, sot_synth_envelopes_*,
sot_synth_forward / _backward) for the synthesiser tests, plain numpy.  The float32 values that FIX the result are formed exactly as
the kernels (and ATen's CPU kernels, and so the reference) form them; everything after them runs in float64:

    omega   = fp32( fp32(f * fp32(2 pi)) / sr )                       float32 arithmetic
    sums_t  = sum_{i <= t} omega_i                                    float64, sequential
    phase_t = fp32(sums_t)
    a'      = 0 where f >= sr / 2, else a                             (the muted sinusoid still advances its phase)
    audio_t = sum_k a'_{t,k} sin(phase_{t,k})                         float64
    grad_amp  = g sin(phase), 0 where muted;   dphi = g a' cos(phase);   grad_freq_t = (sum_{t' >= t} dphi_t') / sr * fp32(2 pi)

    envelopes from frame-rate controls (hop = samples / frames, w = the caller's float32 hann(2 hop)):
    s  = max(fp32(scale (t + 0.5) - 0.5), 0), scale = fp32(frames) / fp32(samples)      (one rounding: the kernel's fmaf)
    i0 = min(int(s), frames - 1), i1 = min(i0 + 1, frames - 1), l1 = clamp(s - i0, 0, 1), l0 = 1 - l1                float32
    freq_env = fmaf(l0, F[i0], fp32(l1 F[i1]))           F = f0 * (k + 1) (a float32 product) when harmonic
    amp_env  = fp32(fp32(A'[a] w[u + hop]) + fp32(A'[min(a + 1, frames - 1)] w[u])),   t = a hop + u,  A' = 0 where F >= sr / 2
    and the backward is the transpose of these two linear maps (muted frames get no amplitude gradient; d f0 = sum_k (k + 1) d F_k).

Phase ties.  The kernels add the same omegas in float64 in another association (runs of 8, segment totals, a scan over segments); their sum
differs from the sequential one by at most samples * 2^-53 * sum in either direction, and on the rare element whose sum lies that close to
a float32 rounding boundary the kernel's phase may be the neighbouring float32.  `oscillator_bank` reports those elements (`ties`) with the
neighbouring phase (`alt_phase`), and the bounds below accept either phase there.  The tests cap the share of such elements at TIE_SHARE.
Where a sinusoid's omegas are all multiples of one quantum q with sum |omega| < 2^53 q (float32 omegas of similar size over a few thousand
samples: nearly every input) every partial sum is exact in any association, the kernel's sum IS the sequential one, and nothing is flagged.

Error bounds, per element (eps = 2^-24, A_t = sum_k |a'_{t,k}|, u = U_SIN):
    audio      (K - 1 + u + 1) eps A_t                   float32 sum over K, the product's rounding, the device sinf
    grad_amp   (u + 1) eps |g_t|
    grad_freq  (2 pi / sr) [(u + 3) eps sum_{t' >= t} |dphi_t'| + 3 eps |sum_{t' >= t} dphi_t'|]
    frame-rate gradients of the one-piece backward: the same terms through the transposed interpolation, + 2 eps relative (amplitudes)
    frame-rate gradients of sot_synth_envelopes_backward alone (float32 gradient envelopes in): eps sum |g weight| (one float32 product
    per term, float64 accumulation) + eps |result| (the final rounding).

U_SIN: the error of the device's sinf / sincosf in ulp of the result.  |sin|, |cos| <= 1, so one ulp is at most eps and u ulp bound the
absolute error by u eps -- the unit u has in every bound above.  ROCm ships no accuracy table for them in its documentation tree, so it was
measured on an MI355X with tools/sinf_accuracy.hip (a stand-alone HIP program compiled with the library's flags): sinf and sincosf on 2^25
float32 arguments (a uniform grid over [0, 1.3e5] rad -- the sweeps' phases stay below 2.2e4 -- and random bit patterns from 2^-10 to
2^17) against the host's float64 sin / cos.  Worst error: sinf 1.61 ulp, sincosf's sine 1.61 ulp, its cosine 1.58 ulp (below 2.2e4 rad:
1.58 / 1.58 / 1.58).  MEASURED_SIN_ULP is the worst of them, U_SIN twice it.
"""
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -24
MEASURED_SIN_ULP = 1.61    # measured: see above
U_SIN = 2.0 * MEASURED_SIN_ULP
TIE_SHARE = 1e-4           # most elements of one input that may sit on a phase tie
TWO_PI_F32 = np.float32(6.283185307179586)
F32, F64 = np.float32, np.float64


def _f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def _round_sum_to_f32(p, q):
    """fp32(p + q) with ONE rounding for float64 p, q (an fma's tail): the float64 sum, and where that sum is inexact and sits exactly on
    a float32 rounding boundary, the side the lost part points to."""
    shape = np.broadcast(p, q).shape
    p, q = np.broadcast_to(p, shape).ravel(), np.broadcast_to(q, shape).ravel()
    s = p + q
    bb = s - p
    err = (p - (s - bb)) + (q - bb)                       # TwoSum: p + q = s + err exactly
    r = s.astype(F32)
    for i in np.nonzero((err != 0.0) & (r.astype(F64) != s))[0]:
        for side in (np.nextafter(r[i], F32(np.inf)), np.nextafter(r[i], F32(-np.inf))):
            if s[i] == 0.5 * (F64(r[i]) + F64(side)) and (err[i] > 0) == (side > r[i]):
                r[i] = side                               # ties-to-even kept r, the exact sum is past the midpoint
                break
    return r.reshape(shape)


def omegas(freq, sr):
    return (_f32(freq) * TWO_PI_F32) / F32(sr)


def sums_are_exact(omega):
    """[batch, K]: True where every partial sum of the column's omegas, in ANY association, is exact in float64 -- all of them are multiples of
    the smallest omega's last bit q, and sum |omega| < 2^53 q.  No reassociation error, so no phase tie, exists there."""
    mag = np.abs(omega.astype(F64))
    smallest = np.where(mag > 0, mag, np.inf).min(axis=1)
    _, e = np.frexp(np.where(np.isfinite(smallest), smallest, 1.0))
    q = np.maximum(np.ldexp(1.0, e - 24), 2.0 ** -149)
    return mag.sum(axis=1) < 2.0 ** 53 * q


def phase_ties(sums, samples, exact=None):
    """(mask, alt_phase): elements whose float64 sum lies within samples * 2^-52 * |sum| of a float32 rounding boundary -- except in columns
    whose sums are exact in every association (sums_are_exact) -- and the float32 on the other side of that boundary."""
    ph = sums.astype(F32)
    p64 = ph.astype(F64)
    up, down = np.nextafter(ph, F32(np.inf)), np.nextafter(ph, F32(-np.inf))
    d_up, d_down = np.abs(sums - 0.5 * (p64 + up.astype(F64))), np.abs(sums - 0.5 * (p64 + down.astype(F64)))
    tol = samples * 2.0 ** -52 * np.abs(sums)
    mask = (np.minimum(d_up, d_down) <= tol) & (sums != 0.0)
    if exact is not None:
        mask &= ~exact[:, None, :]
    return mask, np.where(d_up <= d_down, up, down)


def oscillator_bank(freq, amp, sr):
    """freq, amp [batch, samples, K] -> audio [batch, samples] (float64), phase (float32), sums (float64), abs_amp = sum_k |a'| per sample,
    muted, ties / alt_phase (phase_ties) and slack = what the audio may move by if tied elements take their other phase."""
    freq, amp = _f32(freq), _f32(amp)
    omega = omegas(freq, sr)
    sums = np.cumsum(omega.astype(F64), axis=1)
    phase = sums.astype(F32)
    muted = freq >= F32(sr) / F32(2.0)
    a = np.where(muted, 0.0, amp.astype(F64))
    ties, alt = phase_ties(sums, freq.shape[1], sums_are_exact(omega))
    sin = np.sin(phase.astype(F64))
    slack = (ties * np.abs(a) * np.abs(np.sin(alt.astype(F64)) - sin)).sum(-1)
    return SimpleNamespace(audio=(a * sin).sum(-1), phase=phase, sums=sums, abs_amp=np.abs(a).sum(-1), muted=muted, amp=a, ties=ties,
                           alt_phase=alt, slack=slack)


def _suffix(x):
    return np.flip(np.cumsum(np.flip(x, 1), axis=1), 1)


def oscillator_bank_backward(freq, amp, sr, grad_audio, fwd=None):
    """grad_freq, grad_amp [batch, samples, K] (float64), dphi, the suffix sums abs_suffix = sum_{t' >= t} |dphi| and suffix = sum_{t' >= t}
    dphi, and for tied elements grad_amp_alt plus the slack of the dphi suffix sums."""
    m = fwd if fwd is not None else oscillator_bank(freq, amp, sr)
    g = np.asarray(grad_audio, F64)[:, :, None]
    ph = m.phase.astype(F64)
    sin, cos = np.sin(ph), np.cos(ph)
    grad_amp = np.where(m.muted, 0.0, g * sin)
    dphi = g * m.amp * cos
    suffix, abs_suffix = _suffix(dphi), _suffix(np.abs(dphi))
    out = float(TWO_PI_F32) / float(F32(sr))
    alt = m.alt_phase.astype(F64)
    grad_amp_alt = np.where(m.ties & ~m.muted, g * np.sin(alt), grad_amp)
    tie_slack = _suffix(m.ties * np.abs(g * m.amp * np.cos(alt) - dphi))
    return SimpleNamespace(grad_freq=suffix * out, grad_amp=grad_amp, dphi=dphi, suffix=suffix, abs_suffix=abs_suffix, scale=out,
                           grad_amp_alt=grad_amp_alt, tie_slack=tie_slack, g=np.abs(g))


def audio_bound(m, K):
    return (K - 1 + U_SIN + 1) * EPS * m.abs_amp + m.slack


def grad_amp_bound(b):
    return (U_SIN + 1) * EPS * np.broadcast_to(b.g, b.grad_amp.shape)


def grad_freq_bound(b):
    return b.scale * ((U_SIN + 3) * EPS * b.abs_suffix + 3 * EPS * np.abs(b.suffix) + b.tie_slack)


def ratio(err, bound):
    """Largest err / bound over the elements; an element with bound 0 must be exact."""
    err, bound = np.abs(np.asarray(err, F64)), np.asarray(bound, F64)
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max())


def grad_amp_ratio(got, b):
    got = np.asarray(got, F64)
    err = np.minimum(np.abs(got - b.grad_amp), np.abs(got - b.grad_amp_alt))
    return ratio(err, grad_amp_bound(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# envelopes
# ---------------------------------------------------------------------------------------------------------------------------------
def linear_taps(frames, samples):
    """i0, i1 (int), l0, l1 (float32) of every sample, as the kernel's linear_taps forms them."""
    scale = F32(frames) / F32(samples)
    t = np.arange(samples, dtype=F64)
    s = (F64(scale) * (t + 0.5) - 0.5).astype(F32)        # exact in float64 wherever it is not negative: one rounding, the fmaf
    s = np.where(s < 0, F32(0.0), s).astype(F32)
    i0 = np.minimum(s.astype(np.int64), frames - 1)
    i1 = np.minimum(i0 + 1, frames - 1)
    l1 = np.clip(s - i0.astype(F32), F32(0.0), F32(1.0)).astype(F32)
    return i0, i1, (F32(1.0) - l1).astype(F32), l1


def frame_frequencies(freq_frames, K, harmonic):
    freq_frames = _f32(freq_frames)
    return freq_frames * np.arange(1, K + 1, dtype=F32) if harmonic else freq_frames


def envelopes(amp_frames, freq_frames, window, samples, sr, harmonic):
    """amp_frames [batch, frames, K], freq_frames [batch, frames, K or 1], window [2 hop] float32 -> (amp_env, freq_env) float32."""
    amp_frames, window = _f32(amp_frames), _f32(window)
    batch, frames, K = amp_frames.shape
    hop = samples // frames
    assert hop * frames == samples and frames < samples and window.shape == (2 * hop,)
    F = frame_frequencies(freq_frames, K, harmonic)
    i0, i1, l0, l1 = linear_taps(frames, samples)
    tail = l1[None, :, None] * F[:, i1, :]                                            # float32 product
    freq_env = _round_sum_to_f32(l0.astype(F64)[None, :, None] * F[:, i0, :].astype(F64), tail.astype(F64))
    A = np.where(F >= F32(sr) / F32(2.0), F32(0.0), amp_frames)
    held = np.concatenate([A, A[:, -1:, :]], axis=1)
    lead = held[:, :-1, None, :] * window[None, None, hop:, None]
    follow = held[:, 1:, None, :] * window[None, None, :hop, None]
    return (lead + follow).reshape(batch, samples, K), freq_env


def _amp_transpose(x, window, frames):
    """[batch, samples, K] -> [batch, frames, K]: the transposed window upsampling (the held last frame collects both halves)."""
    batch, samples, K = x.shape
    hop = samples // frames
    w = window.astype(F64)
    x = x.reshape(batch, frames, hop, K)
    lead = np.einsum("bfuk,u->bfk", x, w[hop:])
    follow = np.einsum("bfuk,u->bfk", x, w[:hop])
    out = lead
    out[:, 1:] += follow[:, :-1]
    out[:, -1] += follow[:, -1]
    return out


def _freq_transpose(x, frames):
    batch, samples, K = x.shape
    i0, i1, l0, l1 = linear_taps(frames, samples)
    out = np.zeros((frames, batch, K))
    xt = x.transpose(1, 0, 2)
    np.add.at(out, i0, xt * l0.astype(F64)[:, None, None])
    np.add.at(out, i1, xt * l1.astype(F64)[:, None, None])
    return out.transpose(1, 0, 2)


def _to_f0(x, harmonic):
    return (x * np.arange(1, x.shape[-1] + 1, dtype=F64)).sum(-1, keepdims=True) if harmonic else x


def envelopes_backward(amp_frames, freq_frames, window, samples, sr, harmonic, grad_amp_env, grad_freq_env):
    """Transposed upsampling of float gradient envelopes [batch, samples, K] (either may be None): grad_amp, grad_freq of the frame-rate
    controls in float64, and the bounds for a kernel that takes the float32 products and adds them up in float64."""
    amp_frames, window = _f32(amp_frames), _f32(window)
    batch, frames, K = amp_frames.shape
    live = frame_frequencies(freq_frames, K, harmonic) < F32(sr) / F32(2.0)
    out = SimpleNamespace(grad_amp=None, grad_freq=None, amp_bound=None, freq_bound=None, live=live)
    if grad_amp_env is not None:
        g = np.asarray(grad_amp_env, F64)
        out.grad_amp = np.where(live, _amp_transpose(g, window, frames), 0.0)
        out.amp_bound = np.where(live, EPS * _amp_transpose(np.abs(g), window, frames) + EPS * np.abs(out.grad_amp), 0.0)
    if grad_freq_env is not None:
        g = np.asarray(grad_freq_env, F64)
        out.grad_freq = _to_f0(_freq_transpose(g, frames), harmonic)
        out.freq_bound = _to_f0(EPS * _freq_transpose(np.abs(g), frames), harmonic) + EPS * np.abs(out.grad_freq)
    return out


def synth(amp_frames, freq_frames, window, samples, sr, harmonic):
    """Frame-rate controls -> the oscillator_bank result of their envelopes (plus amp_env / freq_env)."""
    amp_env, freq_env = envelopes(amp_frames, freq_frames, window, samples, sr, harmonic)
    m = oscillator_bank(freq_env, amp_env, sr)
    m.amp_env, m.freq_env = amp_env, freq_env
    return m


def synth_backward(amp_frames, freq_frames, window, samples, sr, harmonic, grad_audio, fwd=None):
    """grad_amp [batch, frames, K], grad_freq [batch, frames, K or 1] in float64 with their per-element bounds for the one-piece kernels."""
    m = fwd if fwd is not None else synth(amp_frames, freq_frames, window, samples, sr, harmonic)
    window = _f32(window)
    frames = np.shape(amp_frames)[1]
    b = oscillator_bank_backward(m.freq_env, m.amp_env, sr, grad_audio, fwd=m)
    env = envelopes_backward(amp_frames, freq_frames, window, samples, sr, harmonic, b.grad_amp, b.grad_freq)
    push = np.where(m.muted, 0.0, (U_SIN + 1) * EPS * b.g) + 2 * EPS * np.abs(b.grad_amp) + np.abs(b.grad_amp_alt - b.grad_amp)
    amp_bound = np.where(env.live, _amp_transpose(push, window, frames), 0.0)
    freq_bound = _to_f0(_freq_transpose(grad_freq_bound(b), frames), harmonic)
    return SimpleNamespace(grad_amp=env.grad_amp, grad_freq=env.grad_freq, amp_bound=amp_bound, freq_bound=freq_bound, bank=b)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs shared by the tests and tools/fuzz_synth.py (sample rate 16 kHz: Nyquist = 8000.0, exact in float32)
# ---------------------------------------------------------------------------------------------------------------------------------
SR = 16000.0
NYQ = F32(8000.0)
BELOW_NYQ = np.nextafter(NYQ, F32(0.0))


def _with_nyquist_entries(rng, freq):
    """A few entries exactly at Nyquist (muted: the test is >=) and one float32 below it (sounding)."""
    flat = freq.reshape(-1)
    n = min(3, flat.size // 2)
    picks = rng.choice(flat.size, size=2 * n, replace=False)
    flat[picks[:n]] = NYQ
    flat[picks[n:]] = BELOW_NYQ
    return freq


def bank_inputs(seed, batch, samples, K):
    """freq, amp [batch, samples, K] and grad_audio [batch, samples], float32: frequencies uniform in [30, 9030) Hz (one in nine muted),
    entries at and just below Nyquist, and -- last sinusoid of clip 0 -- a ramp through Nyquist inside one run of 8 samples."""
    rng = np.random.default_rng(seed)
    freq = (30.0 + 9000.0 * rng.random((batch, samples, K))).astype(F32)
    amp = rng.random((batch, samples, K)).astype(F32)
    grad = rng.standard_normal((batch, samples)).astype(F32)
    _with_nyquist_entries(rng, freq)
    r0 = 8 * (samples // 16)
    n = min(8, samples - r0)
    freq[0, r0:r0 + n, K - 1] = np.linspace(7990.0, 8010.0, 8, dtype=F32)[:n]
    return freq, amp, grad


def control_inputs(seed, batch, frames, K, harmonic):
    """amp_frames [batch, frames, K], freq_frames [batch, frames, K or 1], float32.  Harmonic: the top partial lies between 0.5 and 1.5
    times Nyquist, frame by frame, so some partials are above Nyquist in some frames only."""
    rng = np.random.default_rng(seed)
    amp = rng.random((batch, frames, K)).astype(F32)
    if harmonic:
        freq = ((4000.0 + 8000.0 * rng.random((batch, frames, 1))) / max(K, 2)).astype(F32)
    else:
        freq = _with_nyquist_entries(rng, (30.0 + 9000.0 * rng.random((batch, frames, K))).astype(F32))
    return amp, freq
