"""Producers of the hot path's inputs for BASELINE config 5 (the training-step slice): a harmonic batch
generator and the magnitude STFT that `trainer.py:199-200` applies before the loss.

The magnitude STFT runs hand-written HIP kernels on the GPU (`csrc/sot_stft.hip` and its `csrc/sot_stft_*.hpp` kernel families behind
`sot_stft_mag_forward` / `sot_stft_mag_backward`: in-LDS FFT per frame, closed-form backward with an in-LDS
overlap-add per clip); `stft_magnitude_torch` is the same transform on torch ops (torch.stft -> rocFFT / pocketfft),
kept for CPU tensors, for transform sizes the kernels do not cover and as a cross-check.  The harmonic generator is
torch plumbing.  Mirrors, without copying, the behaviour of
  * features.TorchSTFT / compute_mag / stft (features.py:85-113, 191-237): window from scipy.signal.get_window,
    `normalized=True`, `center=False`, end-padding so that every sample is covered (utils.pad_for_stft,
    utils.py:252-275), magnitude, output [batch, frames, bins];
  * synthetic_data.SimpleSinusoidDataset (synthetic_data.py:76-118, 174-201, 232-237; settings :331-345): f0 ~ U[40,1950] Hz,
    8 harmonic partials with amplitudes ~ U[0.4,1] of which the first max(1, n_active) sound, the frame-rate controls go
    through synths.Sinusoidal (synths.py:43-128: Hann-window / linear upsampling, oscillator bank), 4096 samples @ 16 kHz,
    every item divided by its peak + 1e-7 and scaled to 0.9 -- pinned by tests/golden/synth_generator.npz.
"""
from __future__ import annotations

import torch

_compiling = torch.compiler.is_compiling


def _traced_ops():
    """The sot_amd:: custom ops (ops.py): the GPU route of a call that torch.compile / torch.export is tracing.  Eager calls never ask."""
    from . import ops  # noqa: F401 -- registers them
    return torch.ops.sot_amd


def _window_name(window) -> str:
    return "" if window is None else str(window)


def end_padded(signal: torch.Tensor, frame_size: int, hop: int) -> torch.Tensor:
    """Pad so that the window slides until it is completely beyond the signal (tf.stft(pad_end=True) semantics)."""
    length = signal.shape[1]
    frames = -(-length // hop)
    missing = max(0, frame_size + hop * (frames - 1) - length)
    return signal if missing == 0 else torch.nn.functional.pad(signal, (0, missing))


def analysis_window(name, n_fft: int, device) -> torch.Tensor:
    if name is None:
        return torch.hann_window(n_fft, device=device)
    from scipy.signal import get_window
    return torch.as_tensor(get_window(name, n_fft), dtype=torch.float32, device=device)


class _DeviceTableCache:
    """Process-wide cache of small device tables (analysis windows, Hann upsampling windows, synthesiser tap tables).  A table
    is produced by work enqueued on the stream that first asks for it; like nat.PositionPlan it therefore carries a ready
    event that other streams wait on, and it is never CREATED while a stream capture is in progress (an H2D copy would
    invalidate the capture, and memory from a graph's private pool must not outlive it): a capture that needs a missing
    table gets it uncached when device work alone builds it (built by captured work, owned by that graph's replay) and an
    error when host data would have to be copied."""

    def __init__(self):
        self.entries = {}

    def get(self, key, device, make, host_side=False):
        """host_side: `make` copies host data to the device (cannot happen inside a capture: the caller must have used the
        table once outside it, as any warm-up step does).  A table is always an ordinary tensor, also when the first caller runs under
        torch.inference_mode() (the evaluation metrics do): an inference tensor in the cache could not be saved for backward by the
        training step that asks for the same table later."""
        with torch.inference_mode(False):
            return self._get(key, device, make, host_side)

    def _get(self, key, device, make, host_side):
        hit = self.entries.get(key)
        if hit is not None:
            table, ready, stream = hit
            if ready is not None:
                from . import _native as nat
                if nat.stream_ptr(table.device) != stream:
                    torch.cuda.current_stream(table.device).wait_event(ready)
            return table
        dev = torch.device(device)
        if dev.type != "cuda":
            table = make()
            self.entries[key] = (table, None, None)
            return table
        if torch.cuda.is_current_stream_capturing():
            if host_side:
                raise RuntimeError(f"sot_amd: table {key} is built from host data and is not cached yet; run the step once outside "
                                   "the stream capture first")
            return make()   # not cached: see the class docstring
        from . import _native as nat
        table = make()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(table.device))
        self.entries[key] = (table, ready, nat.stream_ptr(table.device))
        return table


_WINDOWS = _DeviceTableCache()


def _cached_window(name, n_fft: int, device) -> torch.Tensor:
    return _WINDOWS.get((str(name), int(n_fft), str(device)), device, lambda: analysis_window(name, n_fft, device), host_side=True)


_WINDOW_LISTS = {}


def _cached_windows(name, sizes, device):
    """The windows of several transform sizes as a list, cached per (sizes, device, STREAM): the first call on a stream goes through
    _cached_window (which makes that stream wait for a table another stream built), later calls on it are one dictionary lookup
    (MSSLoss asked for its six windows one by one on every call: ~20 us of host time per training step)."""
    from . import _native as nat
    key = (name, sizes, device.index, nat.stream_ptr(device))
    hit = _WINDOW_LISTS.get(key)
    if hit is None:
        hit = [_cached_window(name, size, device) for size in sizes]
        if not torch.cuda.is_current_stream_capturing():
            _WINDOW_LISTS[key] = hit
    return hit


SAVE_SPECTRUM = True   # module switch (tests compare both forms): differentiated forwards also store the complex spectrum


class _StftMagnitude(torch.autograd.Function):
    """sot_stft_mag_forward / sot_stft_mag_backward (include/sot_hip.h)."""

    @staticmethod
    def forward(ctx, audio, window, n_fft, hop):
        from . import _native as nat
        audio = audio.contiguous()
        ctx.n_fft, ctx.hop = n_fft, hop
        if ctx.needs_input_grad[0] and SAVE_SPECTRUM:   # keep the complex spectrum (what abs o stft's autograd saves): no recompute in backward
            mag, spec = nat.stft_mag_forward(audio, window, n_fft, hop, want_spec=True)
            ctx.save_for_backward(audio, window, spec)
            return mag
        ctx.save_for_backward(audio, window)
        return nat.stft_mag_forward(audio, window, n_fft, hop)

    @staticmethod
    def backward(ctx, grad_mag):
        from . import _native as nat
        audio, window, *spec = ctx.saved_tensors
        grad_audio = None
        if ctx.needs_input_grad[0]:
            grad_audio = nat.stft_mag_backward(audio, window, ctx.n_fft, ctx.hop, grad_mag.float(), spec=spec[0] if spec else None)
        return grad_audio, None, None, None


def hip_stft_supported(n_fft: int, hop: int, samples: int) -> bool:
    """Sizes the HIP kernels cover: n_fft a power of two in [64, 4096] (a group of frames must fit LDS in the backward)."""
    return 64 <= n_fft <= 4096 and (n_fft & (n_fft - 1)) == 0 and samples >= 1 and 1 <= hop and n_fft + 3 * hop <= 8192


def stft_magnitude(audio: torch.Tensor, n_fft: int = 2048, hop: int = 256, window="flattop") -> torch.Tensor:
    """[batch, samples] -> contiguous [batch, frames, n_fft/2+1] magnitudes, as the reference's TorchSTFT
    (features.py:85-113).  GPU tensors run the HIP kernels (differentiable w.r.t. the audio); CPU tensors and sizes
    outside hip_stft_supported() run torch.stft."""
    if audio.is_cuda and audio.ndim == 2 and hip_stft_supported(n_fft, hop, audio.shape[1]):
        if _compiling():
            want_spec = SAVE_SPECTRUM and torch.is_grad_enabled() and audio.requires_grad
            return _traced_ops().stft_magnitude(audio.float(), _window_name(window), int(n_fft), int(hop), want_spec)[0]
        if audio.dtype == torch.float32 and SAVE_SPECTRUM:
            from . import _native as nat
            glue = nat.glue()
            if glue is not None:   # the same kernels behind ONE C++ call and a C++ autograd node (csrc/sot_torch_glue.cpp)
                return glue.stft_magnitude(audio.contiguous(), _cached_window(window, n_fft, audio.device), int(n_fft), int(hop))
        return _StftMagnitude.apply(audio.float(), _cached_window(window, n_fft, audio.device), int(n_fft), int(hop))
    if audio.is_cuda:   # not silent: a GPU tensor that leaves the HIP path says so, once per size
        from .losses import warn_once
        warn_once(("stft", int(n_fft), int(hop), audio.ndim), f"stft_magnitude: n_fft={n_fft}, hop={hop}, audio.ndim={audio.ndim} is outside what "
                  "the HIP STFT kernels take (2-D audio, n_fft a power of two in [64, 4096]); running torch.stft (rocFFT) instead")
    return stft_magnitude_torch(audio, n_fft, hop, window)


def stft_magnitude_torch(audio: torch.Tensor, n_fft: int = 2048, hop: int = 256, window="flattop") -> torch.Tensor:
    """The same transform on torch ops (torch.stft)."""
    audio = end_padded(audio.float(), n_fft, hop)
    spec = torch.stft(audio, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=analysis_window(window, n_fft, audio.device),
                      center=False, normalized=True, return_complex=True)
    return spec.abs().permute(0, 2, 1).contiguous()


def unit_frequencies(n_fft: int, sample_rate: float, device) -> torch.Tensor:
    """rfftfreq / max: the support positions trainer.py:192-197 passes as x_pos (y_pos = clone)."""
    f = torch.fft.rfftfreq(n_fft, d=1.0 / sample_rate)
    return (f / f.max()).float().to(device)


class _OscillatorBank(torch.autograd.Function):
    """sot_oscillator_bank_forward / _backward (include/sot_hip.h)."""

    @staticmethod
    def forward(ctx, freq, amp, sample_rate):
        from . import _native as nat
        freq, amp = freq.contiguous(), amp.contiguous()
        audio, ws = nat.oscillator_bank_forward(freq, amp, sample_rate, return_workspace=True)
        ctx.save_for_backward(freq, amp, ws)   # ws: the segment start phases, reused by the backward
        ctx.sample_rate = sample_rate
        return audio

    @staticmethod
    def backward(ctx, grad_audio):
        from . import _native as nat
        freq, amp, ws = ctx.saved_tensors
        gf, ga = nat.oscillator_bank_backward(freq, amp, ctx.sample_rate, grad_audio.float(), need_freq=ctx.needs_input_grad[0],
                                              need_amp=ctx.needs_input_grad[1], forward_workspace=ws)
        return gf, ga, None


def oscillator_bank(frequency_envelopes: torch.Tensor, amplitude_envelopes: torch.Tensor, sample_rate: int = 16000) -> torch.Tensor:
    """The reference's ddsp.oscillator_bank (ddsp.py:208-263; sum_sinusoids=True, use_angular_cumsum=False): sample-wise
    frequencies (Hz) and amplitudes [batch, samples, sinusoids] -> audio [batch, samples]; sinusoids at or above Nyquist are
    muted.  GPU tensors run the HIP kernels (differentiable w.r.t. both envelopes), CPU tensors torch ops."""
    f, a = frequency_envelopes.float(), amplitude_envelopes.float()
    if f.is_cuda and f.ndim == 3 and f.shape == a.shape and 1 <= f.shape[1] <= (1 << 20) and 1 <= f.shape[2] <= 512:
        if _compiling():
            return _traced_ops().oscillator_bank(f, a, float(sample_rate))
        return _OscillatorBank.apply(f, a, float(sample_rate))
    a = torch.where(f >= sample_rate / 2.0, torch.zeros_like(a), a)
    phases = torch.cumsum(f * (2.0 * torch.pi) / float(sample_rate), dim=1)
    return torch.sum(a * torch.sin(phases), dim=-1)


def upsample_window(frames: torch.Tensor, n_samples: int) -> torch.Tensor:
    """[batch, n_frames, channels] -> [batch, n_samples, channels] with half-overlapping Hann windows: the reference's
    amplitude upsampler (`ddsp.resample(method="window", add_endpoint=True)` -> `upsample_with_windows`, ddsp.py:121-205, used
    by synths.py:95-102).  The last frame is held for one more step, n_samples must be a multiple of n_frames; with
    hop = n_samples / n_frames and w = hann(2 hop), sample t = a hop + u receives frames[a] w[u + hop] + frames[a + 1] w[u]
    (two products, one sum -- what the reference's fold() adds up; bit-identical on the same device type)."""
    frames = frames.float()
    batch, n_frames, channels = frames.shape
    if n_frames >= n_samples:
        raise ValueError(f"Upsample with windows cannot be used for downsampling: {n_frames} frames, {n_samples} timesteps")
    if n_samples % n_frames != 0:
        raise ValueError(f"the target number of timesteps ({n_samples}) must be divisible by the number of frames ({n_frames})")
    hop = n_samples // n_frames
    held = torch.cat([frames, frames[:, -1:, :]], dim=1)                       # add_endpoint
    w = torch.hann_window(2 * hop, device=frames.device)
    lead = (held[:, :-1, None, :] * w[None, None, hop:, None])                 # frames[a]     * w[u + hop]
    follow = (held[:, 1:, None, :] * w[None, None, :hop, None])                # frames[a + 1] * w[u]
    return (lead + follow).reshape(batch, n_samples, channels)


def upsample_linear(frames: torch.Tensor, n_samples: int) -> torch.Tensor:
    """[batch, n_frames, channels] -> [batch, n_samples, channels]: the reference's frequency upsampler
    (`ddsp.resample(method="bilinear", add_endpoint=True)`, ddsp.py:53-118 -> F.interpolate(align_corners=False))."""
    # the 1-D form of the same interpolation (bit-identical to the reference's bilinear call on a one-column image on the CPU;
    # on the GPU torch's kernel for the tall one-column image takes ~0.4 ms for 256 x 8 envelopes of 4096 samples)
    y = torch.nn.functional.interpolate(frames.float().permute(0, 2, 1), size=n_samples, mode="linear", align_corners=False)
    return y.permute(0, 2, 1).contiguous()


_HANN = _DeviceTableCache()


def _hann_on(device, hop: int) -> torch.Tensor:
    """torch.hann_window(2 hop) as the CPU computes it (the reference's dataset is synthesised on the CPU), resident on `device`."""
    return _HANN.get((str(device), hop), device, lambda: torch.hann_window(2 * hop).to(device), host_side=True)


_TAPS = _DeviceTableCache()


def _tap_tables_on(window: torch.Tensor, frames: int, n_samples: int) -> torch.Tensor:
    """The synthesiser backward's weight tables for this frame / sample count (they depend on nothing else), built once per device."""
    from . import _native as nat
    return _TAPS.get((str(window.device), frames, n_samples), window.device, lambda: nat.synth_tap_tables(window, frames, n_samples))


def _envelope_kernels_apply(amplitudes, frequencies, n_samples, harmonic) -> bool:
    if amplitudes.ndim != 3 or frequencies.ndim != 3:
        return False
    batch, frames, k = amplitudes.shape
    want = (batch, frames, 1) if harmonic else (batch, frames, k)
    return (tuple(frequencies.shape) == want and 1 <= frames < n_samples <= (1 << 20) and n_samples % frames == 0 and 1 <= k <= 512
            and batch >= 1)


class _SynthEnvelopes(torch.autograd.Function):
    """sot_synth_envelopes_forward / _backward (include/sot_hip.h): harmonic frequencies, Nyquist mask, window and linear
    upsampling of synths.Sinusoidal.get_controls / get_signal in one kernel each way."""

    @staticmethod
    def forward(ctx, frequencies, amplitudes, n_samples, sample_rate, harmonic):
        from . import _native as nat
        frequencies, amplitudes = frequencies.contiguous(), amplitudes.contiguous()
        window = _hann_on(amplitudes.device, n_samples // amplitudes.shape[1])
        amp_env, freq_env = nat.synth_envelopes_forward(amplitudes, frequencies, window, n_samples, sample_rate, harmonic)
        ctx.save_for_backward(frequencies, amplitudes, window)
        ctx.cfg = (n_samples, sample_rate, harmonic)
        return freq_env, amp_env

    @staticmethod
    def backward(ctx, grad_freq_env, grad_amp_env):
        from . import _native as nat
        frequencies, amplitudes, window = ctx.saved_tensors
        n_samples, sample_rate, harmonic = ctx.cfg
        need_f, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ga, gf = nat.synth_envelopes_backward(amplitudes, frequencies, window, n_samples, sample_rate, harmonic,
                                              grad_amp_env.float() if need_a else None, grad_freq_env.float() if need_f else None,
                                              need_amp=need_a, need_freq=need_f)
        return gf, ga, None, None, None


FUSED_SYNTH = True   # controls -> audio without sample-rate envelopes in memory (sot_synth_*); False: envelope kernels + bank


class _Synth(torch.autograd.Function):
    """sot_synth_forward / _backward (include/sot_hip.h): the oscillator-bank kernels evaluating the envelopes from the
    frame-rate controls on the fly; same audio, bit for bit, as _SynthEnvelopes followed by _OscillatorBank."""

    @staticmethod
    def forward(ctx, frequencies, amplitudes, n_samples, sample_rate, harmonic):
        from . import _native as nat
        frequencies, amplitudes = frequencies.contiguous(), amplitudes.contiguous()
        window = _hann_on(amplitudes.device, n_samples // amplitudes.shape[1])
        want_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        audio, ws = nat.synth_forward(amplitudes, frequencies, window, n_samples, sample_rate, harmonic, for_backward=want_grad)
        ctx.save_for_backward(frequencies, amplitudes, window, ws)
        ctx.cfg = (n_samples, sample_rate, harmonic)
        return audio

    @staticmethod
    def backward(ctx, grad_audio):
        from . import _native as nat
        frequencies, amplitudes, window, ws = ctx.saved_tensors
        n_samples, sample_rate, harmonic = ctx.cfg
        ga, gf = nat.synth_backward(amplitudes, frequencies, window, n_samples, sample_rate, harmonic, grad_audio.float(),
                                    need_amp=ctx.needs_input_grad[1], need_freq=ctx.needs_input_grad[0], forward_workspace=ws,
                                    tap_tables=_tap_tables_on(window, amplitudes.shape[1], n_samples))
        return gf, ga, None, None, None


def sinusoidal_synth(amplitudes: torch.Tensor, frequencies: torch.Tensor, n_samples: int, sample_rate: int = 16000,
                     harmonic: bool = True, apply_roll_off: bool = False) -> torch.Tensor:
    """The reference's `synths.Sinusoidal(amp_scale_fn=None, freq_scale_fn=None)` (synths.py:43-128): frame-rate controls
    [batch, frames, sinusoids] (frequencies [batch, frames, 1] when `harmonic`: integer multiples of f0, ddsp.py:6-22) ->
    partials at or above Nyquist muted (ddsp.py:25-49) -> amplitudes upsampled with overlapping Hann windows, frequencies
    linearly -> oscillator bank (the HIP kernels behind `oscillator_bank`; differentiable w.r.t. both controls).
    apply_roll_off: the audio then goes through the -6 dB / octave roll-off above 500 Hz of synths.py:121-126 (the decoder of the paper's
    MSS-LogLin runs): `frequency_filter` with the 128 taps of `roll_off_taps`, one filter shared by every clip, on every route."""
    signal = _sinusoidal_signal(amplitudes, frequencies, n_samples, sample_rate, harmonic)
    if apply_roll_off:
        taps = _traced_ops().roll_off_taps(signal.detach()) if (_compiling() and signal.is_cuda) else roll_off_taps(signal.device)
        signal = fft_convolve(signal, taps[None, :].expand(signal.shape[0], -1))
    return signal


def _sinusoidal_signal(amplitudes, frequencies, n_samples, sample_rate, harmonic):
    amplitudes, frequencies = amplitudes.float(), frequencies.float()
    if amplitudes.is_cuda and _envelope_kernels_apply(amplitudes, frequencies, n_samples, harmonic):
        if _compiling():
            return _traced_ops().synth(frequencies, amplitudes, int(n_samples), float(sample_rate), bool(harmonic))
        if FUSED_SYNTH:
            return _Synth.apply(frequencies, amplitudes, int(n_samples), float(sample_rate), bool(harmonic))
        freq_env, amp_env = _SynthEnvelopes.apply(frequencies, amplitudes, int(n_samples), float(sample_rate), bool(harmonic))
        return oscillator_bank(freq_env, amp_env, sample_rate)
    if harmonic:
        k = amplitudes.shape[-1]
        frequencies = frequencies * torch.linspace(1.0, float(k), k, device=frequencies.device)
    amplitudes = torch.where(frequencies >= sample_rate / 2.0, torch.zeros_like(amplitudes), amplitudes)
    return oscillator_bank(upsample_linear(frequencies, n_samples), upsample_window(amplitudes, n_samples), sample_rate)


def slope_frequency_response(decay_per_octave_db, n_freqs, f_ref):
    """The reference's `ddsp.slope_frequency_response` (ddsp.py:738-769): magnitudes [batch, frames, n_freqs] of a response that is 1 up to
    `f_ref` and falls by `decay_per_octave_db` dB per octave above it, on `n_freqs` frequencies from 0 to 8000 Hz.  `decay_per_octave_db`
    is a tensor ([batch, frames, 1], or 0-d); the frequency grid takes ITS dtype and device, as in the reference: the synthesiser's
    `torch.tensor(6)` is int64, so its grid is the exact integers 0, 125, ... and the result (float32 by promotion, [1, 1, n_freqs]) is
    exactly 1 up to 500 Hz.  Torch ops on a handful of values, differentiable w.r.t. a floating decay."""
    decay = decay_per_octave_db
    grid = torch.linspace(0, 8000, n_freqs).to(decay).reshape(1, 1, n_freqs)
    grid[..., :1] = grid[..., :1] + 1e-7                       # keeps log2 away from 0 Hz; vanishes on an integer grid
    per_octave = 10 ** (-decay / 20)                           # pressure factor of one octave
    octaves = torch.log2(grid / f_ref)
    return torch.where(grid > f_ref, per_octave ** octaves, torch.tensor(1.0).to(decay))


def frequency_impulse_response(magnitudes: torch.Tensor, window_size: int = 0) -> torch.Tensor:
    """The reference's `ddsp.frequency_impulse_response` (ddsp.py:382-482), the frequency-sampling design: one-sided magnitudes
    [batch, n_freqs] or [batch, frames, n_freqs] -> zero-phase impulse response (irfft, 2 (n_freqs - 1) taps) -> times a Hann window of
    `window_size` taps centred on tap 0 -> rotated into causal form.  window_size < 1 or beyond the response: the whole response (its
    first tap is then the window's zero); a smaller window also crops the result: to window_size taps when odd, window_size - 1 when even.
    Torch ops, differentiable."""
    response = torch.fft.irfft(magnitudes, dim=-1)
    framed = response.ndim == 3
    if not framed:
        response = response[:, None, :]
    response = response.type(torch.float32)
    size = int(response.shape[-1])
    if window_size <= 0 or window_size > size:
        window_size = size
    window = torch.hann_window(window_size, device=response.device)
    gap = size - window_size
    if gap > 0:
        half = (window_size + 1) // 2
        # the window's second half at the front, its first half at the back, nothing in between
        window = torch.cat([window[half:], torch.zeros(gap, device=response.device), window[:half]], dim=0)
        response = window[None, None, :] * response
        response = torch.cat([response[..., size - half + 2:], response[..., :half + 1]], dim=-1)
    else:
        window = torch.roll(window, shifts=window_size // 2, dims=-1)
        response = torch.roll(window[None, None, :] * response, shifts=size // 2, dims=-1)
    return response if framed else response[:, 0, :]


def _fft_convolve_torch(audio, impulse_response, padding="same", delay_compensation=-1, cross_fade=False):
    """`fft_convolve` on torch ops, in the reference's op order (ddsp.py:504-734): float32 casts, the audio cut into as many frames as the
    impulse response has, both zero-padded to the next power of two >= frame + taps - 1, rfft, product, irfft, overlap-add (fold), crop.
    The crop keeps the reference's arithmetic, oddities included: `start = (taps - 1) // 2 - 1` by default (two samples short of a
    linear-phase filter's delay; -1 and an empty result for two taps), and for padding="valid" an end index that is wrong (empty when
    frame + taps - 1 is a power of two).  cross_fade: the reference's branch cannot run (it hands `irfft` a tuple for `n`); this is what it
    describes -- every frame also filtered with the PREVIOUS frame's response, the two mixed over the first taps - 1 samples with
    sin^2 / cos^2 ramps."""
    audio, impulse_response = audio.type(torch.float32), impulse_response.type(torch.float32)
    if impulse_response.ndim == 2:
        impulse_response = impulse_response[:, None, :]
    ir_batch, n_frames, taps = impulse_response.shape
    batch, samples = audio.shape
    if batch != ir_batch:
        raise ValueError(f"Batch size of audio ({batch}) and impulse response ({ir_batch}) must be the same.")
    frame = -(-samples // n_frames)
    pieces = list(torch.split(audio, frame, dim=-1))
    if pieces[-1].shape[-1] < frame:
        pieces[-1] = torch.nn.functional.pad(pieces[-1], (0, frame - pieces[-1].shape[-1]))
    frames = torch.stack(pieces, dim=1)
    if frames.shape[1] != n_frames:
        raise ValueError(f"Number of audio frames ({frames.shape[1]}) and impulse response frames ({n_frames}) do not match: the number "
                         "of impulse response frames must divide the audio into whole frames.")
    fft_size = 1
    while fft_size < frame + taps - 1:
        fft_size *= 2
    frames = torch.nn.functional.pad(frames, (0, fft_size - frame))
    impulse_response = torch.nn.functional.pad(impulse_response, (0, fft_size - taps))
    audio_spec = torch.fft.rfft(frames)
    ir_spec = torch.fft.rfft(impulse_response)
    filtered = torch.fft.irfft(audio_spec * ir_spec, n=fft_size)
    if cross_fade:
        previous = torch.fft.irfft(audio_spec * torch.roll(ir_spec, shifts=1, dims=1), n=fft_size)
        overlap = taps - 1
        ramp = torch.pi * torch.linspace(0, overlap, overlap, device=audio.device) / (2 * overlap)
        fade_in, fade_out = torch.ones_like(filtered), torch.zeros_like(previous)
        fade_in[:, 1:, :overlap] = torch.sin(ramp) ** 2      # the first frame has no predecessor to fade from
        fade_out[:, 1:, :overlap] = torch.cos(ramp) ** 2
        filtered = filtered * fade_in + previous * fade_out
    total = (n_frames - 1) * frame + fft_size
    out = torch.nn.functional.fold(filtered.transpose(1, 2), output_size=(1, total), kernel_size=(1, fft_size), stride=(1, frame))[:, 0, 0, :]
    if padding == "valid":
        keep = taps + samples - 1
    elif padding == "same":
        keep = samples
    else:
        raise ValueError(f"Padding must be 'valid' or 'same', instead of {padding}.")
    start = (taps - 1) // 2 - 1 if delay_compensation < 0 else delay_compensation
    end = (total - keep) - start
    return out[:, start:-end]


class _FirSame(torch.autograd.Function):
    """sot_fir_same_forward / sot_fir_same_backward (include/sot_hip.h): taps [batch, n_taps], or one shared [n_taps] filter whose
    gradient is the batch sum."""

    @staticmethod
    def forward(ctx, audio, taps, start):
        from . import _native as nat
        ctx.start = start
        ctx.save_for_backward(audio if ctx.needs_input_grad[1] else None, taps)   # the audio is read by the tap gradient only
        return nat.fir_same_forward(audio, taps, start)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        from . import _native as nat
        audio, taps = ctx.saved_tensors
        need_audio, need_taps = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if audio is None:   # not kept (no tap gradient asked): the call then takes the shape from it and never reads it
            audio = grad_out
        grad_audio, grad_taps = nat.fir_same_backward(grad_out.float(), audio, taps, ctx.start, need_audio=need_audio, need_taps=need_taps)
        return grad_audio, grad_taps, None


def fft_convolve(audio: torch.Tensor, impulse_response: torch.Tensor, padding: str = "same", delay_compensation: int = -1,
                 cross_fade: bool = False) -> torch.Tensor:
    """The reference's `ddsp.fft_convolve` (ddsp.py:504-633): audio [batch, samples] filtered with an impulse response [batch, taps]
    (time-invariant) or [batch, frames, taps] (one response per frame of the audio, overlap-added).  padding="same": the full convolution
    cropped to `samples` outputs from sample `delay_compensation`, by default from (taps - 1) // 2 - 1 -- 62 for the 128 taps of
    `frequency_impulse_response`, two short of their delay of 64, so the output is the zero-phase result delayed by two samples (kept:
    it is what the reference's models were trained with).
    float32 GPU tensors with a 2-D response, padding="same", no cross-fade, 3..512 taps, a crop start in [0, taps - 2] and up to 2^20
    samples run the HIP FIR kernels as ONE autograd node (a direct fp32 sum per output; gradients w.r.t. audio and taps; a response
    expanded over the batch is one shared filter).  Everything else -- CPU tensors, other dtypes, time-varying responses, cross_fade,
    padding="valid", sizes outside that domain -- runs `_fft_convolve_torch`, the reference's FFT route on torch ops; a GPU tensor that
    takes it says so once."""
    if audio.is_cuda or impulse_response.is_cuda:
        from . import _native as nat
        taps = int(impulse_response.shape[-1])
        start = (taps - 1) // 2 - 1 if delay_compensation < 0 else int(delay_compensation)
        on_hip = (audio.is_cuda and impulse_response.is_cuda and audio.device == impulse_response.device and audio.dtype == torch.float32
                  and impulse_response.dtype == torch.float32 and audio.ndim == 2 and impulse_response.ndim == 2
                  and audio.shape[0] == impulse_response.shape[0] and audio.shape[0] >= 1 and padding == "same" and not cross_fade
                  and nat.fir_in_domain(int(audio.shape[1]), taps, start))
        if on_hip:
            shared = impulse_response.shape[0] > 1 and impulse_response.stride(0) == 0
            if _compiling():
                return _traced_ops().fir_same(audio, impulse_response[0] if shared else impulse_response, start)
            return _FirSame.apply(audio, impulse_response[0] if shared else impulse_response, start)
        from .losses import warn_once
        warn_once(("fft_convolve", padding, bool(cross_fade), impulse_response.ndim, str(audio.dtype), str(impulse_response.dtype), taps, start),
                  f"fft_convolve: padding={padding!r}, cross_fade={cross_fade}, a {impulse_response.ndim}-D {impulse_response.dtype} response of "
                  f"{taps} taps cropped from {start} on {audio.dtype} audio is outside what the HIP FIR kernels take (float32, 2-D response, "
                  "padding='same', no cross-fade, 3..512 taps, 0 <= start <= taps - 2, up to 2^20 samples); running the FFT route on torch ops "
                  "(rocFFT) instead")
    return _fft_convolve_torch(audio, impulse_response, padding, delay_compensation, cross_fade)


def frequency_filter(audio: torch.Tensor, magnitudes: torch.Tensor, window_size: int = 0, padding: str = "same",
                     cross_fade: bool = False) -> torch.Tensor:
    """The reference's `ddsp.frequency_filter` (ddsp.py:350-379): audio [batch, samples] through the linear-phase FIR filter that
    `frequency_impulse_response` designs from the magnitudes [batch, n_freqs] (or [batch, frames, n_freqs]: time-varying).  Gradients
    w.r.t. the magnitudes flow through the taps' torch ops.  Magnitudes expanded over the batch (stride 0, as the synthesiser's roll-off
    passes them) are designed once and stay one shared filter."""
    if magnitudes.ndim == 2 and magnitudes.shape[0] > 1 and magnitudes.stride(0) == 0:
        taps = frequency_impulse_response(magnitudes[:1], window_size=window_size).expand(magnitudes.shape[0], -1)
    else:
        taps = frequency_impulse_response(magnitudes, window_size=window_size)
    return fft_convolve(audio, taps, padding=padding, cross_fade=cross_fade)


def roll_off_magnitudes(device) -> torch.Tensor:
    """[1, 65] magnitudes of the synthesiser's harmonic roll-off (synths.py:122-123): -6 dB per octave above 500 Hz, from the int64 decay
    the reference passes (see slope_frequency_response)."""
    return slope_frequency_response(torch.tensor(6).to(device), n_freqs=65, f_ref=500)[0]


_ROLL_OFF = _DeviceTableCache()


def roll_off_taps(device) -> torch.Tensor:
    """The 128 taps of the roll-off filter on `device` -- a constant, designed once per device (on that device, like the reference)."""
    return _ROLL_OFF.get(("roll-off taps", str(device)), device, lambda: frequency_impulse_response(roll_off_magnitudes(device))[0],
                         host_side=True)


def harmonic_parameters(size: int, seed: int, n_sinusoids: int = 8, freq_min: float = 40.0, freq_max: float = 1950.0,
                        amp_min: float = 0.4, amp_max: float = 1.0, n_sinusoids_min: int = 1):
    """The parameter draws of the reference's `SimpleSinusoidDataset.setup()` (synthetic_data.py:76-118) after
    `torch.manual_seed(seed)`, harmonic case: frequency [size, 1] ~ U[freq_min, freq_max), weights [size, n] ~ U[amp_min,
    amp_max) with the partials after the first max(1, n_active) muted, n_active ~ U{n_min - 1 .. n - 1} (sequential mask).
    CPU generator, same call order as the reference: identical values for the same seed."""
    g = torch.Generator().manual_seed(seed)
    freqs = torch.rand(size, 1, generator=g) * (freq_max - freq_min) + freq_min
    weights = torch.rand(size, n_sinusoids, generator=g) * (amp_max - amp_min) + amp_min
    n_active = torch.randint(low=n_sinusoids_min - 1, high=n_sinusoids, size=(size,), generator=g)
    mask = torch.arange(1, n_sinusoids).expand(size, n_sinusoids - 1) < n_active.unsqueeze(1)
    mask = torch.cat((torch.ones(size, 1, dtype=torch.bool), mask), dim=1)
    return freqs, weights * mask.float()


def harmonic_items(frequency: torch.Tensor, weights: torch.Tensor, n_samples: int = 4096, sample_rate: int = 16000,
                   n_frames: int = 16) -> torch.Tensor:
    """The audio `x` of the reference's dataset items (synthetic_data.py:174-201 generate_sinusoids + :232-237): the controls
    held constant over `n_frames` frames -> `sinusoidal_synth` -> every clip divided by (its peak + 1e-7) and scaled to 0.9."""
    amps = weights.float().unsqueeze(1).repeat(1, n_frames, 1)
    f0 = frequency.float().reshape(-1, 1, 1).repeat(1, n_frames, 1)
    signal = sinusoidal_synth(amps, f0, n_samples, sample_rate, harmonic=True)
    return signal / (signal.abs().amax(dim=1, keepdim=True) + 1e-7) * 0.9


def harmonic_batch(batch: int, n_samples: int = 4096, sample_rate: float = 16000.0, generator=None, device="cuda", seed=None):
    """`batch` harmonic clips with the reference dataset's distribution and synthesis (harmonic_parameters + harmonic_items)
    on `device`.  seed: the torch.manual_seed the reference would have been given; otherwise the draws come from `generator`
    (a device generator) with the same distribution."""
    dev = torch.device(device)
    if seed is not None:
        freqs, weights = harmonic_parameters(batch, seed)
        return harmonic_items(freqs.to(dev), weights.to(dev), n_samples, int(sample_rate))
    freqs = 40 + (1950 - 40) * torch.rand(batch, 1, generator=generator, device=dev)
    amps = 0.4 + 0.6 * torch.rand(batch, 8, generator=generator, device=dev)
    n_active = torch.randint(0, 8, (batch, 1), generator=generator, device=dev)
    keep = torch.arange(8, device=dev).view(1, 8) < n_active.clamp_min(1)
    return harmonic_items(freqs, amps * keep.float(), n_samples, int(sample_rate))


class _AudioToLoss(torch.autograd.Function):
    """The whole slice behind ONE autograd node: STFT magnitudes of target and estimate, SOT loss with the batch mean
    (forward: 4 kernels), and on the way back the SOT backward kernel w.r.t. the estimate's spectrum followed by the STFT
    backward kernel into the estimate's audio.  Same kernels as the separate nodes, two autograd round trips fewer."""

    @staticmethod
    def forward(ctx, audio_target, audio_estimate, window, pos_x, pos_y, n_fft, hop, p, flags, plan):
        from . import _native as nat
        audio_estimate = audio_estimate.contiguous()
        cplx = None
        if ctx.needs_input_grad[1] and SAVE_SPECTRUM:   # the estimate's complex spectrum rides along: the backward skips its forward transforms
            spec_x, spec_y, cplx = nat.stft_mag_forward_pair(audio_target.contiguous(), audio_estimate, window, n_fft, hop, want_spec_b=True)
        else:
            spec_x, spec_y = nat.stft_mag_forward_pair(audio_target.contiguous(), audio_estimate, window, n_fft, hop)
        rows_x = spec_x.view(-1, spec_x.shape[-1])
        rows_y = spec_y.view(-1, spec_y.shape[-1])
        ctx.early_gy = None
        if ctx.needs_input_grad[1]:   # the gradient w.r.t. the estimate's spectrum comes out of the same pass as the loss
            mean, _, ctx.early_gy = nat.loss_and_grad(rows_x, rows_y, pos_x, pos_y, p, flags, plan)
        else:
            mean, _, _ = nat.loss_fused(rows_x, rows_y, pos_x, pos_y, p, flags, plan)
        ctx.save_for_backward(audio_estimate, window, rows_x, rows_y, pos_x, pos_y, *([cplx] if cplx is not None else []))
        ctx.cfg = (n_fft, hop, p, flags, plan, tuple(spec_y.shape))
        return mean

    @staticmethod
    def backward(ctx, g):
        from . import _native as nat
        audio_estimate, window, rows_x, rows_y, pos_x, pos_y, *cplx = ctx.saved_tensors
        cplx = cplx[0] if cplx else None
        n_fft, hop, p, flags, plan, shape = ctx.cfg
        if not ctx.needs_input_grad[1]:
            return (None,) * 10
        if ctx.early_gy is not None:   # d mean / d spectrum from the forward pass; the STFT backward applies the upstream scalar
            grad_audio = nat.stft_mag_backward(audio_estimate, window, n_fft, hop, ctx.early_gy.view(shape), g.float().contiguous(), spec=cplx)
        else:
            _, gy = nat.backward_rows(rows_x, rows_y, pos_x, pos_y, p, flags, g.float(), need_gx=False, need_gy=True, plan=plan,
                                      grad_scale=1.0 / rows_x.shape[0])
            grad_audio = nat.stft_mag_backward(audio_estimate, window, n_fft, hop, gy.view(shape), spec=cplx)
        return None, grad_audio, None, None, None, None, None, None, None, None


_POSITIONS = {}


def training_step_slice(loss_module, audio_target: torch.Tensor, audio_estimate: torch.Tensor, n_fft: int = 2048, hop: int = 256,
                        sample_rate: float = 16000.0, window="flattop"):
    """One step of the slice trainer.py:192-221 runs around the loss: spectra of target and estimate, unit-scaled
    frequency positions, SOT loss (forward).  The caller backpropagates into `audio_estimate`.
    On the GPU, for the module's plain mean (no hinge) the slice is one autograd node (_AudioToLoss); otherwise it is the
    composition of stft_magnitude and the module."""
    if _compiling() and audio_target.is_cuda:
        return _traced_step_slice(loss_module, audio_target, audio_estimate, n_fft, hop, sample_rate, window)
    dev = audio_target.device
    key = (int(n_fft), float(sample_rate), str(dev))
    pos = _POSITIONS.get(key)
    if pos is None:
        p0 = unit_frequencies(n_fft, sample_rate, dev)
        pos = _POSITIONS[key] = (p0, p0.clone())
    # the one-node form differentiates w.r.t. the estimate only (trainer.py: the target is data); a target that asks for a
    # gradient takes the composed path below, which differentiates through both transforms like losses.py:316-343
    target_needs_grad = torch.is_grad_enabled() and audio_target.requires_grad
    fused = (audio_target.is_cuda and audio_target.ndim == 2 and audio_estimate.shape == audio_target.shape and
             hip_stft_supported(n_fft, hop, audio_target.shape[1]) and not getattr(loss_module, "hinge", False) and
             not target_needs_grad)
    if fused:
        from . import _native as nat
        from .losses import EARLY_GRADIENT, _flags
        flags = _flags(loss_module.square_dist, bool(loss_module.dont_normalize), bool(loss_module.limit_quantile_range),
                       loss_module.require_sort)
        plan = loss_module._plans.get(pos[0], pos[1]) if loss_module.require_sort else None
        glue = nat.glue() if (plan is not None and EARLY_GRADIENT and SAVE_SPECTRUM and audio_target.dtype == torch.float32 and
                              audio_estimate.dtype == torch.float32) else None
        if glue is not None:   # the same four / three kernels behind ONE C++ call and a C++ autograd node (csrc/sot_torch_glue.cpp)
            plan.use_on_current_stream(dev)
            return glue.audio_to_loss(audio_target.contiguous(), audio_estimate.contiguous(), _cached_window(window, n_fft, dev),
                                      plan.xpos_sorted, plan.ypos_sorted, plan.xperm, plan.yperm, plan.ident, int(n_fft), int(hop),
                                      float(loss_module.p), nat.problem_flags(loss_module.p, flags, plan))
        return _AudioToLoss.apply(audio_target.float(), audio_estimate.float(), _cached_window(window, n_fft, dev), pos[0], pos[1],
                                  int(n_fft), int(hop), float(loss_module.p), flags, plan)
    spec_x = stft_magnitude(audio_target, n_fft, hop, window)
    spec_y = stft_magnitude(audio_estimate, n_fft, hop, window)
    return loss_module(spec_x, spec_y, x_pos=pos[0], y_pos=pos[1])


def _traced_step_slice(loss_module, audio_target, audio_estimate, n_fft, hop, sample_rate, window):
    """training_step_slice while torch.compile traces it: the same decision, the one-node form as the op sot_amd::audio_to_loss (which keeps
    the position table and its plan inside), the composition on a copy of the table (sot_amd::unit_frequencies)."""
    o = _traced_ops()
    target_needs_grad = torch.is_grad_enabled() and audio_target.requires_grad
    fused = (audio_target.ndim == 2 and audio_estimate.shape == audio_target.shape and hip_stft_supported(n_fft, hop, audio_target.shape[1])
             and not getattr(loss_module, "hinge", False) and not target_needs_grad)
    if fused:
        from .losses import _flags
        flags = _flags(loss_module.square_dist, bool(loss_module.dont_normalize), bool(loss_module.limit_quantile_range), loss_module.require_sort)
        want_grad = torch.is_grad_enabled() and audio_estimate.requires_grad
        return o.audio_to_loss(audio_target.float(), audio_estimate.float(), _window_name(window), int(n_fft), int(hop), float(sample_rate),
                               float(loss_module.p), flags, want_grad)[0]
    pos = o.unit_frequencies(audio_target.detach(), int(n_fft), float(sample_rate))
    spec_x = stft_magnitude(audio_target, n_fft, hop, window)
    spec_y = stft_magnitude(audio_estimate, n_fft, hop, window)
    return loss_module(spec_x, spec_y, x_pos=pos, y_pos=pos.clone())


def hz_to_unit(hz, hz_min=20.0, hz_max=8000.0, clip: bool = False) -> torch.Tensor:
    """The reference's `utils.hz_to_unit` (utils.py:85-114): frequencies -> MIDI notes (`12 (log(f) / log 2 - log(440) / log 2) + 69` in float32, 0 Hz and
    below -> note 0) -> `(note - note(hz_min)) / (note(hz_max) - note(hz_min))`, optionally clamped to [0, 1].  The position map of the trainer for a loss
    with `log_scaled_x` (trainer.py:187-191).  Plain torch ops: a few hundred bins once per step."""
    def notes(f):
        f = f.type(torch.float32) if isinstance(f, torch.Tensor) else torch.tensor(f, dtype=torch.float32)
        two, a4 = torch.tensor(2.0, dtype=torch.float32), torch.tensor(440.0, dtype=torch.float32)
        n = 12.0 * (torch.log(f) / torch.log(two) - torch.log(a4) / torch.log(two)) + 69.0
        return torch.where(f <= 0.0, torch.tensor(0.0, dtype=torch.float32, device=f.device), n)
    lo, hi = notes(hz_min), notes(hz_max)
    unit = (notes(hz) - lo) / (hi - lo)
    return torch.clamp(unit, 0.0, 1.0) if clip else unit


FUSED_TRAINER_STEP = True    # module switch: trainer_loss_step may take the one-node form below (tests and the bench compare both)


def _fused_mix_step(loss_fn, x, x_hat, x_pos, y_pos, n_fft, hop, window, unit_positions=False, terms=None):
    """`MixOfLosses([MSSLoss, Wasserstein1D], weights)` of the paper's step (train_config.yaml:73-102) on a float32 GPU audio pair as ONE
    C++ call and ONE autograd node (csrc/sot_torch_glue.cpp: MixLossStep) -> the 0-d total, or None when the configuration is not that
    node's case (any other mix, a target that asks for a gradient, `hinge`, per-row positions, transform sizes outside the fused MSS
    kernels): the caller then composes the modules one by one.  Same kernels as the module-by-module route; what goes away is the trainer's
    own arithmetic around them (`* weight`, `.mean()` of a scalar, `0 + value`, gradient accumulation: ~15 launches).
    unit_positions: x_pos / y_pos are the bin frequencies as they are and the node divides them by their maximum inside the plan's launch
    (sot_prepare_unit_positions: `x_pos / x_pos.max()` and the clone of trainer.py:196-197 without their three torch kernels)."""
    from . import losses as L
    from . import _native as nat
    fns, weights = list(loss_fn.losses), list(loss_fn.weights)
    if len(fns) != 2 or not all(isinstance(w, (int, float)) for w in weights):
        return None
    mss = next((f for f in fns if type(f) is L.MSSLoss), None)
    sot = next((f for f in fns if type(f) is L.Wasserstein1D), None)
    if mss is None or sot is None:
        return None
    w_mss, w_sot = float(weights[fns.index(mss)]), float(weights[fns.index(sot)])
    grad_on = torch.is_grad_enabled()
    if not (x.is_cuda and x_hat.is_cuda and x.dtype is torch.float32 and x_hat.dtype is torch.float32 and x.ndim == 2 and x.shape == x_hat.shape
            and x.shape[0] > 0 and x.is_contiguous() and x_hat.is_contiguous() and x.device == x_hat.device
            and not (grad_on and (x.requires_grad or x_pos.requires_grad or y_pos.requires_grad))):
        return None
    samples, bins = x.shape[1], n_fft // 2 + 1
    sizes = tuple(int(s) for s in mss.fft_sizes)
    kind = str(mss.loss_type).upper()
    if not (L.MSS_FUSED and kind in ("L1", "L2") and (mss.mag_weight > 0 or mss.logmag_weight > 0) and 1 <= len(sizes) <= 8
            and all(s in nat.MSS_FUSED_SIZES and hip_stft_supported(s, int(s * 0.25), samples) for s in sizes)):
        return None
    if not (L.EARLY_GRADIENT and SAVE_SPECTRUM and not sot.hinge and sot.require_sort and sot.p >= 1 and hip_stft_supported(n_fft, hop, samples)
            and 2 * bins <= 12000 and L._fresh_grid_ok(x_pos, x, bins) and L._fresh_grid_ok(y_pos, x, bins)):
        return None
    glue = None if _compiling() else nat.glue()
    if not _compiling() and (glue is None or not hasattr(glue, "mix_loss_step")):
        return None
    flags = L._flags(sot.square_dist, sot.dont_normalize, sot.limit_quantile_range, sot.require_sort)
    if getattr(sot, "tie_free_gradient", False):
        flags |= nat.FLAG_TIE_FREE_GRADIENT
    if _compiling():   # the same kernel sequence as the C++ node, as one op
        total, mss_term, sot_term, _ = _traced_ops().mix_loss_step(
            x, x_hat, _window_name(window), x_pos, y_pos, int(n_fft), int(hop), float(sot.p), int(flags), list(sizes), float(mss.mag_weight),
            float(mss.logmag_weight), kind == "L2", w_mss, w_sot, bool(unit_positions), grad_on and x_hat.requires_grad)
    else:
        total, mss_term, sot_term = glue.mix_loss_step(x, x_hat, _cached_window(window, n_fft, x.device), x_pos, y_pos, int(n_fft), int(hop), float(sot.p),
                                                       int(flags), _cached_windows(None, sizes, x.device), list(sizes), float(mss.mag_weight),
                                                       float(mss.logmag_weight), kind == "L2", w_mss, w_sot, bool(unit_positions))
    if terms is not None:   # what the trainer logs per loss (trainer.py:231-236): `(loss_fn(...) * weight).mean()`, values only
        for fn in fns:      # in the order of the mix, like the reference's dict
            terms[fn.__class__.__name__] = mss_term if fn is mss else sot_term
    return total


def trainer_loss_step(loss_fn, x: torch.Tensor, x_hat: torch.Tensor, n_fft: int = 2048, hop: int = 256, window="flattop",
                      sample_rate: float = 16000.0, positions=None, fused=None, terms=None, freq_hz_min="auto", freq_hz_max="auto") -> torch.Tensor:
    """The loss block of the reference's `trainer.shared_step` (trainer.py:183-245) for a `MixOfLosses` (or a single loss module):
    unit-scaled bin frequencies built AFRESH (`x_pos = torch.tensor(transform.get_frequencies()).to(device); x_pos = x_pos / x_pos.max();
    y_pos = x_pos.clone()`, :192-197), both signals through the transform (`TorchSTFT`, :199-200), `MSSLoss` fed the audio and every
    other loss the spectra, each `loss_fn(a, b, x_pos=, y_pos=) * weight` (:206-221), the total = sum of `value.mean()` (:231-236).
    `positions`: a device tensor of bin frequencies to start from; by default the transform's (`rfftfreq`), copied to the device on the first call
    and kept (they are constants of the transform); the division and the clone still run per step (in the one-node form: inside the plan's launch).  The caller backpropagates into `x_hat`.
    `fused` (None = the module switch FUSED_TRAINER_STEP): the paper's own mix -- `MixOfLosses([MSSLoss, Wasserstein1D])` on float32 GPU
    audio -- runs as one host call and one autograd node (_fused_mix_step: the same kernels, none of the per-module arithmetic between
    them); every other configuration, and `fused=False`, composes the modules one by one exactly as the reference's trainer does.
    `terms`: a dict that receives the value of every loss of a mix by class name -- what the trainer logs as `loss/<step>/<name>`
    (trainer.py:231-236) -- detached; costs nothing in the one-node form (the node has both scalars anyway).
    A single loss that carries `log_scaled_x` gets `hz_to_unit` positions between `freq_hz_min` / `freq_hz_max` (trainer.py:187-191)."""
    if positions is None and _compiling() and x.is_cuda:
        positions = _traced_ops().bin_frequencies(x.detach(), int(n_fft), float(sample_rate))   # a copy of the table below, as a value of the traced graph
    if positions is None:
        # torch.tensor(self.transform.get_frequencies()).to(x.device) (trainer.py:192): the values depend on the transform alone, so the copy from the
        # host (pageable memory: a synchronising ~40 us per step, and impossible inside a stream capture) is made once per (n_fft, rate, device) and kept
        positions = _WINDOWS.get(("bin frequencies", int(n_fft), float(sample_rate), str(x.device)), x.device,
                                 lambda: torch.fft.rfftfreq(n_fft, d=1.0 / sample_rate).clone().to(x.device), host_side=True)
    if getattr(loss_fn, "log_scaled_x", False):
        # trainer.py:187-191 (the loss object itself carries the flag -- a MixOfLosses does not, whatever its members say): log-frequency positions
        # between freq_hz_min / freq_hz_max ("auto": the transform's first / last bin frequency, trainer.py:65-70)
        lo = float(positions[0]) if freq_hz_min == "auto" else freq_hz_min
        hi = float(positions[-1]) if freq_hz_max == "auto" else freq_hz_max
        x_pos = hz_to_unit(positions, lo, hi)
        y_pos = x_pos.clone()
        a, b = (x, x_hat) if loss_fn.__class__.__name__ == "MSSLoss" else (stft_magnitude(x, n_fft, hop, window), stft_magnitude(x_hat, n_fft, hop, window))
        return loss_fn(a, b, x_pos=x_pos, y_pos=y_pos).mean()
    if (FUSED_TRAINER_STEP if fused is None else fused) and hasattr(loss_fn, "losses") and hasattr(loss_fn, "weights"):
        # the frequencies go in as they are: the division by the maximum and the second grid are part of the node's plan launch
        total = _fused_mix_step(loss_fn, x, x_hat, positions, positions, n_fft, hop, window, unit_positions=True, terms=terms)
        if total is not None:
            return total
    x_pos = positions / positions.max()
    y_pos = x_pos.clone()
    spec_x = stft_magnitude(x, n_fft, hop, window)
    spec_x_hat = stft_magnitude(x_hat, n_fft, hop, window)
    if hasattr(loss_fn, "losses") and hasattr(loss_fn, "weights"):   # isinstance(self.loss_fn, losses.MixOfLosses)
        distance = {}
        for fn, weight in zip(loss_fn.losses, loss_fn.weights):
            name = fn.__class__.__name__
            a, b = (x, x_hat) if name == "MSSLoss" else (spec_x, spec_x_hat)
            distance[name] = fn(a, b, x_pos=x_pos, y_pos=y_pos) * weight
        loss = 0
        for key, value in distance.items():
            term = value.mean()
            if terms is not None:
                terms[key] = term.detach()
            loss = loss + term
        return loss
    a, b = (x, x_hat) if loss_fn.__class__.__name__ == "MSSLoss" else (spec_x, spec_x_hat)
    return loss_fn(a, b, x_pos=x_pos, y_pos=y_pos).mean()


_METRIC_MODULES = {}


@torch.inference_mode()
def wasserstein_distance(x: torch.Tensor, x_hat: torch.Tensor, p=1, n_fft: int = 512) -> torch.Tensor:
    """The reference's evaluation metric `metrics.wasserstein_distance` (metrics.py:144-149; logged as `1-wasserstein` /
    `2-wasserstein`): magnitude STFTs of both signals as `features.compute_mag` makes them (hann window, 75 % overlap, end padding,
    normalized; features.py:191-237) compared by `Wasserstein1D(p=p, fixed_x=n_fft/2+1)`, mean over every frame.  On the GPU: one STFT
    launch for both signals, then the p = 1 merge-free kernel (both measures live on the `fixed_x` grid) or the merge kernel (p = 2).
    The module is kept per (p, bins, device), so its position plan is made once, not on every evaluation step."""
    from .losses import Wasserstein1D
    hop = int(n_fft * (1.0 - 0.75))
    bins = n_fft // 2 + 1
    key = (p, bins, str(x.device))
    mod = _METRIC_MODULES.get(key)
    if mod is None:
        mod = _METRIC_MODULES[key] = Wasserstein1D(p=p, fixed_x=bins).to(x.device)
    if x.is_cuda and x.ndim == 2 and x.shape == x_hat.shape and hip_stft_supported(n_fft, hop, x.shape[1]):
        from . import _native as nat
        mag_x, mag_x_hat = nat.stft_mag_forward_pair(x.float().contiguous(), x_hat.float().contiguous(), _cached_window(None, n_fft, x.device), n_fft, hop)
    else:
        mag_x, mag_x_hat = stft_magnitude(x, n_fft, hop, None), stft_magnitude(x_hat, n_fft, hop, None)
    return mod(mag_x, mag_x_hat)
