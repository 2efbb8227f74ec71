"""The native calls as `torch.library` custom ops (namespace ``sot_amd``), so that `torch.compile` / `torch.export` can trace the package.

Dynamo cannot look into the ctypes binding (_native.py), the C++ host path (_sot_glue) or the identity-keyed caches in front of them; an
op is opaque to it, carries a fake (meta) implementation for shape propagation and an autograd formula made of `sot_amd::` ops and torch
ops only, so AOTAutograd can trace the backward as well.  The public interface (losses.py, spectra.py) takes these ops when
`torch.compiler.is_compiling()` is true and never otherwise: eager calls keep the autograd.Function classes and the C++ glue.

Every op body is the existing Python binding: the same kernels, the same launch order and the same summation order as the eager route, so
a compiled call returns the eager call's bits.  The bodies
  * do not synchronise, take torch's current stream (the bindings do) and return fresh tensors only (never an input or a view of one);
  * build a position plan from the raw positions on every call and keep none (a plan kept from the warm-up run of
    `mode="reduce-overhead"` would be a live allocation in the graph's private memory pool, which CUDA-graph trees refuse), and decide
    "both measures live on one grid" (the merge-free p = 1 kernel) from tensor identity alone -- never by comparing device memory;
  * fetch the tables that come from host memory (analysis windows, bin frequencies, Hann upsampling windows, roll-off taps, the
    synthesiser's tap tables) from the package's caches by NAME or size.  Those caches are filled when the graph is TRACED -- the fake
    implementations below do it, outside every tracing mode and every graph memory pool -- so neither the warm-up run nor the capture of a
    compiled step allocates a table or meets a pageable-host copy.
An output an op does not compute (a gradient nobody asked for) is an empty tensor of shape [0].

CALLS counts the executions of each op body (tests assert that eager calls never come here).
"""
import collections
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor
from torch.library import custom_op

from . import _native as nat

CALLS = collections.Counter()


def _prefill(make):
    """Run `make` (a call that fills one of the package's device-table caches) for real from a fake implementation, i.e. while a graph is
    being traced: with every dispatch mode off (fake tensors, proxies) and on the real device, if there is one."""
    if torch.cuda.is_available():
        from torch.utils._python_dispatch import _disable_current_modes
        with _disable_current_modes(), torch.no_grad():
            make()


def _none(like: Tensor) -> Tensor:
    return like.new_empty(0)


def _plan(xpos, ypos, flags, unit=False):
    """Position plan of two shared grids, built inside the op on every call (one allocation, one two-workgroup launch) and owned by it.
    One grid is recognised by tensor identity only (PositionPlan.same_grid would compare device memory: a synchronisation); `unit` grids
    are two grids to the kernels, as in the C++ one-node step."""
    if not (flags & nat.FLAG_REQUIRE_SORT):
        return None
    plan = nat.PositionPlan(xpos, ypos, unit=unit)
    plan._same_grid = bool(plan._same_tensor) and not unit
    return plan


def _marshal(x, y, xpos, ypos, flags):
    """(x, y, xpos, ypos, mixed, plan): rows the library can address; mixed = exactly one side is a shared 1-D grid."""
    x, y = nat.rows_view(x), nat.rows_view(y)
    xpos, ypos = xpos.contiguous(), ypos.contiguous()
    if (xpos.ndim == 1) != (ypos.ndim == 1):
        grid = xpos if xpos.ndim == 1 else ypos
        return x, y, xpos, ypos, True, _plan(grid, grid, flags)
    return x, y, xpos, ypos, False, (_plan(xpos, ypos, flags) if xpos.ndim == 1 else None)


def _window(name: str, n_fft: int, device):
    from . import spectra
    return spectra._cached_window(name or None, n_fft, device)   # "" = the reference's window=None (hann)


# ---------------------------------------------------------------- W_p^p rows: shared, per-row and mixed supports

@custom_op("sot_amd::w1d_rows", mutates_args=(), device_types="cuda")
def w1d_rows(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int) -> Tensor:
    """rows[B] = W_p^p per pair (sot_w1d_forward; one 1-D and one 2-D position tensor: sot_w1d_mixed_forward)."""
    CALLS["w1d_rows"] += 1
    x, y, xpos, ypos, mixed, plan = _marshal(x, y, xpos, ypos, flags)
    if mixed:
        return nat.mixed_forward_rows(x, y, xpos, ypos, p, flags, plan)
    return nat.forward_rows(x, y, xpos, ypos, p, flags, plan)


@w1d_rows.register_fake
def _(x, y, xpos, ypos, p, flags):
    return x.new_empty(x.shape[0])


@custom_op("sot_amd::w1d_rows_backward", mutates_args=(), device_types="cuda")
def w1d_rows_backward(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int, grad_rows: Tensor, mean: bool,
                      need_gx: bool, need_gy: bool) -> Tuple[Tensor, Tensor]:
    """Weight gradients (sot_w1d_backward / sot_w1d_mixed_backward).  grad_rows: [B], or one element for every row; mean: the upstream
    is that of the batch mean, i.e. scaled by 1 / B inside the kernel."""
    CALLS["w1d_rows_backward"] += 1
    x, y, xpos, ypos, mixed, plan = _marshal(x, y, xpos, ypos, flags)
    scale = 1.0 / x.shape[0] if mean else 1.0
    call = nat.mixed_backward_rows if mixed else nat.backward_rows
    gx, gy = call(x, y, xpos, ypos, p, flags, grad_rows.float(), need_gx=need_gx, need_gy=need_gy, plan=plan, grad_scale=scale)
    return (gx if gx is not None else _none(x)), (gy if gy is not None else _none(y))


@w1d_rows_backward.register_fake
def _(x, y, xpos, ypos, p, flags, grad_rows, mean, need_gx, need_gy):
    return (x.new_empty(x.shape) if need_gx else x.new_empty(0)), (y.new_empty(y.shape) if need_gy else y.new_empty(0))


@custom_op("sot_amd::w1d_position_grad", mutates_args=(), device_types="cuda")
def w1d_position_grad(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int, grad_rows: Tensor, need_x: bool,
                      need_y: bool) -> Tuple[Tensor, Tensor]:
    """Position gradients (sot_w1d_position_grad + sot_column_sum for a shared row; mixed: sot_w1d_mixed_position_grad, the per-row
    side only), each of its position tensor's shape."""
    CALLS["w1d_position_grad"] += 1
    x, y, xpos, ypos, mixed, plan = _marshal(x, y, xpos, ypos, flags)
    g = grad_rows.float()
    if mixed:
        gpos = nat.mixed_position_grad(x, y, xpos, ypos, p, flags, g, plan=plan)
        return (_none(x), gpos) if xpos.ndim == 1 else (gpos, _none(x))
    from .losses import _position_grads
    gxp, gyp = _position_grads(x, y, xpos, ypos, p, flags, plan, g, need_x, need_y)
    return (gxp if gxp is not None else _none(x)), (gyp if gyp is not None else _none(x))


@w1d_position_grad.register_fake
def _(x, y, xpos, ypos, p, flags, grad_rows, need_x, need_y):
    mixed = (xpos.ndim == 1) != (ypos.ndim == 1)
    want_x = need_x and not (mixed and xpos.ndim == 1)
    want_y = need_y and not (mixed and ypos.ndim == 1)
    return (x.new_empty(xpos.shape) if want_x else x.new_empty(0)), (x.new_empty(ypos.shape) if want_y else x.new_empty(0))


def _weight_and_position_grads(ctx, g, mean):
    """The input gradients of a row / mean op from the upstream `g` ([B], or 0-d for the mean): (gx, gy, gxpos, gypos)."""
    x, y, xpos, ypos = ctx.saved_tensors[:4]
    need = ctx.needs_input_grad
    o = torch.ops.sot_amd
    mixed = (xpos.ndim == 1) != (ypos.ndim == 1)
    if mixed and need[2 if xpos.ndim == 1 else 3]:
        raise RuntimeError("sot_amd: the mixed-supports route has no gradient for the shared grid")
    g = g.float()
    gx = gy = gxp = gyp = None
    if need[0] or need[1]:
        gx, gy = o.w1d_rows_backward(x, y, xpos, ypos, ctx.p, ctx.flags, g, mean, need[0], need[1])
    if need[2] or need[3]:
        rows_g = (g / x.shape[0]).expand(x.shape[0]) if mean else g
        gxp, gyp = o.w1d_position_grad(x, y, xpos, ypos, ctx.p, ctx.flags, rows_g, need[2], need[3])
    return (gx if need[0] else None), (gy if need[1] else None), (gxp if need[2] else None), (gyp if need[3] else None)


def _save_problem(ctx, inputs, output):
    x, y, xpos, ypos, p, flags = inputs[:6]
    ctx.save_for_backward(x, y, xpos, ypos)
    ctx.p, ctx.flags = p, flags


def _rows_backward(ctx, g):
    return (*_weight_and_position_grads(ctx, g, False), None, None)


w1d_rows.register_autograd(_rows_backward, setup_context=_save_problem)


# ---------------------------------------------------------------- the batch mean (Wasserstein1D's default reduction)

@custom_op("sot_amd::w1d_mean", mutates_args=(), device_types="cuda")
def w1d_mean(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int) -> Tensor:
    """0-d mean of the row losses: forward kernel + fixed-order batch-mean kernel behind one native call (sot_w1d_loss)."""
    CALLS["w1d_mean"] += 1
    x, y, xpos, ypos, _, plan = _marshal(x, y, xpos, ypos, flags)
    return nat.loss_fused(x, y, xpos, ypos, p, flags, plan)[0]


@w1d_mean.register_fake
def _(x, y, xpos, ypos, p, flags):
    return x.new_empty(())


def _mean_backward(ctx, g):
    return (*_weight_and_position_grads(ctx, g, True), None, None)


w1d_mean.register_autograd(_mean_backward, setup_context=_save_problem)


@custom_op("sot_amd::w1d_mean_and_grad", mutates_args=(), device_types="cuda")
def w1d_mean_and_grad(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int) -> Tuple[Tensor, Tensor]:
    """The training form (sot_w1d_loss_and_grad): the mean and d mean / d y [B, m] out of one pass over the rows.  Differentiable
    w.r.t. y (the stored gradient times the upstream scalar) and the positions, not w.r.t. x."""
    CALLS["w1d_mean_and_grad"] += 1
    x, y, xpos, ypos, _, plan = _marshal(x, y, xpos, ypos, flags)
    mean, _, gy = nat.loss_and_grad(x, y, xpos, ypos, p, flags, plan)
    return mean, gy


@w1d_mean_and_grad.register_fake
def _(x, y, xpos, ypos, p, flags):
    return x.new_empty(()), x.new_empty((x.shape[0], y.shape[1]))


def _mean_and_grad_setup(ctx, inputs, output):
    x, y, xpos, ypos, p, flags = inputs
    ctx.save_for_backward(x, y, xpos, ypos, output[1])
    ctx.p, ctx.flags = p, flags


def _mean_and_grad_backward(ctx, g, _g_of_gy):
    if ctx.needs_input_grad[0]:
        raise RuntimeError("sot_amd::w1d_mean_and_grad has no gradient w.r.t. x (w1d_mean has)")
    need = ctx.needs_input_grad
    x, y, xpos, ypos, gy = ctx.saved_tensors
    g = g.float()
    gxp = gyp = None
    if need[2] or need[3]:
        gxp, gyp = torch.ops.sot_amd.w1d_position_grad(x, y, xpos, ypos, ctx.p, ctx.flags, (g / x.shape[0]).expand(x.shape[0]), need[2], need[3])
    return None, (gy * g if need[1] else None), (gxp if need[2] else None), (gyp if need[3] else None), None, None


w1d_mean_and_grad.register_autograd(_mean_and_grad_backward, setup_context=_mean_and_grad_setup)


@custom_op("sot_amd::row_mean", mutates_args=(), device_types="cuda")
def row_mean(rows: Tensor) -> Tensor:
    """0-d mean of a flat float32 tensor in the library's fixed-order fp64 accumulation (sot_w1d_reduce_mean)."""
    CALLS["row_mean"] += 1
    return nat.reduce_mean(rows.contiguous())


@row_mean.register_fake
def _(rows):
    return rows.new_empty(())


def _row_mean_setup(ctx, inputs, output):
    ctx.count = inputs[0].numel()


def _row_mean_backward(ctx, g):
    return ((g / ctx.count).expand(ctx.count),)


row_mean.register_autograd(_row_mean_backward, setup_context=_row_mean_setup)


# ---------------------------------------------------------------- return_quantiles

@custom_op("sot_amd::w1d_quantiles", mutates_args=(), device_types="cuda")
def w1d_quantiles(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(uq, vq, Q: [B, n + m]; U: [B, n]; V: [B, m]) -- sot_w1d_quantiles."""
    CALLS["w1d_quantiles"] += 1
    x, y, xpos, ypos, _, plan = _marshal(x, y, xpos, ypos, flags)
    return nat.quantiles(x, y, xpos, ypos, p, flags, plan)


@w1d_quantiles.register_fake
def _(x, y, xpos, ypos, p, flags):
    rows, n, m = x.shape[0], x.shape[1], y.shape[1]
    return (x.new_empty((rows, n + m)), x.new_empty((rows, n + m)), x.new_empty((rows, n + m)), x.new_empty((rows, n)), x.new_empty((rows, m)))


@custom_op("sot_amd::w1d_quantiles_backward", mutates_args=(), device_types="cuda")
def w1d_quantiles_backward(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int, grad_uq: Optional[Tensor],
                           grad_vq: Optional[Tensor], grad_q: Optional[Tensor], grad_u: Optional[Tensor], grad_v: Optional[Tensor],
                           need_x: bool, need_y: bool, need_xpos: bool, need_ypos: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Vector-Jacobian product of w1d_quantiles (sot_w1d_quantiles_backward); an upstream that is None costs no traffic."""
    CALLS["w1d_quantiles_backward"] += 1
    x, y, xpos, ypos, _, plan = _marshal(x, y, xpos, ypos, flags)
    grads = [None if g is None else g.float() for g in (grad_uq, grad_vq, grad_q, grad_u, grad_v)]
    outs = nat.quantiles_backward(x, y, xpos, ypos, p, flags, grads, (need_x, need_y, need_xpos, need_ypos), plan)
    return tuple(t if t is not None else _none(x) for t in outs)


@w1d_quantiles_backward.register_fake
def _(x, y, xpos, ypos, p, flags, grad_uq, grad_vq, grad_q, grad_u, grad_v, need_x, need_y, need_xpos, need_ypos):
    shapes = (x.shape, y.shape, xpos.shape, ypos.shape)
    return tuple(x.new_empty(s) if want else x.new_empty(0) for want, s in zip((need_x, need_y, need_xpos, need_ypos), shapes))


def _quantiles_setup(ctx, inputs, output):
    _save_problem(ctx, inputs, output)
    ctx.set_materialize_grads(False)


def _quantiles_backward(ctx, *grads):
    if all(g is None for g in grads):
        return (None,) * 6
    x, y, xpos, ypos = ctx.saved_tensors
    need = ctx.needs_input_grad[:4]
    out = torch.ops.sot_amd.w1d_quantiles_backward(x, y, xpos, ypos, ctx.p, ctx.flags, *grads, *need)
    return (*[t if want else None for want, t in zip(need, out)], None, None)


w1d_quantiles.register_autograd(_quantiles_backward, setup_context=_quantiles_setup)


# ---------------------------------------------------------------- the STFT producer

def _stft_frames(samples, hop):
    return (samples + hop - 1) // hop   # sot_stft_frames


@custom_op("sot_amd::stft_magnitude", mutates_args=(), device_types="cuda")
def stft_magnitude(audio: Tensor, window: str, n_fft: int, hop: int, want_spec: bool) -> Tuple[Tensor, Tensor]:
    """[clips, samples] -> (magnitudes [clips, frames, n_fft/2+1], complex spectrum [clips, frames, n_fft/2+1, 2] or [0]) --
    sot_stft_mag_forward_spec.  window: a scipy window name, "" for hann; want_spec: keep the spectrum for the backward."""
    CALLS["stft_magnitude"] += 1
    out = nat.stft_mag_forward(audio.contiguous(), _window(window, n_fft, audio.device), n_fft, hop, want_spec=want_spec)
    return out if want_spec else (out, _none(audio))


@stft_magnitude.register_fake
def _(audio, window, n_fft, hop, want_spec):
    _prefill(lambda: _window(window, n_fft, audio.device))
    clips, frames, bins = audio.shape[0], _stft_frames(audio.shape[1], hop), n_fft // 2 + 1
    return audio.new_empty((clips, frames, bins)), (audio.new_empty((clips, frames, bins, 2)) if want_spec else audio.new_empty(0))


@custom_op("sot_amd::stft_magnitude_backward", mutates_args=(), device_types="cuda")
def stft_magnitude_backward(audio: Tensor, window: str, n_fft: int, hop: int, grad_mag: Tensor, grad_scale: Optional[Tensor],
                            spec: Optional[Tensor]) -> Tensor:
    """d L / d audio [clips, samples] (sot_stft_mag_backward_spec).  grad_scale: a one-element tensor multiplying grad_mag inside the
    kernel; spec: the forward's complex spectrum (`audio` then only supplies the shape)."""
    CALLS["stft_magnitude_backward"] += 1
    scale = None if grad_scale is None else grad_scale.float().contiguous()
    return nat.stft_mag_backward(audio.contiguous(), _window(window, n_fft, audio.device), n_fft, hop, grad_mag.float(), scale,
                                 spec=None if spec is None else spec.contiguous())


@stft_magnitude_backward.register_fake
def _(audio, window, n_fft, hop, grad_mag, grad_scale, spec):
    _prefill(lambda: _window(window, n_fft, audio.device))
    return audio.new_empty(audio.shape)


def _stft_setup(ctx, inputs, output):
    audio, ctx.window, ctx.n_fft, ctx.hop, ctx.want_spec = inputs
    ctx.save_for_backward(audio, output[1])


def _stft_backward(ctx, grad_mag, _g_spec):
    audio, spec = ctx.saved_tensors
    grad = torch.ops.sot_amd.stft_magnitude_backward(audio, ctx.window, ctx.n_fft, ctx.hop, grad_mag, None, spec if ctx.want_spec else None)
    return grad, None, None, None, None


stft_magnitude.register_autograd(_stft_backward, setup_context=_stft_setup)


# ---------------------------------------------------------------- MSSLoss, the audio-in slice and the paper's whole loss block

@custom_op("sot_amd::mss_loss", mutates_args=(), device_types="cuda")
def mss_loss(target: Tensor, value: Tensor, fft_sizes: Sequence[int], mag_w: float, logmag_w: float, l2: bool, per_item: bool,
             post_scale: float, want_grad: bool) -> Tuple[Tensor, Tensor]:
    """MSSLoss of [clips, samples] audio (hann windows, 75 % overlap) and d loss / d value in two launches (sot_mss_loss_and_grad):
    (loss: 0-d, or [clips] with per_item; grad_value [clips, samples] or [0]).  Differentiable w.r.t. `value`."""
    CALLS["mss_loss"] += 1
    from . import spectra
    sizes = tuple(int(s) for s in fft_sizes)
    wins = spectra._cached_windows(None, sizes, value.device)
    loss, grad = nat.mss_loss_and_grad(target, value, sizes, wins, mag_w, logmag_w, 1e-5, l2, per_item, want_grad, post_scale)
    return loss, (grad if grad is not None else _none(value))


def _hann_windows(sizes, device):
    from . import spectra
    return [spectra._cached_window(None, int(s), device) for s in sizes]


@mss_loss.register_fake
def _(target, value, fft_sizes, mag_w, logmag_w, l2, per_item, post_scale, want_grad):
    _prefill(lambda: _hann_windows(fft_sizes, value.device))
    return value.new_empty((value.shape[0],) if per_item else ()), (value.new_empty(value.shape) if want_grad else value.new_empty(0))


def _mss_setup(ctx, inputs, output):
    ctx.per_item, ctx.want_grad = inputs[6], inputs[8]
    ctx.save_for_backward(output[1])


def _mss_backward(ctx, g, _g_grad):
    if ctx.needs_input_grad[0]:
        raise RuntimeError("sot_amd::mss_loss has no gradient w.r.t. the target")
    grad_value = None
    if ctx.needs_input_grad[1]:
        if not ctx.want_grad:
            raise RuntimeError("sot_amd::mss_loss was called with want_grad=False")
        (grad,) = ctx.saved_tensors
        g = g.float()
        grad_value = grad * (g.reshape(-1, 1) if ctx.per_item else g)
    return None, grad_value, None, None, None, None, None, None, None


mss_loss.register_autograd(_mss_backward, setup_context=_mss_setup)


def _slice_positions(n_fft, sample_rate, device):
    """The position pair spectra.training_step_slice keeps per (n_fft, rate, device)."""
    from . import spectra
    key = (int(n_fft), float(sample_rate), str(device))
    pos = spectra._POSITIONS.get(key)
    if pos is None:
        p0 = spectra.unit_frequencies(n_fft, sample_rate, device)
        pos = spectra._POSITIONS[key] = (p0, p0.clone())
    return pos


@custom_op("sot_amd::audio_to_loss", mutates_args=(), device_types="cuda")
def audio_to_loss(target: Tensor, estimate: Tensor, window: str, n_fft: int, hop: int, sample_rate: float, p: float, flags: int,
                  want_grad: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """spectra.training_step_slice as one node: STFT pair -> SOT mean on the transform's unit-scaled bin frequencies (+ d mean / d
    spectrum in the same pass) -> (mean 0-d, grad_spectrum [clips, frames, bins] or [0], the estimate's complex spectrum or [0]).
    The backward is stft_magnitude_backward from the stored spectrum with the upstream scalar applied inside it."""
    CALLS["audio_to_loss"] += 1
    dev = target.device
    pos = _slice_positions(n_fft, sample_rate, dev)
    plan = _plan(pos[0], pos[0], flags)   # one grid, by identity
    win = _window(window, n_fft, dev)
    target, estimate = target.contiguous(), estimate.contiguous()
    if want_grad:
        spec_x, spec_y, cplx = nat.stft_mag_forward_pair(target, estimate, win, n_fft, hop, want_spec_b=True)
    else:
        spec_x, spec_y = nat.stft_mag_forward_pair(target, estimate, win, n_fft, hop)
    rows_x, rows_y = spec_x.view(-1, spec_x.shape[-1]), spec_y.view(-1, spec_y.shape[-1])
    if want_grad:
        mean, _, gy = nat.loss_and_grad(rows_x, rows_y, pos[0], pos[0], p, flags, plan)
        return mean, gy.view(spec_y.shape), cplx
    return nat.loss_fused(rows_x, rows_y, pos[0], pos[0], p, flags, plan)[0], _none(target), _none(target)


@audio_to_loss.register_fake
def _(target, estimate, window, n_fft, hop, sample_rate, p, flags, want_grad):
    _prefill(lambda: (_window(window, n_fft, target.device), _slice_positions(n_fft, sample_rate, target.device)))
    clips, frames, bins = target.shape[0], _stft_frames(target.shape[1], hop), n_fft // 2 + 1
    if not want_grad:
        return target.new_empty(()), target.new_empty(0), target.new_empty(0)
    return target.new_empty(()), target.new_empty((clips, frames, bins)), target.new_empty((clips, frames, bins, 2))


def _audio_to_loss_setup(ctx, inputs, output):
    _, estimate, ctx.window, ctx.n_fft, ctx.hop, _, _, _, ctx.want_grad = inputs
    ctx.save_for_backward(estimate, output[1], output[2])


def _audio_to_loss_backward(ctx, g, _g1, _g2):
    if ctx.needs_input_grad[0]:
        raise RuntimeError("sot_amd::audio_to_loss has no gradient w.r.t. the target")
    grad = None
    if ctx.needs_input_grad[1]:
        if not ctx.want_grad:
            raise RuntimeError("sot_amd::audio_to_loss was called with want_grad=False")
        estimate, gy, cplx = ctx.saved_tensors
        grad = torch.ops.sot_amd.stft_magnitude_backward(estimate, ctx.window, ctx.n_fft, ctx.hop, gy, g.float(), cplx)
    return None, grad, None, None, None, None, None, None, None


audio_to_loss.register_autograd(_audio_to_loss_backward, setup_context=_audio_to_loss_setup)


@custom_op("sot_amd::mix_loss_step", mutates_args=(), device_types="cuda")
def mix_loss_step(target: Tensor, estimate: Tensor, window: str, xpos: Tensor, ypos: Tensor, n_fft: int, hop: int, p: float, flags: int,
                  mss_sizes: Sequence[int], mag_w: float, logmag_w: float, l2: bool, w_mss: float, w_sot: float, unit_positions: bool,
                  want_grad: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The paper's loss block `MixOfLosses([MSSLoss, Wasserstein1D])` as one node, the kernel sequence of the C++ host path
    (csrc/sot_torch_glue.cpp: MixLossStep): plan -> STFT pair -> SOT mean + gradient -> MSS loss + gradient (post_scale = w_mss) ->
    STFT backward accumulated into the MSS gradient -> (total, w_mss * MSS, w_sot * SOT, d total / d estimate or [0])."""
    CALLS["mix_loss_step"] += 1
    from . import spectra
    dev = target.device
    target, estimate = target.contiguous(), estimate.contiguous()
    sizes = tuple(int(s) for s in mss_sizes)
    win = _window(window, n_fft, dev)
    plan = _plan(xpos.contiguous(), ypos.contiguous(), flags | nat.FLAG_REQUIRE_SORT, unit=unit_positions)
    if want_grad:
        spec_x, spec_y, cplx = nat.stft_mag_forward_pair(target, estimate, win, n_fft, hop, want_spec_b=True)
    else:
        spec_x, spec_y = nat.stft_mag_forward_pair(target, estimate, win, n_fft, hop)
    rows_x, rows_y = spec_x.view(-1, spec_x.shape[-1]), spec_y.view(-1, spec_y.shape[-1])
    if want_grad:
        sot_mean, _, gy = nat.loss_and_grad(rows_x, rows_y, xpos, ypos, p, flags, plan)
        if w_sot != 1.0:
            gy.mul_(w_sot)
    else:
        sot_mean = nat.loss_fused(rows_x, rows_y, xpos, ypos, p, flags, plan)[0]
    mss_term, grad_audio = nat.mss_loss_and_grad(target, estimate, sizes, spectra._cached_windows(None, sizes, dev), mag_w, logmag_w, 1e-5, l2,
                                                 False, want_grad, post_scale=w_mss)
    if want_grad:
        nat.stft_mag_backward(estimate, win, n_fft, hop, gy.view(spec_y.shape), accumulate_into=grad_audio, spec=cplx)
    sot_term = sot_mean if w_sot == 1.0 else torch.mul(sot_mean, w_sot)
    return torch.add(mss_term, sot_term), mss_term, sot_term, (grad_audio if want_grad else _none(target))


@mix_loss_step.register_fake
def _(target, estimate, window, xpos, ypos, n_fft, hop, p, flags, mss_sizes, mag_w, logmag_w, l2, w_mss, w_sot, unit_positions, want_grad):
    _prefill(lambda: (_window(window, n_fft, target.device), _hann_windows(mss_sizes, target.device)))
    s = target.new_empty(())
    return s, target.new_empty(()), target.new_empty(()), (target.new_empty(target.shape) if want_grad else target.new_empty(0))


def _mix_setup(ctx, inputs, output):
    ctx.want_grad = inputs[-1]
    ctx.save_for_backward(output[3])
    ctx.mark_non_differentiable(output[1], output[2], output[3])


def _mix_backward(ctx, g, *_):
    if any(ctx.needs_input_grad[i] for i in (0, 3, 4)):
        raise RuntimeError("sot_amd::mix_loss_step has no gradient w.r.t. the target or the positions")
    grad = None
    if ctx.needs_input_grad[1]:
        if not ctx.want_grad:
            raise RuntimeError("sot_amd::mix_loss_step was called with want_grad=False")
        (grad_audio,) = ctx.saved_tensors
        grad = grad_audio * g.float()
    return (None, grad) + (None,) * 15


mix_loss_step.register_autograd(_mix_backward, setup_context=_mix_setup)


# ---------------------------------------------------------------- tables that live in host-filled caches, as graph values

@custom_op("sot_amd::bin_frequencies", mutates_args=(), device_types="cuda")
def bin_frequencies(like: Tensor, n_fft: int, sample_rate: float) -> Tensor:
    """rfftfreq(n_fft, 1 / sample_rate) on `like`'s device: a copy of the table spectra.trainer_loss_step keeps."""
    CALLS["bin_frequencies"] += 1
    return _bin_frequency_table(n_fft, sample_rate, like.device).clone()


def _bin_frequency_table(n_fft, sample_rate, dev):
    from . import spectra
    return spectra._WINDOWS.get(("bin frequencies", int(n_fft), float(sample_rate), str(dev)), dev,
                                lambda: torch.fft.rfftfreq(n_fft, d=1.0 / sample_rate).clone().to(dev), host_side=True)


@bin_frequencies.register_fake
def _(like, n_fft, sample_rate):
    _prefill(lambda: _bin_frequency_table(n_fft, sample_rate, like.device))
    return like.new_empty(n_fft // 2 + 1, dtype=torch.float32)


@custom_op("sot_amd::unit_frequencies", mutates_args=(), device_types="cuda")
def unit_frequencies(like: Tensor, n_fft: int, sample_rate: float) -> Tensor:
    """spectra.unit_frequencies on `like`'s device: a copy of a table made once per (n_fft, rate, device)."""
    CALLS["unit_frequencies"] += 1
    return _unit_frequency_table(n_fft, sample_rate, like.device).clone()


def _unit_frequency_table(n_fft, sample_rate, dev):
    from . import spectra
    return spectra._WINDOWS.get(("unit frequencies", int(n_fft), float(sample_rate), str(dev)), dev,
                                lambda: spectra.unit_frequencies(n_fft, sample_rate, dev), host_side=True)


@unit_frequencies.register_fake
def _(like, n_fft, sample_rate):
    _prefill(lambda: _unit_frequency_table(n_fft, sample_rate, like.device))
    return like.new_empty(n_fft // 2 + 1, dtype=torch.float32)


@custom_op("sot_amd::roll_off_taps", mutates_args=(), device_types="cuda")
def roll_off_taps(like: Tensor) -> Tensor:
    """A copy of the 128 taps of the synthesiser's roll-off filter (spectra.roll_off_taps) on `like`'s device."""
    CALLS["roll_off_taps"] += 1
    from . import spectra
    return spectra.roll_off_taps(like.device).clone()


@roll_off_taps.register_fake
def _(like):
    from . import spectra
    _prefill(lambda: spectra.roll_off_taps(like.device))
    return like.new_empty(128, dtype=torch.float32)


# ---------------------------------------------------------------- the synthesiser side

@custom_op("sot_amd::synth", mutates_args=(), device_types="cuda")
def synth(frequencies: Tensor, amplitudes: Tensor, n_samples: int, sample_rate: float, harmonic: bool) -> Tensor:
    """Frame-rate controls -> audio [clips, n_samples] (sot_synth_forward)."""
    CALLS["synth"] += 1
    frequencies, amplitudes = frequencies.contiguous(), amplitudes.contiguous()
    window, _ = _synth_tables(amplitudes, n_samples, False)
    return nat.synth_forward(amplitudes, frequencies, window, n_samples, sample_rate, harmonic)[0]


def _synth_tables(amplitudes, n_samples, backward):
    from . import spectra
    window = spectra._hann_on(amplitudes.device, n_samples // amplitudes.shape[1])
    return window, (spectra._tap_tables_on(window, amplitudes.shape[1], n_samples) if backward else None)


@synth.register_fake
def _(frequencies, amplitudes, n_samples, sample_rate, harmonic):
    if isinstance(n_samples, int) and isinstance(amplitudes.shape[1], int):
        _prefill(lambda: _synth_tables(amplitudes, n_samples, False))
    return amplitudes.new_empty((amplitudes.shape[0], n_samples))


@custom_op("sot_amd::synth_backward", mutates_args=(), device_types="cuda")
def synth_backward(frequencies: Tensor, amplitudes: Tensor, n_samples: int, sample_rate: float, harmonic: bool, grad_audio: Tensor,
                   need_freq: bool, need_amp: bool) -> Tuple[Tensor, Tensor]:
    """(grad_frequencies, grad_amplitudes) of synth (sot_synth_backward; the segment start phases are computed again)."""
    CALLS["synth_backward"] += 1
    frequencies, amplitudes = frequencies.contiguous(), amplitudes.contiguous()
    window, taps = _synth_tables(amplitudes, n_samples, True)
    ga, gf = nat.synth_backward(amplitudes, frequencies, window, n_samples, sample_rate, harmonic, grad_audio.float(), need_amp=need_amp,
                                need_freq=need_freq, tap_tables=taps)
    return (gf if gf is not None else _none(frequencies)), (ga if ga is not None else _none(amplitudes))


@synth_backward.register_fake
def _(frequencies, amplitudes, n_samples, sample_rate, harmonic, grad_audio, need_freq, need_amp):
    if isinstance(n_samples, int) and isinstance(amplitudes.shape[1], int):
        _prefill(lambda: _synth_tables(amplitudes, n_samples, True))
    return (frequencies.new_empty(frequencies.shape) if need_freq else frequencies.new_empty(0),
            amplitudes.new_empty(amplitudes.shape) if need_amp else amplitudes.new_empty(0))


def _synth_setup(ctx, inputs, output):
    frequencies, amplitudes, ctx.n_samples, ctx.sample_rate, ctx.harmonic = inputs
    ctx.save_for_backward(frequencies, amplitudes)


def _synth_backward(ctx, grad_audio):
    frequencies, amplitudes = ctx.saved_tensors
    need_f, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gf, ga = torch.ops.sot_amd.synth_backward(frequencies, amplitudes, ctx.n_samples, ctx.sample_rate, ctx.harmonic, grad_audio, need_f, need_a)
    return (gf if need_f else None), (ga if need_a else None), None, None, None


synth.register_autograd(_synth_backward, setup_context=_synth_setup)


@custom_op("sot_amd::oscillator_bank", mutates_args=(), device_types="cuda")
def oscillator_bank(freq: Tensor, amp: Tensor, sample_rate: float) -> Tensor:
    """Sample-rate envelopes [clips, samples, sinusoids] -> audio [clips, samples] (sot_oscillator_bank_forward)."""
    CALLS["oscillator_bank"] += 1
    return nat.oscillator_bank_forward(freq, amp, sample_rate)


@oscillator_bank.register_fake
def _(freq, amp, sample_rate):
    return freq.new_empty((freq.shape[0], freq.shape[1]))


@custom_op("sot_amd::oscillator_bank_backward", mutates_args=(), device_types="cuda")
def oscillator_bank_backward(freq: Tensor, amp: Tensor, sample_rate: float, grad_audio: Tensor, need_freq: bool,
                             need_amp: bool) -> Tuple[Tensor, Tensor]:
    """(grad_freq, grad_amp) of oscillator_bank (sot_oscillator_bank_backward; the segment start phases are computed again)."""
    CALLS["oscillator_bank_backward"] += 1
    gf, ga = nat.oscillator_bank_backward(freq, amp, sample_rate, grad_audio.float(), need_freq=need_freq, need_amp=need_amp)
    return (gf if gf is not None else _none(freq)), (ga if ga is not None else _none(amp))


@oscillator_bank_backward.register_fake
def _(freq, amp, sample_rate, grad_audio, need_freq, need_amp):
    return (freq.new_empty(freq.shape) if need_freq else freq.new_empty(0)), (amp.new_empty(amp.shape) if need_amp else amp.new_empty(0))


def _osc_setup(ctx, inputs, output):
    freq, amp, ctx.sample_rate = inputs
    ctx.save_for_backward(freq, amp)


def _osc_backward(ctx, grad_audio):
    freq, amp = ctx.saved_tensors
    need_f, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gf, ga = torch.ops.sot_amd.oscillator_bank_backward(freq, amp, ctx.sample_rate, grad_audio, need_f, need_a)
    return (gf if need_f else None), (ga if need_a else None), None


oscillator_bank.register_autograd(_osc_backward, setup_context=_osc_setup)


@custom_op("sot_amd::fir_same", mutates_args=(), device_types="cuda")
def fir_same(audio: Tensor, taps: Tensor, start: int) -> Tensor:
    """out[b, t] = sum_k taps[b, k] audio[b, t + start - k] (sot_fir_same_forward); taps [clips, n_taps] or one shared [n_taps]."""
    CALLS["fir_same"] += 1
    return nat.fir_same_forward(audio, taps, start)


@fir_same.register_fake
def _(audio, taps, start):
    return audio.new_empty(audio.shape)


@custom_op("sot_amd::fir_same_backward", mutates_args=(), device_types="cuda")
def fir_same_backward(grad_out: Tensor, audio: Tensor, taps: Tensor, start: int, need_audio: bool, need_taps: bool) -> Tuple[Tensor, Tensor]:
    """(grad_audio, grad_taps) of fir_same (sot_fir_same_backward; a shared filter's gradient is the batch sum)."""
    CALLS["fir_same_backward"] += 1
    ga, gt = nat.fir_same_backward(grad_out.float(), audio, taps, start, need_audio=need_audio, need_taps=need_taps)
    return (ga if ga is not None else _none(audio)), (gt if gt is not None else _none(taps))


@fir_same_backward.register_fake
def _(grad_out, audio, taps, start, need_audio, need_taps):
    return (audio.new_empty(audio.shape) if need_audio else audio.new_empty(0)), (taps.new_empty(taps.shape) if need_taps else taps.new_empty(0))


def _fir_setup(ctx, inputs, output):
    audio, taps, ctx.start = inputs
    ctx.save_for_backward(audio, taps)


def _fir_backward(ctx, grad_out):
    audio, taps = ctx.saved_tensors
    need_a, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    ga, gt = torch.ops.sot_amd.fir_same_backward(grad_out, audio, taps, ctx.start, need_a, need_t)
    return (ga if need_a else None), (gt if need_t else None), None


fir_same.register_autograd(_fir_backward, setup_context=_fir_setup)

# ---------------------------------------------------------------- bfloat16 weight rows (include/sot_hip.h, ABI 19)

@custom_op("sot_amd::rows_to_f32", mutates_args=(), device_types="cuda")
def rows_to_f32(rows: Tensor) -> Tensor:
    """[B, n] bfloat16 rows -> dense float32 (sot_rows_bf16_to_f32; exact).  Backward: rows_to_bf16 of the incoming gradient."""
    CALLS["rows_to_f32"] += 1
    return nat.rows_to_f32(rows)


@rows_to_f32.register_fake
def _(rows):
    return rows.new_empty(rows.shape, dtype=torch.float32)


@custom_op("sot_amd::rows_to_bf16", mutates_args=(), device_types="cuda")
def rows_to_bf16(rows: Tensor) -> Tensor:
    """[B, n] float32 rows -> dense bfloat16, round to nearest even (sot_rows_f32_to_bf16).  Backward: rows_to_f32 of the gradient."""
    CALLS["rows_to_bf16"] += 1
    return nat.rows_to_bf16(rows.float())


@rows_to_bf16.register_fake
def _(rows):
    return rows.new_empty(rows.shape, dtype=torch.bfloat16)


def _no_setup(ctx, inputs, output):
    pass


def _rows_to_f32_backward(ctx, g):
    return (torch.ops.sot_amd.rows_to_bf16(g),)


def _rows_to_bf16_backward(ctx, g):
    return (torch.ops.sot_amd.rows_to_f32(g),)


rows_to_f32.register_autograd(_rows_to_f32_backward, setup_context=_no_setup)
rows_to_bf16.register_autograd(_rows_to_bf16_backward, setup_context=_no_setup)


@custom_op("sot_amd::w1d_rows_bf16", mutates_args=(), device_types="cuda")
def w1d_rows_bf16(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int) -> Tensor:
    """float32 rows[B] = W_p^p per pair of bfloat16 weight rows (sot_w1d_forward_bf16): shared or per-row float32 positions."""
    CALLS["w1d_rows_bf16"] += 1
    x, y, xpos, ypos, mixed, plan = _marshal(x, y, xpos, ypos, flags)
    if mixed:
        raise RuntimeError("sot_amd::w1d_rows_bf16 takes both position tensors of one kind (widen with rows_to_f32 for mixed supports)")
    return nat.forward_rows_bf16(x, y, xpos, ypos, p, flags, plan)


@w1d_rows_bf16.register_fake
def _(x, y, xpos, ypos, p, flags):
    return x.new_empty(x.shape[0], dtype=torch.float32)


@custom_op("sot_amd::w1d_mean_bf16", mutates_args=(), device_types="cuda")
def w1d_mean_bf16(x: Tensor, y: Tensor, xpos: Tensor, ypos: Tensor, p: float, flags: int) -> Tensor:
    """0-d float32 mean of the row losses of bfloat16 weight rows (sot_w1d_loss_bf16)."""
    CALLS["w1d_mean_bf16"] += 1
    x, y, xpos, ypos, mixed, plan = _marshal(x, y, xpos, ypos, flags)
    if mixed:
        raise RuntimeError("sot_amd::w1d_mean_bf16 takes both position tensors of one kind (widen with rows_to_f32 for mixed supports)")
    return nat.loss_fused_bf16(x, y, xpos, ypos, p, flags, plan)[0]


@w1d_mean_bf16.register_fake
def _(x, y, xpos, ypos, p, flags):
    return x.new_empty((), dtype=torch.float32)


def _bf16_grads(ctx, g, mean):
    """The typed forward's input gradients: the float32 backward on the widened operands, weight gradients narrowed to bfloat16."""
    x, y, xpos, ypos = ctx.saved_tensors
    need = ctx.needs_input_grad
    o = torch.ops.sot_amd
    g = g.float()
    gx = gy = gxp = gyp = None
    if need[0] or need[1] or need[2] or need[3]:
        xf, yf = o.rows_to_f32(x), o.rows_to_f32(y)
    if need[0] or need[1]:
        gx, gy = o.w1d_rows_backward(xf, yf, xpos, ypos, ctx.p, ctx.flags, g, mean, need[0], need[1])
        gx = o.rows_to_bf16(gx) if need[0] else None
        gy = o.rows_to_bf16(gy) if need[1] else None
    if need[2] or need[3]:
        rows_g = (g / x.shape[0]).expand(x.shape[0]) if mean else g
        gxp, gyp = o.w1d_position_grad(xf, yf, xpos, ypos, ctx.p, ctx.flags, rows_g, need[2], need[3])
    return gx, gy, (gxp if need[2] else None), (gyp if need[3] else None), None, None


def _rows_bf16_backward(ctx, g):
    return _bf16_grads(ctx, g, False)


def _mean_bf16_backward(ctx, g):
    return _bf16_grads(ctx, g, True)


w1d_rows_bf16.register_autograd(_rows_bf16_backward, setup_context=_save_problem)
w1d_mean_bf16.register_autograd(_mean_bf16_backward, setup_context=_save_problem)

# the bfloat16 ops, listed apart from NAMES / AUTOGRAD below (whose members tests/test_compile_*.py enumerate one by one)
BF16_NAMES = ("rows_to_f32", "rows_to_bf16", "w1d_rows_bf16", "w1d_mean_bf16")
BF16_AUTOGRAD = {
    "rows_to_f32": (_no_setup, _rows_to_f32_backward), "rows_to_bf16": (_no_setup, _rows_to_bf16_backward),
    "w1d_rows_bf16": (_save_problem, _rows_bf16_backward), "w1d_mean_bf16": (_save_problem, _mean_bf16_backward),
}

# op name -> (setup_context, backward): the autograd formulas registered above (tests trace them without an autograd engine)
AUTOGRAD = {
    "w1d_rows": (_save_problem, _rows_backward), "w1d_mean": (_save_problem, _mean_backward),
    "w1d_mean_and_grad": (_mean_and_grad_setup, _mean_and_grad_backward), "row_mean": (_row_mean_setup, _row_mean_backward),
    "w1d_quantiles": (_quantiles_setup, _quantiles_backward), "stft_magnitude": (_stft_setup, _stft_backward),
    "mss_loss": (_mss_setup, _mss_backward), "audio_to_loss": (_audio_to_loss_setup, _audio_to_loss_backward),
    "mix_loss_step": (_mix_setup, _mix_backward), "synth": (_synth_setup, _synth_backward), "oscillator_bank": (_osc_setup, _osc_backward),
    "fir_same": (_fir_setup, _fir_backward),
}

NAMES = ("w1d_rows", "w1d_rows_backward", "w1d_position_grad", "w1d_mean", "w1d_mean_and_grad", "row_mean", "w1d_quantiles",
         "w1d_quantiles_backward", "stft_magnitude", "stft_magnitude_backward", "mss_loss", "audio_to_loss", "mix_loss_step",
         "bin_frequencies", "unit_frequencies", "roll_off_taps", "synth", "synth_backward", "oscillator_bank", "oscillator_bank_backward",
         "fir_same", "fir_same_backward")
