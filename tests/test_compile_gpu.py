"""torch.compile / torch.export on the GPU route (sot_amd/ops.py): a compiled call runs the same kernels on the same inputs in the same
order as the eager call, so values and gradients are compared with torch.equal -- no tolerance, except where Inductor itself rewrites
the torch arithmetic between the ops (the trainer loop's `a * w1 + b * w2`; see test_trainer_loop_inductor).

Shapes are the smallest that reach every route: [5, 33] and [5, 257] weights, a [33] grid against [5, 8] per-row positions, 9 rows of
1025 and 2048 bins (the compile-time kernels), a row stride larger than the row, 3 clips of 1536 samples (n_fft 256 / 64), 4 frames x
8 partials -> 512 samples."""
import pytest
import torch

from gpu_util import device, native

pytestmark = pytest.mark.gpu


def _gen(seed=0):
    return torch.Generator(device=device()).manual_seed(seed)


def _rand(*shape, g, lo=0.0, hi=1.0):
    return lo + (hi - lo) * torch.rand(*shape, generator=g, device=device())


def _flat(out):
    if isinstance(out, dict):
        out = list(out.values())
    return list(out) if isinstance(out, (list, tuple)) else [out]


def _value_and_grads(fn, tensors, wrt):
    """fn(*tensors) on fresh leaves; the outputs are folded into one scalar with fixed non-trivial upstream weights (0.5 .. 1.5 over
    every output's elements, 1.7 for a 0-d output) and differentiated w.r.t. the leaves in `wrt`."""
    leaves = [t.detach().clone().requires_grad_(i in wrt) if t.is_contiguous() else t.detach() for i, t in enumerate(tensors)]
    outs = _flat(fn(*leaves))
    total = 0
    for o in outs:
        w = torch.linspace(0.5, 1.5, o.numel(), device=o.device).reshape(o.shape) if o.ndim else torch.tensor(1.7, device=o.device)
        total = total + (o * w).sum()
    total.backward()
    return [o.detach() for o in outs], [leaves[i].grad for i in wrt]


def _check_compiled_equals_eager(fn, tensors, wrt, backend="aot_eager"):
    from sot_amd import ops
    native()
    before = sum(ops.CALLS.values())
    want_out, want_grads = _value_and_grads(fn, tensors, wrt)
    assert sum(ops.CALLS.values()) == before, "an eager call entered sot_amd/ops.py"
    compiled = torch.compile(fn, fullgraph=True, backend=backend)
    got_out, got_grads = _value_and_grads(compiled, tensors, wrt)
    assert sum(ops.CALLS.values()) > before, "the compiled call did not run the sot_amd:: ops"
    assert len(got_out) == len(want_out)
    for k, (a, b) in enumerate(zip(got_out, want_out)):
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
        assert torch.equal(a, b), f"output {k}: max |diff| {float((a - b).abs().max()):.3e}"
    for i, a, b in zip(wrt, got_grads, want_grads):
        assert a is not None and b is not None, f"no gradient for input {i}"
        assert torch.equal(a, b), f"gradient of input {i}: max |diff| {float((a - b).abs().max()):.3e} of {float(b.abs().max()):.3e}"


def _paper(**kw):
    from sot_amd.losses import Wasserstein1D
    return Wasserstein1D(p=2, dont_normalize=True, limit_quantile_range=True, square_dist=True, **kw).to(device())


def _w1d_cases():
    from sot_amd.losses import Wasserstein1D, wasserstein_1d
    g = _gen(1)
    W = lambda *s: _rand(*s, g=g, lo=0.05, hi=1.0)   # noqa: E731
    P = lambda *s: _rand(*s, g=g)                      # noqa: E731
    paper = _paper()
    p1 = Wasserstein1D(p=1).to(device())
    cases = {}
    # (function of the tensors, tensors, indices of the tensors that get a gradient)
    cases["paper_shared_y"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b), [W(5, 33), W(5, 33), P(33), P(33)], (1,))
    cases["paper_shared_all"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b), [W(5, 33), W(5, 33), P(33), P(33)], (0, 1, 2, 3))
    cases["paper_257"] = (lambda x, y, a: paper(x, y, x_pos=a, y_pos=a), [W(5, 257), W(5, 257), P(257)], (1,))
    cases["per_row_mean"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b), [W(5, 33), W(5, 33), P(5, 33), P(5, 33)], (1, 2, 3))
    cases["per_row_rows"] = (lambda x, y, a, b: paper.row_losses(x, y, x_pos=a, y_pos=b), [W(5, 33), W(5, 33), P(5, 33), P(5, 33)], (0, 1, 2, 3))
    cases["mixed"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b), [W(5, 33), W(5, 8), P(33), P(5, 8)], (0, 1, 3))
    hinged = Wasserstein1D(p=1, hinge=True).to(device())
    cases["hinge"] = (lambda x, y, a, b: hinged(x, y, x_pos=a, y_pos=b, hinge=0.1), [W(5, 33), W(5, 33), P(33), P(33)], (0, 1))
    cases["dims"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b, dims=1), [W(2, 3, 33), W(2, 3, 33), P(33), P(33)], (0, 1))
    cases["quantiles_shared"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b, return_quantiles=True), [W(5, 33), W(5, 33), P(33), P(33)], (0, 1, 2, 3))
    cases["quantiles_per_row"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b, return_quantiles=True), [W(5, 33), W(5, 33), P(5, 33), P(5, 33)],
                                  (0, 1, 2, 3))
    area = Wasserstein1D(p=1, fixed_x=257).to(device())
    cases["p1_one_grid_area"] = (lambda x, y: area(x, y), [W(5, 257), W(5, 257)], (1,))
    cases["p1_two_tensors"] = (lambda x, y, a: p1(x, y, x_pos=a, y_pos=a), [W(5, 33), W(5, 33), P(33)], (0, 1))
    cases["paper_9x1025"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b), [W(9, 1025), W(9, 1025), P(1025), P(1025)], (1,))
    area2048 = Wasserstein1D(p=1, fixed_x=2048).to(device())
    cases["p1_9x2048"] = (lambda x, y: area2048(x, y), [W(9, 2048), W(9, 2048)], (1,))
    cases["strided_x"] = (lambda x, y, a, b: paper(x, y, x_pos=a, y_pos=b), [W(5, 40)[:, :33], W(5, 33), P(33), P(33)], (1,))
    cases["functional"] = (lambda u, v, uw, vw: wasserstein_1d(u, v, uw, vw, p=2), [P(5, 33), P(5, 33), W(5, 33), W(5, 33)], (2, 3))
    return cases


W1D_CASES = ["paper_shared_y", "paper_shared_all", "paper_257", "per_row_mean", "per_row_rows", "mixed", "hinge", "dims", "quantiles_shared",
             "quantiles_per_row", "p1_one_grid_area", "p1_two_tensors", "paper_9x1025", "p1_9x2048", "strided_x", "functional"]


@pytest.mark.parametrize("name", W1D_CASES)
def test_wasserstein_compiled_equals_eager(name):
    fn, tensors, wrt = _w1d_cases()[name]
    _check_compiled_equals_eager(fn, tensors, wrt)


def _mix(sizes=(256, 64)):
    from sot_amd.losses import MixOfLosses, MSSLoss, Wasserstein1D
    return MixOfLosses([MSSLoss(fft_sizes=sizes, loss_type="L1", mag_weight=1, logmag_weight=0),
                        Wasserstein1D(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True, require_sort=True)], [0.05, 1]).to(device())


def _audio_cases():
    from sot_amd import spectra
    from sot_amd.losses import KL, MixOfLosses, MSSLoss, Wasserstein1DWithTransform
    g = _gen(2)
    A = lambda *s: _rand(*s, g=g, lo=-0.5, hi=0.5)   # noqa: E731
    mss = MSSLoss(fft_sizes=(256, 64), mag_weight=1.0, logmag_weight=0.5).to(device())
    mix = _mix()
    paper = _paper()
    audio_in = Wasserstein1DWithTransform(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True,
                                          transform_kwargs={"type": "stft", "n_fft": 256, "hop_length": 64}).to(device())
    amps = _rand(2, 4, 8, g=g, lo=0.1, hi=1.0)
    f0 = _rand(2, 4, 1, g=g, lo=100.0, hi=400.0)
    cases = {}
    cases["mss"] = (lambda t, v: mss(t, v), [A(3, 1536), A(3, 1536)], (1,))
    cases["mss_per_clip"] = (lambda t, v: mss(t, v, dims=(1, 2)), [A(3, 1536), A(3, 1536)], (1,))
    cases["stft_flattop"] = (lambda a: spectra.stft_magnitude(a, n_fft=256, hop=64), [A(3, 1536)], (0,))
    cases["stft_hann"] = (lambda a: spectra.stft_magnitude(a, 256, 64, None), [A(3, 1536)], (0,))
    cases["trainer_step_fused"] = (lambda a, b: spectra.trainer_loss_step(mix, a, b, n_fft=256, hop=64), [A(3, 1536), A(3, 1536)], (1,))
    cases["trainer_step_modules"] = (lambda a, b: spectra.trainer_loss_step(mix, a, b, n_fft=256, hop=64, fused=False), [A(3, 1536), A(3, 1536)], (1,))
    cases["step_slice"] = (lambda a, b: spectra.training_step_slice(paper, a, b, n_fft=256, hop=64), [A(3, 1536), A(3, 1536)], (1,))
    cases["audio_in_module"] = (lambda a, b: audio_in(a, b), [A(3, 1536), A(3, 1536)], (1,))
    spectral_mix = MixOfLosses([paper, KL()], [0.5, 2.0]).to(device())   # -> {class name: weighted loss}
    cases["mix_of_losses"] = (lambda a, b, pos: spectral_mix(spectra.stft_magnitude(a, 256, 64), spectra.stft_magnitude(b, 256, 64), x_pos=pos, y_pos=pos),
                              [A(3, 1536), A(3, 1536), _rand(129, g=g)], (1,))
    cases["synth"] = (lambda a, f: spectra.sinusoidal_synth(a, f, 512), [amps, f0], (0, 1))
    cases["synth_roll_off"] = (lambda a, f: spectra.sinusoidal_synth(a, f, 512, apply_roll_off=True), [amps, f0], (0, 1))
    cases["oscillator_bank"] = (lambda f, a: spectra.oscillator_bank(f, a), [_rand(2, 512, 8, g=g, lo=100.0, hi=4000.0), _rand(2, 512, 8, g=g)], (0, 1))
    cases["fft_convolve"] = (lambda a, t: spectra.fft_convolve(a, t), [A(2, 512), A(2, 128)], (0, 1))
    cases["frequency_filter"] = (lambda a, m: spectra.frequency_filter(a, m), [A(2, 512), _rand(2, 65, g=g)], (0, 1))
    return cases


AUDIO_CASES = ["mss", "mss_per_clip", "stft_flattop", "stft_hann", "trainer_step_fused", "trainer_step_modules", "step_slice", "audio_in_module",
               "mix_of_losses", "synth", "synth_roll_off", "oscillator_bank", "fft_convolve", "frequency_filter"]


@pytest.mark.parametrize("name", AUDIO_CASES)
def test_audio_calls_compiled_equal_eager(name):
    fn, tensors, wrt = _audio_cases()[name]
    _check_compiled_equals_eager(fn, tensors, wrt)


def _opcheck_samples():
    g = _gen(3)
    W = lambda *s: _rand(*s, g=g, lo=0.05, hi=1.0)   # noqa: E731
    P = lambda *s: _rand(*s, g=g)                      # noqa: E731
    A = lambda *s: _rand(*s, g=g, lo=-0.5, hi=0.5)   # noqa: E731
    R = lambda t: t.requires_grad_(True)               # noqa: E731
    F = 1 | 2 | 4 | 8                                  # square, dont_normalize, cutoff, require_sort
    x, y, pos, rp = W(5, 33), W(5, 33), P(33), P(5, 33)
    a3, f0, amps = A(3, 1536), _rand(2, 4, 1, g=g, lo=100.0, hi=400.0), _rand(2, 4, 8, g=g, lo=0.1, hi=1.0)
    env_f, env_a = _rand(2, 512, 8, g=g, lo=100.0, hi=4000.0), _rand(2, 512, 8, g=g)
    grows = W(5)
    return {
        "w1d_rows": [(R(x.clone()), R(y.clone()), R(pos.clone()), R(pos.clone()), 2.0, F), (R(x.clone()), R(y.clone()), R(rp.clone()), R(rp.clone()), 2.0, F),
                     (R(x.clone()), R(W(5, 8)), pos, R(P(5, 8)), 2.0, F)],
        "w1d_rows_backward": [(x, y, pos, pos, 2.0, F, grows, False, True, True), (x, y, rp, rp, 1.0, 8, grows[:1], True, False, True)],
        "w1d_position_grad": [(x, y, pos, pos, 2.0, F, grows, True, True), (x, W(5, 8), pos, P(5, 8), 2.0, F, grows, False, True)],
        "w1d_mean": [(R(x.clone()), R(y.clone()), R(pos.clone()), R(pos.clone()), 2.0, F)],
        "w1d_mean_and_grad": [(x, R(y.clone()), R(pos.clone()), R(pos.clone()), 2.0, F)],
        "row_mean": [(R(W(5)),)],
        "w1d_quantiles": [(R(x.clone()), R(y.clone()), R(pos.clone()), R(pos.clone()), 2.0, F)],
        "w1d_quantiles_backward": [(x, y, pos, pos, 2.0, F, W(5, 66), None, W(5, 66), None, W(5, 33), True, True, True, False)],
        "stft_magnitude": [(R(a3.clone()), "flattop", 256, 64, True), (R(a3.clone()), "", 256, 64, False)],
        "stft_magnitude_backward": [(a3, "", 256, 64, W(3, 24, 129), None, None), (a3, "", 256, 64, W(3, 24, 129), W(1), None)],
        "mss_loss": [(a3, R(A(3, 1536)), [256, 64], 1.0, 0.5, False, False, 1.0, True), (a3, R(A(3, 1536)), [256, 64], 1.0, 0.0, True, True, 0.05, True)],
        "audio_to_loss": [(a3, R(A(3, 1536)), "flattop", 256, 64, 16000.0, 2.0, F, True)],
        "mix_loss_step": [(a3, R(A(3, 1536)), "flattop", P(129), P(129), 256, 64, 2.0, F, [256, 64], 1.0, 0.0, False, 0.05, 1.0, False, True),
                          (a3, R(A(3, 1536)), "flattop", pos_hz(), pos_hz(), 256, 64, 2.0, F, [256, 64], 1.0, 0.0, False, 0.05, 1.0, True, True)],
        "bin_frequencies": [(a3, 256, 16000.0)],
        "unit_frequencies": [(a3, 256, 16000.0)],
        "roll_off_taps": [(a3,)],
        "synth": [(R(f0.clone()), R(amps.clone()), 512, 16000.0, True)],
        "synth_backward": [(f0, amps, 512, 16000.0, True, A(2, 512), True, True)],
        "oscillator_bank": [(R(env_f.clone()), R(env_a.clone()), 16000.0)],
        "oscillator_bank_backward": [(env_f, env_a, 16000.0, A(2, 512), True, True)],
        "fir_same": [(R(A(2, 512)), R(A(2, 128)), 62), (R(A(2, 512)), R(A(128)), 62)],
        "fir_same_backward": [(A(2, 512), A(2, 512), A(2, 128), 62, True, True)],
    }


def pos_hz():
    return torch.fft.rfftfreq(256, d=1.0 / 16000.0).to(device())


def test_opcheck_covers_every_op():
    from sot_amd import ops
    assert sorted(_opcheck_samples()) == sorted(ops.NAMES)


@pytest.mark.parametrize("name", ["w1d_rows", "w1d_rows_backward", "w1d_position_grad", "w1d_mean", "w1d_mean_and_grad", "row_mean", "w1d_quantiles",
                                  "w1d_quantiles_backward", "stft_magnitude", "stft_magnitude_backward", "mss_loss", "audio_to_loss", "mix_loss_step",
                                  "bin_frequencies", "unit_frequencies", "roll_off_taps", "synth", "synth_backward", "oscillator_bank",
                                  "oscillator_bank_backward", "fir_same", "fir_same_backward"])
def test_opcheck(name):
    """torch.library.opcheck with its default utilities: schema (no undeclared mutation or aliasing), autograd registration, fake tensor
    agreement, AOT dispatch (static and dynamic)."""
    native()
    op = getattr(torch.ops.sot_amd, name).default
    for args in _opcheck_samples()[name]:
        torch.library.opcheck(op, args)


def test_export_runs_and_equals_eager():
    from sot_amd.losses import MSSLoss
    native()
    g = _gen(4)
    paper = _paper()
    x, y, pos = _rand(5, 33, g=g, lo=0.05), _rand(5, 33, g=g, lo=0.05), _rand(33, g=g)
    want = paper(x, y, x_pos=pos, y_pos=pos)
    program = torch.export.export(paper, (x, y), {"x_pos": pos, "y_pos": pos})
    assert any("sot_amd" in str(n.target) for n in program.graph.nodes)
    assert torch.equal(program.module()(x, y, x_pos=pos, y_pos=pos), want)
    mss = MSSLoss(fft_sizes=(256, 64), mag_weight=1.0, logmag_weight=0.5).to(device())
    t, v = _rand(3, 1536, g=g, lo=-0.5, hi=0.5), _rand(3, 1536, g=g, lo=-0.5, hi=0.5)
    want = mss(t, v)
    program = torch.export.export(mss, (t, v))
    assert any("sot_amd::mss_loss" in str(n.target) or "sot_amd.mss_loss" in str(n.target) for n in program.graph.nodes)
    assert torch.equal(program.module()(t, v), want)


# ---- the reference trainer's loop, unchanged (trainer.py:206-236): 3 clips of 4096 samples, n_fft 512, MSS sizes (512, 128, 64)

def _trainer_loop(mix, x, x_hat, x_pos, y_pos):
    from sot_amd import spectra
    spec_x, spec_x_hat = spectra.stft_magnitude(x, 512, 128), spectra.stft_magnitude(x_hat, 512, 128)
    terms = []
    for loss_fn, weight in zip(mix.losses, mix.weights):
        a, b = (x, x_hat) if loss_fn.__class__.__name__ == "MSSLoss" else (spec_x, spec_x_hat)
        terms.append((loss_fn(a, b, x_pos=x_pos, y_pos=y_pos) * weight).mean())
    return sum(terms), terms


def _loop_inputs(seed):
    g = _gen(seed)
    pos = torch.fft.rfftfreq(512, d=1.0 / 16000.0).to(device())
    pos = pos / pos.max()
    return _rand(3, 4096, g=g, lo=-0.5, hi=0.5), _rand(3, 4096, g=g, lo=-0.5, hi=0.5), pos, pos.clone()


def _loop_step(fn, mix, x, x_hat, x_pos, y_pos):
    x_hat = x_hat.detach().clone().requires_grad_(True)
    total, terms = fn(mix, x, x_hat, x_pos, y_pos)
    total.backward()
    return total.detach().clone(), [t.detach().clone() for t in terms], x_hat.grad.clone()


def test_trainer_loop_aot_eager():
    native()
    mix = _mix((512, 128, 64))
    inputs = _loop_inputs(5)
    want = _loop_step(_trainer_loop, mix, *inputs)
    got = _loop_step(torch.compile(_trainer_loop, fullgraph=True, backend="aot_eager"), mix, *inputs)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))


def _inductor_or_skip(fn, **kw):
    compiled = torch.compile(fn, fullgraph=True, **kw)

    def first_call(*args):
        try:
            return compiled(*args)
        except Exception as exc:  # noqa: BLE001 -- Inductor needs a working Triton for the torch arithmetic between the ops
            if "triton" in repr(exc).lower() or "inductor" in type(exc).__module__.lower():
                pytest.skip(f"Inductor cannot compile on this machine: {type(exc).__name__}: {str(exc)[:200]}")
            raise
    return compiled, first_call


def _close_under_inductor(got, want):
    """Inductor may contract `a * w1 + b * w2` into one fma: ONE rounding less, at most 2^-24 of the larger product.  The total is held to
    the project's batch-mean tolerance (rtol 1e-6, atol 0: tests/test_gpu_edge.py); the gradient, whose elements are sums of two products
    that may cancel, to 2^-23 of its largest element; each loss's own scalar is one float32 product of an op output, so it is equal."""
    total, terms, grad = got
    assert all(torch.equal(a, b) for a, b in zip(terms, want[1])), "an op's output differs under Inductor"
    torch.testing.assert_close(total, want[0], rtol=1e-6, atol=0)
    assert float((grad - want[2]).abs().max()) <= 2.0 ** -23 * float(want[2].abs().max())


def test_trainer_loop_inductor():
    native()
    mix = _mix((512, 128, 64))
    inputs = _loop_inputs(6)
    want = _loop_step(_trainer_loop, mix, *inputs)
    _, first_call = _inductor_or_skip(_trainer_loop, backend="inductor")
    _close_under_inductor(_loop_step(first_call, mix, *inputs), want)


def test_trainer_loop_reduce_overhead():
    """Four steps of the compiled loop replayed from HIP graphs (mode="reduce-overhead"), each on fresh values copied into the same tensors."""
    native()
    mix = _mix((512, 128, 64))
    x, x_hat, x_pos, y_pos = _loop_inputs(7)
    compiled, first_call = _inductor_or_skip(_trainer_loop, mode="reduce-overhead")
    for step in range(4):
        fresh = _loop_inputs(8 + step)
        x.copy_(fresh[0])
        x_hat.copy_(fresh[1])
        want = _loop_step(_trainer_loop, mix, x, x_hat, x_pos, y_pos)
        torch.compiler.cudagraph_mark_step_begin()
        got = _loop_step(first_call if step == 0 else compiled, mix, x, x_hat, x_pos, y_pos)
        _close_under_inductor(got, want)


def test_eager_calls_never_enter_the_ops():
    """Outside compilation the public calls take the autograd.Function classes and the C++ host path, never sot_amd/ops.py."""
    from sot_amd import ops, spectra
    native()
    mix = _mix()
    g = _gen(9)
    x, x_hat = _rand(3, 1536, g=g, lo=-0.5, hi=0.5), _rand(3, 1536, g=g, lo=-0.5, hi=0.5).requires_grad_(True)
    before = dict(ops.CALLS)
    assert not torch.compiler.is_compiling()
    for fused in (True, False):
        spectra.trainer_loss_step(mix, x, x_hat, n_fft=256, hop=64, fused=fused).backward()
    spectra.sinusoidal_synth(_rand(2, 4, 8, g=g), _rand(2, 4, 1, g=g, lo=100.0, hi=400.0), 512, apply_roll_off=True)
    _paper()(_rand(5, 33, g=g), _rand(5, 33, g=g), x_pos=_rand(5, 33, g=g), y_pos=_rand(33, g=g), return_quantiles=False)
    assert dict(ops.CALLS) == before
