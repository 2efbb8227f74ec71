"""torch.compile support without a GPU: the sot_amd:: custom ops exist with the schemas INTEGRATION.md documents, and every public call
traces into ONE graph (torch._dynamo.export raises on a graph break) on fake GPU tensors -- `torch.empty(..., device="cuda")` under
FakeTensorMode needs no device.  The backward formulas are traced the same way: they hold only sot_amd:: and aten ops.  (The autograd
engine itself refuses fake GPU tensors on a machine without a device, so the formulas registered in ops.AUTOGRAD are called directly
here; torch.library.opcheck with all its utilities runs on the real device in tests/test_compile_gpu.py.)"""
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.proxy_tensor import make_fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_PAPER = 1 | 2 | 4 | 8   # square_dist, dont_normalize, limit_quantile_range, require_sort (include/sot_hip.h)


@pytest.fixture(autouse=True)
def _fresh_dynamo():
    torch._dynamo.reset()
    yield
    torch._dynamo.reset()


def E(*shape):
    return torch.empty(*shape, device="cuda")


def _documented_schemas():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## 3. torch.compile / torch.export"):]
    return dict(re.findall(r"^\| `(\w+)` \| `(\(.*?\) -> .*?)` \|", section, flags=re.M))


def test_ops_exist_with_the_documented_schemas():
    from sot_amd import ops
    documented = _documented_schemas()
    assert sorted(documented) == sorted(ops.NAMES)
    for name, schema in documented.items():
        op = getattr(torch.ops.sot_amd, name).default
        assert str(op._schema) == f"sot_amd::{name}{schema}", name
        assert not op._schema.is_mutable, name   # mutates_args=()
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sot_amd::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"sot_amd::{name}", "CPU")
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sot_amd::{name}", "Meta"), f"{name}: no fake implementation"
    for name in ops.AUTOGRAD:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sot_amd::{name}", "Autograd"), name


def _sot_ops(gm):
    return [str(n.target).split(".")[1] for n in gm.graph.nodes if n.op == "call_function" and str(n.target).startswith("sot_amd.")]


def _paper():
    from sot_amd.losses import Wasserstein1D
    return Wasserstein1D(p=2, dont_normalize=True, limit_quantile_range=True, square_dist=True)


def _mix():
    from sot_amd.losses import MixOfLosses, MSSLoss, Wasserstein1D
    return MixOfLosses([MSSLoss(fft_sizes=(256, 64), loss_type="L1", mag_weight=1, logmag_weight=0),
                        Wasserstein1D(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True, require_sort=True)], [0.05, 1])


def _public_cases():
    """name -> (callable, positional tensors, keyword arguments, the sot_amd:: ops of the graph, the output shapes)"""
    from sot_amd import spectra
    from sot_amd.losses import KL, MixOfLosses, MSSLoss, Wasserstein1D, Wasserstein1DWithTransform, wasserstein_1d
    paper, mix = _paper(), _mix()
    x, y, pos = E(5, 33), E(5, 33).requires_grad_(True), E(33)
    a, b = E(3, 1536), E(3, 1536).requires_grad_(True)
    audio_in = Wasserstein1DWithTransform(p=2, transform_kwargs={"type": "stft", "n_fft": 256, "hop_length": 64, "log": True})
    return {
        "shared_grid": (paper, (x, y), dict(x_pos=pos, y_pos=pos), ["w1d_mean_and_grad"], [()]),
        "shared_grid_257_no_grad": (paper, (E(5, 257), E(5, 257)), dict(x_pos=E(257), y_pos=E(257)), ["w1d_mean"], [()]),
        "per_row_positions": (paper, (x, y), dict(x_pos=E(5, 33), y_pos=E(5, 33)), ["w1d_mean_and_grad"], [()]),
        "mixed_supports": (paper, (E(5, 33), E(5, 8)), dict(x_pos=pos, y_pos=E(5, 8)), ["w1d_rows", "row_mean"], [()]),
        "hinge": (Wasserstein1D(p=1, hinge=True), (x, y), dict(x_pos=pos, y_pos=pos, hinge=0.1), ["w1d_rows", "row_mean"], [()]),
        "dims": (paper, (E(2, 3, 33), E(2, 3, 33)), dict(x_pos=pos, y_pos=pos, dims=1), ["w1d_rows"], [(2,)]),
        "return_quantiles": (paper, (x, y), dict(x_pos=pos, y_pos=pos, return_quantiles=True), ["w1d_quantiles"],
                             [(5, 66), (5, 66), (5, 66), (5, 33), (5, 33)]),
        "row_losses": (paper.row_losses, (x, y), dict(x_pos=pos, y_pos=pos), ["w1d_rows"], [(5,)]),
        "wasserstein_1d": (wasserstein_1d, (E(5, 33), E(5, 33), x, y, 2), {}, ["w1d_rows"], [(5,)]),
        "mss": (MSSLoss(fft_sizes=(256, 64), mag_weight=1.0), (a, b), {}, ["mss_loss"], [()]),
        "mss_per_clip": (MSSLoss(fft_sizes=(256, 64), mag_weight=1.0), (a, b), dict(dims=(1, 2)), ["mss_loss"], [(3,)]),
        "stft_magnitude": (lambda t: spectra.stft_magnitude(t, n_fft=256, hop=64), (a,), {}, ["stft_magnitude"], [(3, 24, 129)]),
        "trainer_loss_step": (lambda s, t: spectra.trainer_loss_step(mix, s, t, n_fft=256, hop=64), (a, b), {}, ["bin_frequencies", "mix_loss_step"], [()]),
        "trainer_loss_step_modules": (lambda s, t: spectra.trainer_loss_step(mix, s, t, n_fft=256, hop=64, fused=False), (a, b), {},
                                      ["bin_frequencies", "stft_magnitude", "stft_magnitude", "mss_loss", "w1d_mean_and_grad"], [()]),
        "training_step_slice": (lambda s, t: spectra.training_step_slice(paper, s, t, n_fft=256, hop=64), (a, b), {}, ["audio_to_loss"], [()]),
        "audio_in_module_log": (audio_in, (a, b), {}, ["stft_magnitude", "stft_magnitude", "unit_frequencies", "w1d_mean_and_grad"], [()]),
        "mix_of_losses": (MixOfLosses([paper, KL()], [0.5, 2.0]), (x, y), dict(x_pos=pos, y_pos=pos), ["w1d_mean_and_grad"], [(), ()]),
        "sinusoidal_synth": (lambda amp, f0: spectra.sinusoidal_synth(amp, f0, 512), (E(2, 4, 8), E(2, 4, 1)), {}, ["synth"], [(2, 512)]),
        "sinusoidal_synth_roll_off": (lambda amp, f0: spectra.sinusoidal_synth(amp, f0, 512, apply_roll_off=True), (E(2, 4, 8), E(2, 4, 1)), {},
                                      ["synth", "roll_off_taps", "fir_same"], [(2, 512)]),
        "oscillator_bank": (lambda f, amp: spectra.oscillator_bank(f, amp), (E(2, 512, 8), E(2, 512, 8)), {}, ["oscillator_bank"], [(2, 512)]),
        "fft_convolve": (lambda s, t: spectra.fft_convolve(s, t), (E(2, 512), E(2, 128)), {}, ["fir_same"], [(2, 512)]),
        "frequency_filter": (lambda s, m: spectra.frequency_filter(s, m), (E(2, 512), E(2, 65)), {}, ["fir_same"], [(2, 512)]),
    }


PUBLIC_CASES = ["shared_grid", "shared_grid_257_no_grad", "per_row_positions", "mixed_supports", "hinge", "dims", "return_quantiles", "row_losses",
                "wasserstein_1d", "mss", "mss_per_clip", "stft_magnitude", "trainer_loss_step", "trainer_loss_step_modules", "training_step_slice",
                "audio_in_module_log", "mix_of_losses", "sinusoidal_synth", "sinusoidal_synth_roll_off", "oscillator_bank", "fft_convolve",
                "frequency_filter"]


@pytest.mark.parametrize("name", PUBLIC_CASES)
def test_public_call_traces_into_one_graph(name):
    with FakeTensorMode(allow_non_fake_inputs=True):
        fn, args, kwargs, want_ops, want_shapes = _public_cases()[name]
        gm, _ = torch._dynamo.export(fn)(*args, **kwargs)   # one graph or an error: export does not split
        assert _sot_ops(gm) == want_ops
        out = gm(*args, **kwargs)
        out = list(out.values()) if isinstance(out, dict) else out   # MixOfLosses: {class name: weighted loss}
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        assert [tuple(o.shape) for o in outs] == want_shapes
        assert all(o.dtype == torch.float32 and o.device.type == "cuda" for o in outs)


def test_public_cases_are_all_listed():
    with FakeTensorMode(allow_non_fake_inputs=True):
        assert sorted(_public_cases()) == sorted(PUBLIC_CASES)


class _Ctx:
    """What a formula registered with register_autograd uses of its context."""

    def __init__(self, needs_input_grad):
        self.needs_input_grad = needs_input_grad
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def set_materialize_grads(self, value):
        pass

    def mark_non_differentiable(self, *tensors):
        pass


def _backward_cases():
    """name -> (op, arguments, indices of the differentiated inputs, which outputs receive an upstream gradient (None = all))"""
    x, y, pos, rows = E(5, 33), E(5, 33), E(33), E(5, 33)
    a, b = E(3, 1536), E(3, 1536)
    return {
        "rows_shared": ("w1d_rows", (x, y, pos, pos, 2.0, F_PAPER), (0, 1, 2, 3), None),
        "rows_per_row": ("w1d_rows", (x, y, rows, rows, 2.0, F_PAPER), (0, 1, 2, 3), None),
        "rows_mixed": ("w1d_rows", (x, E(5, 8), pos, E(5, 8), 2.0, F_PAPER), (0, 1, 3), None),
        "mean": ("w1d_mean", (E(5, 257), E(5, 257), E(257), E(257), 2.0, F_PAPER), (0, 1, 2, 3), None),
        "mean_and_grad": ("w1d_mean_and_grad", (x, y, pos, pos, 2.0, F_PAPER), (1, 2, 3), None),
        "row_mean": ("row_mean", (E(5),), (0,), None),
        "quantiles": ("w1d_quantiles", (x, y, pos, pos, 2.0, F_PAPER), (0, 1, 2, 3), None),
        "quantiles_two_used": ("w1d_quantiles", (x, y, rows, rows, 2.0, F_PAPER), (0, 1, 2, 3), (0, 4)),
        "stft": ("stft_magnitude", (a, "flattop", 256, 64, True), (0,), (0,)),
        "stft_no_spectrum": ("stft_magnitude", (a, "", 256, 64, False), (0,), (0,)),
        "mss": ("mss_loss", (a, b, [256, 64], 1.0, 0.0, False, False, 1.0, True), (1,), (0,)),
        "mss_per_clip": ("mss_loss", (a, b, [256, 64], 1.0, 0.0, False, True, 1.0, True), (1,), (0,)),
        "audio_to_loss": ("audio_to_loss", (a, b, "flattop", 256, 64, 16000.0, 2.0, F_PAPER, True), (1,), (0,)),
        "mix_loss_step": ("mix_loss_step", (a, b, "flattop", E(129), E(129), 256, 64, 2.0, F_PAPER, [256, 64], 1.0, 0.0, False, 0.05, 1.0, True, True),
                          (1,), (0,)),
        "synth": ("synth", (E(2, 4, 1), E(2, 4, 8), 512, 16000.0, True), (0, 1), None),
        "oscillator_bank": ("oscillator_bank", (E(2, 512, 8), E(2, 512, 8), 16000.0), (0, 1), None),
        "fir": ("fir_same", (E(2, 512), E(2, 128), 62), (0, 1), None),
        "fir_shared_filter": ("fir_same", (E(2, 512), E(128), 62), (0, 1), None),
    }


BACKWARD_CASES = ["rows_shared", "rows_per_row", "rows_mixed", "mean", "mean_and_grad", "row_mean", "quantiles", "quantiles_two_used", "stft",
                  "stft_no_spectrum", "mss", "mss_per_clip", "audio_to_loss", "mix_loss_step", "synth", "oscillator_bank", "fir", "fir_shared_filter"]


@pytest.mark.parametrize("name", BACKWARD_CASES)
def test_backward_formula_traces_to_package_and_aten_ops(name):
    from sot_amd import ops
    with FakeTensorMode(allow_non_fake_inputs=True):
        op_name, args, wrt, used = _backward_cases()[name]
        setup, backward = ops.AUTOGRAD[op_name]
        tensors = [t for t in args if isinstance(t, torch.Tensor)]

        def forward_and_backward(*ts):
            it = iter(ts)
            full = tuple(next(it) if isinstance(v, torch.Tensor) else v for v in args)
            out = getattr(torch.ops.sot_amd, op_name)(*full)
            ctx = _Ctx(tuple(i in wrt for i in range(len(full))))
            setup(ctx, full, out)
            outs = out if isinstance(out, tuple) else (out,)
            grads = [torch.ones_like(o) if (used is None or k in used) else None for k, o in enumerate(outs)]
            result = backward(ctx, *grads)
            assert len(result) == len(full)
            for i, (grad, value) in enumerate(zip(result, full)):
                assert (grad is not None) == (i in wrt), f"input {i}"
                if grad is not None:
                    assert grad.shape == value.shape and grad.dtype == torch.float32 and grad.device == value.device, f"input {i}"
            return [grad for grad in result if grad is not None]

        gm = make_fx(forward_and_backward, tracing_mode="fake")(*tensors)
        targets = {str(n.target) for n in gm.graph.nodes if n.op == "call_function"}
        foreign = {t for t in targets if not t.startswith(("sot_amd.", "aten.")) and "getitem" not in t}
        assert not foreign, foreign
        assert sum(t.startswith("sot_amd.") for t in targets) >= 1


def test_backward_cases_cover_every_differentiable_op():
    from sot_amd import ops
    with FakeTensorMode(allow_non_fake_inputs=True):
        cases = _backward_cases()
    assert sorted(cases) == sorted(BACKWARD_CASES)
    assert {op for op, *_ in cases.values()} == set(ops.AUTOGRAD)


def test_one_trace_serves_two_batch_sizes():
    paper = _paper()
    with FakeTensorMode(allow_non_fake_inputs=True):
        x, y, pos = E(5, 33), E(5, 33), E(33)
        torch._dynamo.mark_dynamic(x, 0)
        torch._dynamo.mark_dynamic(y, 0)
        gm, _ = torch._dynamo.export(lambda x, y, pos: paper.row_losses(x, y, x_pos=pos, y_pos=pos))(x, y, pos)
        assert _sot_ops(gm) == ["w1d_rows"]
        for batch in (5, 7):   # the same graph module: symbolic output length
            assert tuple(gm(E(batch, 33), E(batch, 33), pos).shape) == (batch,)
        sizes = [n.meta["example_value"].shape for n in gm.graph.nodes if n.op == "call_function" and "w1d_rows" in str(n.target)]
        assert sizes and not isinstance(sizes[0][0], int), "the batch dimension was specialised"


@pytest.mark.parametrize("samples,n_fft,hop", [(1536, 256, 64), (200, 64, 16), (4096, 2048, 512)])
def test_fake_stft_frame_count_is_the_librarys(samples, n_fft, hop):
    from sot_amd import _native as nat, spectra
    frames = int(nat.load().sot_stft_frames(samples, hop))
    with FakeTensorMode(allow_non_fake_inputs=True):
        audio = E(5, samples)
        torch._dynamo.mark_dynamic(audio, 0)
        gm, _ = torch._dynamo.export(lambda a: spectra.stft_magnitude(a, n_fft, hop))(audio)
        for batch in (5, 7):
            assert tuple(gm(E(batch, samples)).shape) == (batch, frames, n_fft // 2 + 1)
