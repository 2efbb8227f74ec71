"""CPU: the host side of the bfloat16 entry points (include/sot_hip.h, ABI 19) -- the symbols, the workspace arithmetic of
sot_w1d_bf16_workspace_bytes, and the numpy model of the narrowing (tests/bf16_model.py) against torch's own conversion.

A NATIVE problem (shared positions, n == m in {512, 1024, 2048, 4096}, 16-byte aligned rows, kernels with the length at compile time
allowed) needs exactly the float32 problem's workspace: no widened copy exists.  Every other problem is widened inside the call and needs
room for two dense float32 copies on top."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bf16_model as bm
from conftest import ROOT

RS, NS, PRE = 8, 32, 16    # SOT_FLAG_REQUIRE_SORT, SOT_FLAG_NO_SPECIALIZE, SOT_FLAG_PRENORMALIZED
NEW = ("sot_rows_bf16_to_f32", "sot_rows_f32_to_bf16", "sot_w1d_forward_bf16", "sot_w1d_loss_bf16")


@pytest.fixture(scope="module")
def nat():
    from sot_amd import _native
    _native.load()
    return _native


def _problem(nat, B, n, m, flags, rowpos=False, stride=None, address=4096):
    pr = nat.SotProblem()
    pr.B, pr.n, pr.m = B, n, m
    pr.x_row_stride, pr.y_row_stride = (n, m) if stride is None else (stride, stride)
    pr.xpos_row_stride, pr.ypos_row_stride = (n, m) if rowpos else (0, 0)
    pr.p, pr.flags = 2.0, flags
    pr.x = pr.y = address        # never followed: host arithmetic (the alignment of the address is part of it)
    pr.xpos = pr.ypos = 4096
    return pr


def test_header_library_and_binding_agree_on_abi_19(nat):
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    assert int(re.search(r"#define SOT_ABI_VERSION (\d+)", header).group(1)) == nat.ABI_VERSION == nat.load().sot_abi_version() >= 19


def test_new_symbols_are_in_header_binding_and_library(nat):
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    lib = nat.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in nat.BF16_EXPORTS and name not in nat.EXPORTS, name
        assert getattr(lib, name).argtypes == nat.BF16_EXPORTS[name][1], name
    assert re.search(r"^size_t sot_w1d_bf16_workspace_bytes\(", header, flags=re.M)
    assert "sot_w1d_bf16_workspace_bytes" in nat.EXPORTS
    assert nat.BF16_EXPORTS["sot_w1d_loss_bf16"] == nat.EXPORTS["sot_w1d_loss"]          # "with the signature of sot_w1d_loss"
    assert nat.BF16_EXPORTS["sot_w1d_forward_bf16"] == nat.EXPORTS["sot_w1d_forward"]
    import sot_amd
    assert ("bf16", "sot_bf16.hip") in sot_amd.build.OBJECTS


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096])
def test_native_problems_need_the_float32_workspace_and_no_more(nat, n):
    lib = nat.load()
    for B in (1, 67, 8192):
        for flags in (RS, RS | 64, RS | 1 | 2 | 4, 0):
            for stride in (n, n + 8, 3 * n):
                pr = _problem(nat, B, n, n, flags, stride=stride)
                assert lib.sot_w1d_bf16_workspace_bytes(ctypes.byref(pr)) == lib.sot_workspace_bytes(ctypes.byref(pr)) > 0, (B, flags, stride)


def _widened_at_least(nat, pr):
    lib = nat.load()
    got, inner = lib.sot_w1d_bf16_workspace_bytes(ctypes.byref(pr)), lib.sot_workspace_bytes(ctypes.byref(pr))
    assert got >= inner + 4 * pr.B * (pr.n + pr.m), (got, inner)
    assert got <= inner + 4 * pr.B * (pr.n + pr.m) + 2 * 256 + 16      # two copies rounded up to 256 bytes, 16 bytes of alignment slack
    return got


def test_every_other_problem_gets_room_for_two_float32_copies(nat):
    B = 67
    _widened_at_least(nat, _problem(nat, B, 1025, 1025, RS))                     # one-sided spectrum: rows of odd length
    _widened_at_least(nat, _problem(nat, B, 257, 257, RS))
    _widened_at_least(nat, _problem(nat, B, 1000, 1000, RS))                     # run-time length
    _widened_at_least(nat, _problem(nat, B, 8192, 8192, RS))                     # not instantiated for 16-bit rows
    _widened_at_least(nat, _problem(nat, B, 2048, 2048, RS, stride=2049))        # rows alternately 2 bytes off
    _widened_at_least(nat, _problem(nat, B, 2048, 2048, RS, stride=2052))        # a stride that is no multiple of 8 elements
    _widened_at_least(nat, _problem(nat, B, 2048, 2048, RS, address=4096 + 2))   # a pointer 2 bytes off
    _widened_at_least(nat, _problem(nat, B, 2048, 2048, RS, address=4096 + 8))
    _widened_at_least(nat, _problem(nat, B, 512, 512, RS, rowpos=True))          # per-row positions
    _widened_at_least(nat, _problem(nat, B, 2048, 2048, RS | NS))                # generic kernels asked for
    _widened_at_least(nat, _problem(nat, B, 2048, 2048, RS | PRE))               # the functional form: weights as given
    _widened_at_least(nat, _problem(nat, B, 700, 300, RS))                       # n != m
    _widened_at_least(nat, _problem(nat, B, 2048, 512, RS))


def test_workspace_is_zero_for_what_it_refuses(nat):
    lib = nat.load()
    assert lib.sot_w1d_bf16_workspace_bytes(None) == 0
    for n, m in ((0, 4), (4, 0), (-1, 4), (2048, 0)):
        for rowpos in (False, True):
            assert lib.sot_w1d_bf16_workspace_bytes(ctypes.byref(_problem(nat, 3, n, m, RS, rowpos))) == 0, (n, m, rowpos)


def _torch_narrow(values):
    return torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _assert_same_bf16(got, want):
    got_nan, want_nan = bm.is_nan_bits(got), bm.is_nan_bits(want)
    assert np.array_equal(got_nan, want_nan)                      # NaN stays NaN and nothing else becomes one
    assert np.array_equal(got[~got_nan], want[~want_nan])


def test_model_of_the_narrowing_equals_torch_on_the_adversarial_values():
    values = bm.adversarial_values()
    got = bm.narrow(values)
    _assert_same_bf16(got, _torch_narrow(values))
    by_bits = dict(zip(bm.adversarial_bits().tolist(), got.tolist()))
    assert by_bits[0x3F808000] == 0x3F80 and by_bits[0x3F818000] == 0x3F82          # ties go to the even neighbour
    assert by_bits[0x3F807FFF] == 0x3F80 and by_bits[0x3F808001] == 0x3F81
    assert by_bits[0x7F7FFFFF] == 0x7F80 and by_bits[0xFF7FFFFF] == 0xFF80          # the largest finite float32 -> infinity
    assert by_bits[0x7F7F7FFF] == 0x7F7F
    assert by_bits[0x00008000] == 0x0000 and by_bits[0x00018000] == 0x0002 and by_bits[0x007FFFFF] == 0x0080   # subnormals
    assert by_bits[0x00000000] == 0x0000 and by_bits[0x80000000] == 0x8000          # signed zeros
    assert by_bits[0x7F800000] == 0x7F80 and by_bits[0xFF800000] == 0xFF80          # infinities are kept
    for nan in (0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0xFF800001):
        assert bm.is_nan_bits(by_bits[nan]), hex(nan)


def test_model_of_the_narrowing_equals_torch_on_random_bit_patterns():
    values = bm.random_values(200_000, 7)
    _assert_same_bf16(bm.narrow(values), _torch_narrow(values))


def test_widening_is_exact_and_narrowing_inverts_it():
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)        # every bfloat16
    wide = bm.widen(bits)
    want = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.array_equal(wide.view(np.uint32), want.view(np.uint32))
    back = bm.narrow(wide)
    nan = bm.is_nan_bits(bits)
    assert np.array_equal(back[~nan], bits[~nan]) and bm.is_nan_bits(back[nan]).all()


def test_gate_refuses_half_and_mixes_without_a_gpu():
    """The dtype gate is plain Python on dtypes and devices: fake GPU tensors show it without a device."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from sot_amd import losses
    with FakeTensorMode():
        def T(dtype, *shape):
            return torch.empty(*shape, device="cuda", dtype=dtype)
        pos = T(torch.float32, 64)
        assert losses._hip_domain(T(torch.float32, 3, 64), T(torch.float32, 3, 64), pos, pos)
        assert losses._hip_domain(T(torch.bfloat16, 3, 64), T(torch.bfloat16, 3, 64), pos, pos)
        for dx, dy in ((torch.float16, torch.float16), (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float16)):
            with pytest.raises(TypeError, match=r"sot_amd computes in float32; got torch\.(b?float16) \(convert with \.float\(\)\)"):
                losses._hip_domain(T(dx, 3, 64), T(dy, 3, 64), pos, pos)
        with pytest.raises(TypeError, match="sot_amd computes in float32"):       # positions stay float32
            losses._hip_domain(T(torch.bfloat16, 3, 64), T(torch.bfloat16, 3, 64), T(torch.bfloat16, 64), pos)


def test_bf16_ops_exist_with_fakes_and_autograd():
    from sot_amd import ops
    assert set(ops.BF16_NAMES) == set(ops.BF16_AUTOGRAD) and not set(ops.BF16_NAMES) & set(ops.NAMES)
    for name in ops.BF16_NAMES:
        op = getattr(torch.ops.sot_amd, name).default
        assert not op._schema.is_mutable, name
        for key in ("CUDA", "Meta", "Autograd"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sot_amd::{name}", key), (name, key)
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"sot_amd::{name}", "CPU"), name
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(5, 64, device="cuda", dtype=torch.bfloat16)
        pos = torch.empty(64, device="cuda")
        wide = torch.ops.sot_amd.rows_to_f32(x)
        assert wide.dtype is torch.float32 and wide.shape == x.shape
        assert torch.ops.sot_amd.rows_to_bf16(wide).dtype is torch.bfloat16
        rows = torch.ops.sot_amd.w1d_rows_bf16(x, x, pos, pos, 2.0, 15)
        assert rows.dtype is torch.float32 and rows.shape == (5,)
        mean = torch.ops.sot_amd.w1d_mean_bf16(x, x, pos, pos, 1.0, 8)
        assert mean.dtype is torch.float32 and mean.shape == ()


def test_a_bfloat16_call_traces_into_one_graph_without_a_gpu():
    """torch.compile(fullgraph=True)'s front end on fake GPU tensors: no graph break, the typed op when no gradient is asked for, the
    widening op in front of the float32 ops when one is."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from sot_amd.losses import Wasserstein1D
    mod = Wasserstein1D(p=1)

    def sot_ops(gm):
        return [str(n.target).split(".")[1] for n in gm.graph.nodes if n.op == "call_function" and str(n.target).startswith("sot_amd.")]

    def B16(*shape, grad=False):
        return torch.empty(*shape, device="cuda", dtype=torch.bfloat16, requires_grad=grad)

    def cases():
        return [((B16(64, 2048), B16(64, 2048)), {}, mod, ["w1d_mean_bf16"]),
                ((B16(64, 2048), B16(64, 2048, grad=True)), {}, mod, ["rows_to_f32", "rows_to_f32", "w1d_mean_and_grad"]),
                ((B16(2, 3, 257), B16(2, 3, 257)), dict(dims=1), mod, ["w1d_rows_bf16"]),
                ((B16(5, 257), B16(5, 257)), {}, mod.row_losses, ["w1d_rows_bf16"]),
                ((B16(5, 257), B16(5, 257)), dict(return_quantiles=True), mod, ["rows_to_f32", "rows_to_f32", "w1d_quantiles"])]

    for k in range(5):
        torch._dynamo.reset()
        with FakeTensorMode(allow_non_fake_inputs=True):
            args, kwargs, fn, want = cases()[k]
            pos = torch.empty(args[0].shape[-1], device="cuda")
            gm, _ = torch._dynamo.export(fn)(*args, x_pos=pos, y_pos=pos, **kwargs)   # one graph or an error: export does not split
            assert sot_ops(gm) == want, (want, sot_ops(gm))
            out = gm(*args, x_pos=pos, y_pos=pos, **kwargs)
            outs = list(out) if isinstance(out, (list, tuple)) else [out]
            assert all(o.dtype == torch.float32 for o in outs)
    torch._dynamo.reset()
