"""CPU: the host side of bfloat16 training (include/sot_hip.h, ABI 20; csrc/sot_bf16_bwd.hip) -- the symbols, the workspace arithmetic of
sot_w1d_bf16_backward_workspace_bytes, the predicate sot_w1d_bf16_native and the module's gate _typed_training_applies.

A NATIVE problem (the typed forward's condition on the problem, without SOT_FLAG_TIE_FREE_GRADIENT) needs exactly the float32 problem's
workspace: no float32 image of a spectrum or of a gradient exists.  Every other problem is widened inside the call and needs room for the
two spectra and for each gradient asked for, as dense float32 rows, on top."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

RS, NS, PRE, TIE_FREE = 8, 32, 16, 256    # SOT_FLAG_REQUIRE_SORT, _NO_SPECIALIZE, _PRENORMALIZED, _TIE_FREE_GRADIENT
EXTERN = ("sot_w1d_bf16_native", "sot_w1d_backward_bf16", "sot_w1d_loss_and_grad_bf16")
BF16 = torch.bfloat16


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


def test_header_library_and_binding_agree_on_abi_20(nat):
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    assert int(re.search(r"#define SOT_ABI_VERSION (\d+)", header).group(1)) == nat.ABI_VERSION == nat.load().sot_abi_version() >= 20


def test_new_symbols_are_in_header_binding_and_library(nat):
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    lib = nat.load()
    for name in EXTERN:
        assert re.search(r"^extern int %s\(" % name, header, flags=re.M), name
        assert name in nat.BF16_TRAIN_EXPORTS and name not in nat.EXPORTS and name not in nat.BF16_EXPORTS, name
        assert getattr(lib, name).argtypes == nat.BF16_TRAIN_EXPORTS[name][1], name
    assert re.search(r"^size_t sot_w1d_bf16_backward_workspace_bytes\(const sot_problem \*prob, int want_grad_x, int want_grad_y\);", header, flags=re.M)
    assert "sot_w1d_bf16_backward_workspace_bytes" in nat.EXPORTS
    # "the signature of sot_w1d_backward with uint16_t* gradients, plus const float* rescale" behind them; "the signature of sot_w1d_loss_and_grad"
    res, args = nat.EXPORTS["sot_w1d_backward"]
    assert nat.BF16_TRAIN_EXPORTS["sot_w1d_backward_bf16"] == (res, args[:6] + [ctypes.c_void_p] + args[6:])
    assert nat.BF16_TRAIN_EXPORTS["sot_w1d_loss_and_grad_bf16"] == nat.EXPORTS["sot_w1d_loss_and_grad"]
    assert "There is no typed backward" not in header
    import sot_amd
    assert ("bf16_bwd", "sot_bf16_bwd.hip") in sot_amd.build.OBJECTS
    for name in ("bf16_native", "backward_rows_bf16", "loss_and_grad_bf16"):
        assert callable(getattr(nat, name)), name


def _sizes(nat, pr, want_x, want_y):
    lib = nat.load()
    return (lib.sot_w1d_bf16_backward_workspace_bytes(ctypes.byref(pr), want_x, want_y), lib.sot_workspace_bytes(ctypes.byref(pr)),
            lib.sot_w1d_bf16_native(ctypes.byref(pr)))


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096])
def test_native_problems_need_the_float32_workspace_and_no_more(nat, n):
    for B in (1, 67, 8192):
        for flags in (RS, RS | 64, RS | 1 | 2 | 4, 0):
            for stride in (n, n + 8, 3 * n):
                for want_x, want_y in ((0, 1), (1, 1), (1, 0)):
                    got, inner, native = _sizes(nat, _problem(nat, B, n, n, flags, stride=stride), want_x, want_y)
                    assert got == inner > 0 and native == 1, (B, flags, stride)


OTHERS = [("bins1025", dict(n=1025, m=1025)), ("bins257", dict(n=257, m=257)), ("bins1000", dict(n=1000, m=1000)),
          ("bins8192", dict(n=8192, m=8192)), ("stride2049", dict(n=2048, m=2048, stride=2049)), ("stride2052", dict(n=2048, m=2048, stride=2052)),
          ("pointer_2_off", dict(n=2048, m=2048, address=4096 + 2)), ("pointer_8_off", dict(n=2048, m=2048, address=4096 + 8)),
          ("rowpos512", dict(n=512, m=512, rowpos=True)), ("no_specialize", dict(n=2048, m=2048, extra=NS)),
          ("prenormalized", dict(n=2048, m=2048, extra=PRE)), ("tie_free_gradient", dict(n=2048, m=2048, extra=TIE_FREE)),
          ("n700_m300", dict(n=700, m=300)), ("n2048_m512", dict(n=2048, m=512))]


@pytest.mark.parametrize("name,kw", OTHERS, ids=[name for name, _ in OTHERS])
def test_every_other_problem_gets_room_for_the_float32_images(nat, name, kw):
    B = 67
    kw = dict(kw)
    flags = RS | kw.pop("extra", 0)
    n, m = kw.pop("n"), kw.pop("m")
    for want_x, want_y in ((0, 1), (1, 1), (1, 0)):
        pr = _problem(nat, B, n, m, flags, **kw)
        got, inner, native = _sizes(nat, pr, want_x, want_y)
        images = 4 * B * (n + m) + 4 * B * (n * want_x + m * want_y)
        assert native == 0
        assert got >= inner + images, (got, inner, images)
        assert got <= inner + images + 4 * 256 + 16      # four images rounded up to 256 bytes, 16 bytes of alignment slack


def test_workspace_and_predicate_are_zero_for_what_they_refuse(nat):
    lib = nat.load()
    assert lib.sot_w1d_bf16_backward_workspace_bytes(None, 1, 1) == 0 and lib.sot_w1d_bf16_native(None) == 0
    for n, m in ((0, 4), (4, 0), (-1, 4), (2048, 0), (0, 2048)):
        for rowpos in (False, True):
            pr = _problem(nat, 3, n, m, RS, rowpos)
            assert lib.sot_w1d_bf16_backward_workspace_bytes(ctypes.byref(pr), 1, 1) == 0, (n, m, rowpos)
            assert lib.sot_w1d_bf16_native(ctypes.byref(pr)) == 0, (n, m, rowpos)


def test_tie_free_flag_means_nothing_to_the_typed_forward(nat):
    """the forward's workspace function keeps reporting by its own predicate: the flag that only the training form reads does not widen it"""
    lib = nat.load()
    pr = _problem(nat, 67, 2048, 2048, RS | TIE_FREE)
    assert lib.sot_w1d_bf16_workspace_bytes(ctypes.byref(pr)) == lib.sot_workspace_bytes(ctypes.byref(pr))


def test_typed_training_gate_on_cpu_stand_ins(nat):
    """_typed_training_applies is a function of dtypes, shapes, strides, requires_grad, the grad mode, the flag word and pointer alignment:
    CPU tensors answer it (torch's CPU allocations are 64-byte aligned)."""
    from sot_amd import losses
    gate = losses._typed_training_applies

    def T(*shape, dtype=BF16, grad=False):
        return torch.zeros(*shape, dtype=dtype).requires_grad_(grad)

    pos = torch.linspace(0, 1, 2048)
    x, y = T(6, 2048), T(6, 2048, grad=True)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    assert gate(x, y, pos, pos.clone())                                             # the training step
    assert gate(T(6, 2048, grad=True), y, pos, pos)                                 # both operands differentiated
    assert gate(T(2, 3, 2048), T(2, 3, 2048, grad=True), pos, pos)                  # [batch, time, bins]
    assert gate(x, y, pos, pos, False, RS | 1 | 2 | 4, 2.0)                         # the paper's flags
    for n in (512, 1024, 4096):
        assert gate(T(3, n), T(3, n, grad=True), torch.linspace(0, 1, n), torch.linspace(0, 1, n)), n
    wide = T(6, 2056)
    assert gate(wide[:, :2048], y, pos, pos)                                        # rows 2048 + 8 elements apart
    # ... and what keeps the widening route
    assert not gate(x, T(6, 2048), pos, pos)                                        # nothing requires a gradient
    with torch.no_grad():
        assert not gate(x, y, pos, pos)
    assert not gate(x.float(), T(6, 2048, dtype=torch.float32, grad=True), pos, pos)
    assert not gate(x, y, pos.clone().requires_grad_(True), pos) and not gate(x, y, pos, pos.clone().requires_grad_(True))
    assert not gate(x, y, pos, pos, True)                                           # return_quantiles
    assert not gate(x, y, pos, pos, False, RS | TIE_FREE)                           # the opt-in merge-free training form
    assert not gate(x, y, pos, pos, False, RS | PRE)
    for n in (1025, 257, 1000, 8192):
        assert not gate(T(3, n), T(3, n, grad=True), torch.linspace(0, 1, n), torch.linspace(0, 1, n)), n
    assert not gate(T(6, 512), T(6, 2048, grad=True), torch.linspace(0, 1, 512), pos)   # n != m
    rowpos = torch.rand(6, 2048)
    assert not gate(x, y, rowpos, rowpos.clone())                                   # per-row positions
    assert not gate(x, y, pos, rowpos)                                              # mixed supports
    odd = T(6, 2049)
    assert not gate(odd[:, :2048], y, pos, pos)                                     # rows alternately 2 bytes off
    assert not gate(odd[:, 1:], y, pos, pos)                                        # a pointer 2 bytes off
    # meta stand-ins answer too: shapes and strides only, no storage
    xm, ym = torch.empty(6, 2048, dtype=BF16, device="meta"), torch.empty(6, 2048, dtype=BF16, device="meta", requires_grad=True)
    pm = torch.empty(2048, device="meta")
    assert gate(xm, ym, pm, pm)
    assert not gate(torch.empty(6, 1025, dtype=BF16, device="meta"), torch.empty(6, 1025, dtype=BF16, device="meta", requires_grad=True),
                    torch.empty(1025, device="meta"), torch.empty(1025, device="meta"))
