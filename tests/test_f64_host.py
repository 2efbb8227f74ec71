"""CPU: the host side of the float64 route (include/sot_hip.h, ABI 21; csrc/sot_f64.hip) -- the symbols, the size predicate
sot_w1d_f64_supported, the module's gate losses._f64_route_applies on meta tensors, and the input recipe of tests/f64_cases.py that the GPU
tests (tests/test_f64_gpu.py) hold the kernels to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import f64_cases as fc
from conftest import ROOT

RS, PRE = 8, 16    # SOT_FLAG_REQUIRE_SORT, SOT_FLAG_PRENORMALIZED
EXTERN = ("sot_w1d_f64_supported", "sot_w1d_forward_f64", "sot_w1d_backward_f64")
F64 = torch.float64


@pytest.fixture(scope="module")
def nat():
    from sot_amd import _native
    _native.load()
    return _native


def test_header_library_and_binding_agree_on_abi_21(nat):
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    assert int(re.search(r"#define SOT_ABI_VERSION (\d+)", header).group(1)) == nat.ABI_VERSION == nat.load().sot_abi_version() >= 21


def test_new_symbols_are_in_header_binding_and_library(nat):
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    lib = nat.load()
    for name in EXTERN:
        assert re.search(r"^extern int %s\(" % name, header, flags=re.M), name
        assert name in nat.F64_EXPORTS and name not in nat.EXPORTS, name
        assert getattr(lib, name).argtypes == nat.F64_EXPORTS[name][1], name
    assert re.search(r"^size_t sot_w1d_f64_workspace_bytes\(const sot_problem_f64 \*prob\);", header, flags=re.M)
    assert "sot_w1d_f64_workspace_bytes" in nat.EXPORTS
    import sot_amd
    assert ("f64", "sot_f64.hip") in sot_amd.build.OBJECTS
    for name in ("forward_rows_f64", "backward_rows_f64", "f64_supported"):
        assert callable(getattr(nat, name)), name
    # sot_problem_f64: the data fields of sot_problem with a double p, no plan or permutation fields
    names = [f[0] for f in nat.SotProblemF64._fields_]
    assert names == [f[0] for f in nat.SotProblem._fields_][:len(names)] and names[-2:] == ["p", "flags"]
    assert dict(nat.SotProblemF64._fields_)["p"] is ctypes.c_double


def _problem(nat, n, m, flags=0, rowpos=False, B=3, p=2.0, xs=None, ys=None):
    pr = nat.SotProblemF64()
    pr.B, pr.n, pr.m = B, n, m
    pr.x_row_stride, pr.y_row_stride = (n if xs is None else xs), (m if ys is None else ys)
    pr.xpos_row_stride, pr.ypos_row_stride = (n, m) if rowpos else (0, 0)
    pr.p, pr.flags = p, flags
    pr.x = pr.y = pr.xpos = pr.ypos = 4096      # never followed: host arithmetic
    return pr


def test_supported_predicate_on_a_table_of_problems(nat):
    lib = nat.load()
    ok = lambda pr, bwd: lib.sot_w1d_f64_supported(ctypes.byref(pr), bwd)   # noqa: E731
    for rowpos in (False, True):
        assert ok(_problem(nat, 4097, 4097, rowpos=rowpos), 0) == 1          # the forward's stated limit
        assert ok(_problem(nat, 2049, 2049, rowpos=rowpos), 1) == 1          # the backward's
        assert ok(_problem(nat, 1, 1, rowpos=rowpos), 1) == 1
        assert ok(_problem(nat, 1, 8193, rowpos=rowpos), 0) == 1
    # one CU's 160 KiB: 16 (n + m) bytes forward, 24 (n + m) bytes backward, plus the reduction scratch
    assert ok(_problem(nat, 5200, 5200), 0) == 0 and ok(_problem(nat, 4097, 4097), 1) == 0 and ok(_problem(nat, 3500, 3500), 1) == 0
    first = {bwd: next(k for k in range(2, 20000, 2) if not ok(_problem(nat, k // 2, k // 2), bwd)) for bwd in (0, 1)}
    assert first[0] > 8194 and first[1] > 4098, first
    assert all(ok(_problem(nat, k // 2, k // 2), bwd) == 0 for bwd in (0, 1) for k in range(first[bwd], first[bwd] + 64, 2))   # monotone beyond
    for flags in (1, 2, 4, 1 | 2 | 4, PRE, PRE | 4):
        assert ok(_problem(nat, 300, 411, flags), 1) == 1
    # refusals: REQUIRE_SORT, strides, shapes, p, NULL
    assert ok(_problem(nat, 300, 300, RS), 0) == 0 and ok(_problem(nat, 300, 300, RS | 1 | 2 | 4), 1) == 0
    assert ok(_problem(nat, 300, 300, xs=299), 0) == 0 and ok(_problem(nat, 300, 300, ys=12), 0) == 0
    assert ok(_problem(nat, 300, 300, xs=517, ys=301), 0) == 1
    mixed = _problem(nat, 300, 300)
    mixed.xpos_row_stride = 300              # a shared grid against per-row positions: not this ABI's
    assert ok(mixed, 0) == 0
    short = _problem(nat, 300, 300, rowpos=True)
    short.ypos_row_stride = 299
    assert ok(short, 0) == 0
    assert ok(_problem(nat, 0, 300), 0) == 0 and ok(_problem(nat, 300, -1), 0) == 0 and ok(_problem(nat, 300, 300, B=-1), 0) == 0
    assert ok(_problem(nat, 300, 300, p=0.5), 0) == 0 and ok(_problem(nat, 300, 300, p=float("nan")), 0) == 0
    assert lib.sot_w1d_f64_supported(None, 0) == 0 and lib.sot_w1d_f64_supported(None, 1) == 0
    assert lib.sot_w1d_f64_workspace_bytes(None) == 0 and lib.sot_w1d_f64_workspace_bytes(ctypes.byref(_problem(nat, 300, 300))) == 0
    assert nat.f64_supported(4097, 4097) and not nat.f64_supported(4097, 4097, backward=True) and nat.f64_supported(2049, 2049, backward=True)


# ---- the gate, on meta tensors: no device is touched.  A meta tensor is not `is_cuda`, so the gate's device test is patched to take them.

def _meta(*shape, dtype=F64, grad=False):
    return torch.empty(*shape, dtype=dtype, device="meta", requires_grad=grad)


@pytest.fixture()
def gate(monkeypatch, nat):
    from sot_amd import losses
    monkeypatch.setattr(losses, "_is_hip_tensor", lambda t: t.device.type == "meta")
    return losses._f64_route_applies


def test_gate_accepts_float64_rows_on_shared_and_per_row_supports(gate):
    for lead in ((9,), (4, 5)):
        x, y = _meta(*lead, 300), _meta(*lead, 411, grad=True)
        assert gate(x, y, _meta(300), _meta(411))                               # shared 1-D grids
        assert gate(x, y, _meta(*lead, 300), _meta(*lead, 411))                 # per-row positions
        assert gate(x, y, _meta(300).expand(*lead, 300), _meta(411).expand(*lead, 411))   # the stride-0 expansion of one row
    assert gate(_meta(3, 4097), _meta(3, 4097), _meta(4097), _meta(4097))       # forward at its limit, no gradient asked for
    assert gate(_meta(3, 2049, grad=True), _meta(3, 2049, grad=True), _meta(2049), _meta(2049))
    with torch.no_grad():                                                        # the grad mode decides which size limit holds
        assert gate(_meta(3, 4097, grad=True), _meta(3, 4097, grad=True), _meta(4097), _meta(4097))


def test_gate_rejects_everything_else(gate, monkeypatch):
    from sot_amd import losses
    x, y, xp, yp = _meta(9, 300), _meta(9, 300, grad=True), _meta(300), _meta(300)
    assert gate(x, y, xp, yp)
    assert not gate(x, y, xp, yp, return_quantiles=True)
    assert not gate(x, y, _meta(300, dtype=torch.float32), _meta(300, dtype=torch.float32))     # float64 weights on float32 positions
    assert not gate(x.float(), y.float(), xp, yp) and not gate(x, _meta(9, 300, dtype=torch.float32), xp, yp)
    assert not gate(x, y, _meta(300, grad=True), yp) and not gate(x, y, xp, _meta(9, 300, grad=True))   # position gradients
    with torch.no_grad():
        assert gate(x, y, _meta(300, grad=True), yp)                                            # ... which nobody asks for under no_grad
    assert not gate(x, y, xp, _meta(9, 300)) and not gate(x, y, _meta(9, 300), yp)              # mixed supports
    assert not gate(_meta(3, 4097), _meta(3, 4097, grad=True), _meta(4097), _meta(4097))        # beyond the backward's LDS
    assert not gate(_meta(3, 6000), _meta(3, 6000), _meta(6000), _meta(6000))                   # beyond the forward's
    assert not gate(x, y, _meta(299), yp) and not gate(_meta(300), _meta(300), xp, yp) and not gate(x, _meta(8, 300), xp, yp)
    assert not gate(torch.empty(9, 300, dtype=F64), torch.empty(9, 300, dtype=F64), torch.empty(300, dtype=F64), torch.empty(300, dtype=F64))   # CPU
    monkeypatch.setattr(losses, "_compiling", lambda: True)
    assert not gate(x, y, xp, yp)                                                               # a call that is being traced


def test_cpu_tensors_keep_the_composition():
    """existing behaviour: float64 CPU tensors never see the gate's route (no device, no library call)"""
    from sot_amd.losses import Wasserstein1D
    x, y = fc.plain_rows(4, 33, 33, seed=2)
    pos = torch.tensor(fc.grid(33))
    out = Wasserstein1D(p=2, square_dist=True)(torch.tensor(x), torch.tensor(y), x_pos=pos, y_pos=pos.clone())
    assert out.dtype == F64 and not out.is_cuda


# ---- the input recipe (256 x 300, as probed when the recipe was designed)

def _cpu_route(x, y, pos, mode):
    from sot_amd import _torch_path as tp
    kw = fc.mode_kwargs(mode)
    t = torch.tensor
    return tp.module_forward(t(x), t(y), t(pos), t(pos), p=kw["p"], square_dist=kw["square_dist"], dont_normalize=kw["dont_normalize"],
                             limit_quantile_range=kw["limit_quantile_range"], require_sort=True, hinge_on=False, rows_only=True).numpy()


@pytest.mark.parametrize("mode", fc.MODES_CUTOFF, ids=[m[0] for m in fc.MODES_CUTOFF])
def test_recipe_rows_are_insensitive_to_the_order_of_the_prefix_sums(mode):
    B, n = 256, 300
    x, y = fc.cutoff_rows(B, n, n, mode[2], seed=11)
    pos = fc.grid(n)
    k = x * 32
    unit = k * k if mode[2] else k
    mass = unit.sum(1)
    assert (k == np.round(k)).all() and k.min() >= 0 and k.max() <= 31
    assert (np.log2(mass) == np.round(np.log2(mass))).all()                      # the mass the call normalises by is a power of two
    ymass = (y * y).sum(1) / (x * x).sum(1) if mode[2] else y.sum(1) / x.sum(1)
    assert (ymass > 1.19).all() and (ymass < 1.51).all()
    truth = fc.eval_rows(x, y, pos, pos, mode)
    seq = fc.eval_rows(x, y, pos, pos, mode, dtype=np.float64)
    blk = fc.eval_rows(x, y, pos, pos, mode, dtype=np.float64, block=64)
    cpu = _cpu_route(x, y, pos, mode)
    uncut = fc.eval_rows(x, y, pos, pos, mode[:4] + (False,))
    e_scan = float(np.abs(seq - blk).max())
    e_cpu = float(np.abs(cpu - truth).max())
    change = float((np.abs(uncut - truth) / np.abs(uncut)).min())
    print(f"{mode[0]}: sequential vs blocked {e_scan:.3g}, CPU route vs truth {e_cpu:.3g}, smallest relative change by the cutoff {change:.3g}")
    assert e_scan <= 1e-12 and e_cpu <= 1e-12
    assert change >= 1e-2                                                        # the cutoff acts on every row


def test_generic_rows_are_order_sensitive_under_the_cutoff_and_not_without():
    """why the recipe exists: the same two float64 evaluations on generic rows"""
    x, y = fc.plain_rows(64, 300, 300, seed=3)
    pos = fc.grid(300)
    for mode in fc.MODES_PLAIN:
        seq = fc.eval_rows(x, y, pos, pos, mode, dtype=np.float64)
        blk = fc.eval_rows(x, y, pos, pos, mode, dtype=np.float64, block=64)
        assert float(np.abs(seq - blk).max()) <= 1e-13, mode[0]


def test_truth_equals_the_cpu_route_on_small_rows_with_a_zero_mass_row():
    for mode in fc.MODES:
        x, y = fc.rows_for(mode, 5, 17, 17, seed=4, zero_row=2)
        pos = fc.grid(17)
        truth = fc.eval_rows(x, y, pos, pos, mode)
        cpu = _cpu_route(x, y, pos, mode)
        assert float(np.abs(cpu - truth).max()) <= 1e-13 * max(1.0, float(np.abs(truth).max())), mode[0]
