"""Gradients of the five `return_quantiles` tensors on the HIP route (sot_w1d_quantiles_backward, losses._Quantiles).

Yardstick: the package's own CPU float32 route (sot_amd/_torch_path.py under torch autograd), which tests/test_cpu_path.py pins to
the reference.  The loss is sum_t <t, w_t> over the five outputs with seeded random w_t; x.grad, y.grad, x_pos.grad and y_pos.grad
are compared under the project's rule for SOT gradients (tests/test_gpu_parity.py, lines 5-9): per row within 1e-5 of that row's
largest |entry|, per tensor for a position row shared by all batch rows.  The random cases assert on the CPU side that the merged
levels hold no exactly tied neighbours and that no row holds two equal positions, so the comparison is never about the order
`torch.sort` gives to ties (the CPU sort is not stable beyond 16 elements; the HIP sorts are).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

RTOL = 1e-5
NAMES = ("uq", "vq", "Q", "U", "V")
ALL = (0, 1, 2, 3, 4)


# ---- inputs (CPU, seeded) ------------------------------------------------------------------------------------------------------
def make_inputs(shape, pos_kind, seed):
    """Positive uniform weights and positions of the given kind; `shape` is (B, n, m) or (B1, B2, n, m) for 3-D inputs."""
    *lead, n, m = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*lead, n, generator=g) + 0.01
    y = torch.rand(*lead, m, generator=g) + 0.01
    def distinct(width, *batch):
        # one point per cell of a grid of `width` cells, jittered and shuffled: no two positions of a row are equal (torch.sort gives
        # equal positions an order of its own choosing on the CPU; the HIP sort is stable)
        order = torch.argsort(torch.rand(*batch, width, generator=g), -1)
        return (order + 0.5 * torch.rand(*batch, width, generator=g)) / width

    if pos_kind == "fixed_x":
        assert n == m
        xp = yp = None
    elif pos_kind == "shared_unsorted":
        xp, yp = distinct(n), distinct(m)
    elif pos_kind == "rows_unsorted":
        xp, yp = distinct(n, *lead), distinct(m, *lead)
    elif pos_kind == "rows_sorted":
        xp, yp = torch.sort(distinct(n, *lead), -1)[0], torch.sort(distinct(m, *lead), -1)[0]
    else:
        raise ValueError(pos_kind)
    ws = [torch.randn(*lead, k, generator=g) for k in (n + m, n + m, n + m, n, m)]
    return x, y, xp, yp, ws


def quantile_call(mode, x, y, xp, yp):
    """The five tensors through the public interface, on whatever device the inputs live."""
    from sot_amd.losses import Wasserstein1D, wasserstein_1d
    if mode == "functional":   # weights used as given (prenormalized); a shared position row goes in as the reference's stride-0 expand
        u = xp if xp.ndim == x.ndim else xp.unsqueeze(0).expand_as(x)
        v = yp if yp.ndim == y.ndim else yp.unsqueeze(0).expand_as(y)
        return wasserstein_1d(u, v, x, y, p=1, return_quantiles=True)
    kw = dict(p=1) if mode == "p1" else dict(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True)
    mod = Wasserstein1D(fixed_x=x.shape[-1] if xp is None else None, **kw).to(x.device)
    if xp is None:
        return mod(x, y, return_quantiles=True)
    return mod(x, y, x_pos=xp, y_pos=yp, return_quantiles=True)


def run(device, mode, inputs, which, req):
    """Gradients of sum_{t in which} <out_t, w_t> w.r.t. the inputs named in `req`; None where nothing flows."""
    x, y, xp, yp, ws = inputs
    leaves = {"x": x, "y": y, "xp": xp, "yp": yp}
    leaves = {k: (None if v is None else v.detach().clone().to(device).requires_grad_(k in req)) for k, v in leaves.items()}
    out = quantile_call(mode, leaves["x"], leaves["y"], leaves["xp"], leaves["yp"])
    loss = sum((out[t] * ws[t].to(device)).sum() for t in which)
    loss.backward()
    grads = {k: (None if (v is None or v.grad is None) else v.grad.detach().cpu()) for k, v in leaves.items()}
    return [o.detach().cpu() for o in out], grads


def assert_no_tied_levels(out_cpu):
    q = out_cpu[2].reshape(-1, out_cpu[2].shape[-1])
    assert int((q[:, 1:] == q[:, :-1]).sum()) == 0, "tied merged levels on the CPU route: change the seed"


def assert_grads_close(got, want, inputs, req, label=""):
    x, y, xp, yp, _ = inputs
    for key, ref in (("x", x), ("y", y), ("xp", xp), ("yp", yp)):
        if key not in req:
            assert got[key] is None, (label, key)
            continue
        w = want[key] if want[key] is not None else torch.zeros_like(ref)
        g = got[key] if got[key] is not None else torch.zeros_like(ref)
        assert g.shape == ref.shape, (label, key, g.shape)
        g2 = g.reshape(-1, g.shape[-1]).double().numpy()
        w2 = w.reshape(-1, w.shape[-1]).double().numpy()
        assert np.isfinite(g2).all(), (label, key)
        err = np.abs(g2 - w2).max(axis=1)
        bar = RTOL * np.abs(w2).max(axis=1)
        print(f"{label} {key}: worst err / row max = {float((err / np.maximum(np.abs(w2).max(axis=1), 1e-300)).max()):.3e}")
        assert (err <= bar).all(), (label, key, float(err.max()), float(bar[np.argmax(err - bar)]))


_cpu_cache = {}


def cpu_reference(mode, shape, pos_kind, seed, which, req):
    key = (mode, shape, pos_kind, seed, which, req)
    if key not in _cpu_cache:
        inputs = make_inputs(shape, pos_kind, seed)
        for pos in inputs[2:4]:
            if pos is not None:
                srt = torch.sort(pos, -1)[0]
                assert int((srt[..., 1:] == srt[..., :-1]).sum()) == 0, "equal positions in a row: change the seed"
        out, grads = run("cpu", mode, inputs, which, req)
        assert_no_tied_levels(out)
        _cpu_cache[key] = (inputs, out, grads)
    return _cpu_cache[key]


XY = ("x", "y")
FULL = ("x", "y", "xp", "yp")

# (shape, positions, mode, upstreams, inputs that require grad, seed)
CASES = [
    ((5, 33, 33), "fixed_x", "p1", ALL, XY, 22),
    ((5, 33, 33), "rows_unsorted", "paper", ALL, FULL, 0),
    ((5, 33, 33), "shared_unsorted", "functional", ALL, FULL, 0),
    ((5, 33, 33), "rows_unsorted", "paper", ALL, ("y",), 1),
    ((3, 257, 257), "rows_sorted", "p1", ALL, FULL, 0),
    ((3, 257, 257), "shared_unsorted", "paper", (2,), FULL, 0),
    ((3, 257, 257), "rows_unsorted", "functional", (0,), FULL, 0),
    ((2, 1025, 1025), "rows_unsorted", "paper", (1,), FULL, 0),
    ((2, 1025, 1025), "fixed_x", "paper", (3,), XY, 0),
    ((2, 1025, 1025), "shared_unsorted", "functional", (4,), FULL, 1),
    ((3, 2048, 2048), "rows_unsorted", "paper", ALL, FULL, 1),
    ((3, 2048, 2048), "fixed_x", "p1", ALL, XY, 0),
    ((3, 2048, 2048), "rows_sorted", "functional", ALL, FULL, 0),
    ((4, 300, 411), "rows_unsorted", "paper", ALL, FULL, 0),
    ((4, 300, 411), "shared_unsorted", "p1", ALL, FULL, 0),
    ((4, 300, 411), "rows_sorted", "functional", ALL, FULL, 0),
    ((3, 1, 1), "rows_unsorted", "paper", ALL, FULL, 0),
    ((3, 1, 1), "shared_unsorted", "functional", ALL, FULL, 0),
    ((3, 2, 2), "rows_unsorted", "paper", ALL, FULL, 0),
    ((3, 2, 2), "fixed_x", "paper", ALL, XY, 0),
    ((2, 3, 65, 65), "rows_unsorted", "paper", ALL, FULL, 0),
    ((2, 4994, 1916), "rows_unsorted", "paper", ALL, FULL, 2),   # the per-row sort image fills the layout: the segment ends must fit in it
    ((20011, 33, 33), "rows_unsorted", "paper", ALL, FULL, 7),
]


def _case_id(c):
    shape, pos, mode, which, req, seed = c
    ups = "all" if which == ALL else "+".join(NAMES[t] for t in which)
    return f"{'x'.join(map(str, shape))}-{pos}-{mode}-{ups}-{''.join(k[-1] if k in ('x', 'y') else k for k in req)}"


# ---- host test (no GPU): header, binding table and ABI version agree on the new symbol -------------------------------------------
def test_quantiles_backward_symbol_in_header_binding_and_library():
    import sot_amd
    from sot_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    m = re.search(r"^int\s+sot_w1d_quantiles_backward\s*\(([^;]*)\)\s*;", header, flags=re.M)
    assert m, "sot_w1d_quantiles_backward is not declared in include/sot_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 13 and params[0].startswith("const sot_problem")
    assert [p.split("*")[-1].strip() for p in params[1:10]] == ["grad_uq", "grad_vq", "grad_Q", "grad_U", "grad_V", "grad_x", "grad_y",
                                                                "grad_xpos", "grad_ypos"]
    res, args = nat.EXPORTS["sot_w1d_quantiles_backward"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert args[-2] is ctypes.c_size_t and all(a is ctypes.c_void_p for a in args[1:11])
    version = int(re.search(r"#define SOT_ABI_VERSION (\d+)", header).group(1))
    assert version == nat.ABI_VERSION >= 14
    handle = ctypes.CDLL(sot_amd.build.build())
    assert hasattr(handle, "sot_w1d_quantiles_backward")
    handle.sot_abi_version.restype = ctypes.c_int
    assert handle.sot_abi_version() == version
    assert callable(nat.quantiles_backward)


def test_status_codes_on_the_host_before_anything_is_enqueued():
    """The cases the header comment names that are decided on the host (no device is touched): NULL problem / NULL inputs, bad
    shapes, rows past the gradient LDS budget."""
    from sot_amd import _native as nat
    lib = nat.load()
    fn = lib.sot_w1d_quantiles_backward
    none9 = [None] * 9
    assert fn(None, *none9, None, 0, None) == nat.SOT_ERR_NULL_POINTER
    pr = nat.SotProblem()
    pr.B, pr.n, pr.m = 4, 16, 16
    pr.x_row_stride = pr.y_row_stride = 16
    pr.p, pr.flags = 1.0, 0
    buf = (ctypes.c_float * 64)()
    out = [None] * 5 + [ctypes.addressof(buf)] + [None] * 3
    assert fn(ctypes.byref(pr), *out, None, 0, None) == nat.SOT_ERR_NULL_POINTER      # x / y / xpos / ypos NULL with B > 0
    pr.n = 0
    assert fn(ctypes.byref(pr), *out, None, 0, None) == nat.SOT_ERR_BAD_SHAPE
    pr.n, pr.x_row_stride = 16, 8
    assert fn(ctypes.byref(pr), *out, None, 0, None) == nat.SOT_ERR_BAD_SHAPE
    pr.x_row_stride = 16
    pr.B = -1
    assert fn(ctypes.byref(pr), *out, None, 0, None) == nat.SOT_ERR_BAD_SHAPE


# ---- GPU tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_gradients_match_cpu_route(case):
    from gpu_util import device, native
    native()
    shape, pos_kind, mode, which, req, seed = case
    inputs, out_cpu, want = cpu_reference(mode, shape, pos_kind, seed, which, req)
    out_gpu, got = run(device(), mode, inputs, which, req)
    lead = tuple(inputs[0].shape[:-1])
    for t, o in enumerate(out_gpu):
        assert tuple(o.shape[:-1]) == lead and o.shape == out_cpu[t].shape, (NAMES[t], o.shape)
    assert_grads_close(got, want, inputs, req, _case_id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("t", range(5), ids=NAMES)
def test_each_upstream_alone(t):
    """One output at a time feeds the loss (the other four upstream gradients are absent: NULL pointers in the C call)."""
    from gpu_util import device, native
    native()
    shape, pos_kind, mode, seed = (4, 300, 411), "rows_unsorted", "paper", 0
    inputs, _, want = cpu_reference(mode, shape, pos_kind, seed, (t,), FULL)
    _, got = run(device(), mode, inputs, (t,), FULL)
    assert_grads_close(got, want, inputs, FULL, f"only-{NAMES[t]}")


def _tie_inputs():
    """Rows with zero weights (U_i == U_{i+1}) and x == y (every U_i == V_i): every level is tied."""
    g = torch.Generator().manual_seed(11)
    B, n = 4, 7
    x = torch.rand(B, n, generator=g) + 0.05
    x[:, 2] = 0.0
    x[:, 3] = 0.0
    x[1, 0] = 0.0
    y = x.clone()
    xp = (torch.argsort(torch.rand(B, n, generator=g), -1) + 0.5 * torch.rand(B, n, generator=g)) / n   # distinct per row
    yp = xp.clone()            # the same sort order on both sides, or the CDFs of equal weights would still differ
    ws = [torch.randn(B, k, generator=g) for k in (2 * n, 2 * n, 2 * n, n, n)]
    return x, y, xp, yp, ws


@pytest.mark.gpu
def test_tied_levels_follow_the_stable_order():
    from gpu_util import device, native
    native()
    inputs = _tie_inputs()
    out_cpu, want = run("cpu", "paper", inputs, ALL, FULL)
    q = out_cpu[2]
    assert torch.equal(out_cpu[3], out_cpu[4]) and int((q[:, 1:] == q[:, :-1]).sum()) > q.shape[0] * (q.shape[1] // 2)   # it IS a tie case
    cat = torch.cat((out_cpu[3], out_cpu[4]), 1)
    assert torch.equal(torch.sort(cat, 1)[1], torch.sort(cat, dim=1, stable=True)[1]), "CPU torch.sort is not in stable order here"
    _, got = run(device(), "paper", inputs, ALL, FULL)
    assert_grads_close(got, want, inputs, FULL, "ties")


@pytest.mark.gpu
def test_zero_mass_row():
    """A row whose mass is <= 1e-7 is divided by the guard (utils.py:135-142) and gets no normalisation term: finite, equal to the CPU
    route.  The all-zero row's levels are all tied, so the rows are short enough (16 levels) for the CPU `torch.sort` to be in
    stable order, which is checked as in the tie case."""
    from gpu_util import device, native
    native()
    inputs = list(make_inputs((4, 8, 8), "rows_unsorted", 5))
    inputs[0][1] = 0.0
    inputs[1][1] = 1e-9 * torch.rand(8, generator=torch.Generator().manual_seed(1))
    inputs[0][2] = 1e-9 * torch.rand(8, generator=torch.Generator().manual_seed(2))
    inputs[1][3] = 0.0
    for mode in ("p1", "paper"):
        out_cpu, want = run("cpu", mode, inputs, ALL, FULL)
        cat = torch.cat((out_cpu[3], out_cpu[4]), 1)
        assert torch.equal(torch.sort(cat, 1)[1], torch.sort(cat, dim=1, stable=True)[1]), "CPU torch.sort is not in stable order here"
        _, got = run(device(), mode, inputs, ALL, FULL)
        for k in FULL:
            assert torch.isfinite(got[k]).all(), (mode, k)
        assert_grads_close(got, want, inputs, FULL, f"zero-mass-{mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["p1", "paper"])
def test_custom_cost_on_quantiles_equals_the_loss_gradient(mode):
    """sum_k Delta_k |uq_k - vq_k|^p reassembled in Python from the five tensors (the reference's last lines, losses.py:301-313) has
    the gradients of the module's ordinary loss call: weights and per-row positions."""
    from gpu_util import device, native
    from sot_amd.losses import Wasserstein1D
    native()
    dev = device()
    x0, y0, xp0, yp0, _ = make_inputs((6, 300, 411), "rows_unsorted", 3)
    kw = dict(p=1) if mode == "p1" else dict(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True)
    mod = Wasserstein1D(**kw).to(dev)
    rw = torch.rand(6, generator=torch.Generator().manual_seed(1)).to(dev) + 0.5     # distinct upstream gradient per row
    grads = []
    for custom in (False, True):
        x, y, xp, yp = (t.to(dev).requires_grad_(True) for t in (x0, y0, xp0, yp0))
        if custom:
            uq, vq, qs, _, _ = mod(x, y, x_pos=xp, y_pos=yp, return_quantiles=True)
            qs = torch.nn.functional.pad(qs, pad=(1, 0))
            delta = qs[..., 1:] - qs[..., :-1]
            if mod.limit_quantile_range:
                delta = torch.where(qs[..., 1:] > 1, torch.zeros_like(delta), delta)
            diff = torch.abs(uq - vq)
            rows = torch.sum(delta * (diff if mod.p == 1 else diff.pow(mod.p)), 1)
        else:
            rows = mod.row_losses(x, y, x_pos=xp, y_pos=yp)
        (rows * rw).sum().backward()
        grads.append({k: t.grad.detach().cpu() for k, t in (("x", x), ("y", y), ("xp", xp), ("yp", yp))})
    assert_grads_close(grads[1], grads[0], (x0, y0, xp0, yp0, None), FULL, f"custom-{mode}")


@pytest.mark.gpu
def test_plumbing():
    from gpu_util import device, native
    from sot_amd.losses import Wasserstein1D, wasserstein_1d, _flags
    nat = native()
    dev = device()
    x0, y0, xp0, yp0, ws = make_inputs((5, 33, 40), "rows_unsorted", 7)
    mod = Wasserstein1D(p=2, square_dist=True, dont_normalize=True).to(dev)
    flags = _flags(True, True, False, True)
    x, y, xp, yp = (t.to(dev) for t in (x0, y0, xp0, yp0))
    plain = nat.quantiles(x, y, xp, yp, 2.0, flags)

    # requires_grad of the outputs exactly when an input has it; values torch.equal to the plain native call either way
    out = mod(x, y, x_pos=xp, y_pos=yp, return_quantiles=True)
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    assert all(torch.equal(a, b) for a, b in zip(out, plain))
    for who in range(4):
        leaves = [t.clone().requires_grad_(k == who) for k, t in enumerate((x, y, xp, yp))]
        out = mod(leaves[0], leaves[1], x_pos=leaves[2], y_pos=leaves[3], return_quantiles=True)
        assert all(t.requires_grad and t.grad_fn is not None for t in out), who
        assert all(torch.equal(a.detach(), b) for a, b in zip(out, plain)), who
        with torch.no_grad():
            out = mod(leaves[0], leaves[1], x_pos=leaves[2], y_pos=leaves[3], return_quantiles=True)
        assert all(not t.requires_grad for t in out) and all(torch.equal(a, b) for a, b in zip(out, plain))
    xs, ys = x / x.sum(1, keepdim=True), y / y.sum(1, keepdim=True)
    fplain = nat.quantiles(xs, ys, xp, yp, 1.0, _flags(False, False, False, True, prenormalized=True))
    fout = wasserstein_1d(xp, yp, xs.clone().requires_grad_(True), ys, return_quantiles=True)
    assert all(t.requires_grad for t in fout) and all(torch.equal(a.detach(), b) for a, b in zip(fout, fplain))
    assert not any(t.requires_grad for t in wasserstein_1d(xp, yp, xs, ys, return_quantiles=True))

    # two identical backward calls: bit-identical gradients (no atomics, fixed summation order)
    results = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_(True) for t in (x, y, xp, yp)]
        out = mod(leaves[0], leaves[1], x_pos=leaves[2], y_pos=leaves[3], return_quantiles=True)
        sum((o * w.to(dev)).sum() for o, w in zip(out, ws)).backward()
        results.append([t.grad.clone() for t in leaves])
    assert all(torch.equal(a, b) for a, b in zip(*results))

    # an output the loss does not use, or inputs that do not ask: None in, None out (NULL pointers in the C call)
    g = [w.to(dev) for w in ws]
    only = nat.quantiles_backward(x, y, xp, yp, 2.0, flags, [None, None, g[2], None, None], (False, True, False, False))
    assert only[0] is None and only[2] is None and only[3] is None and only[1].shape == y.shape
    both = nat.quantiles_backward(x, y, xp, yp, 2.0, flags, g, (True, True, True, True))
    assert all(torch.equal(a, b) for a, b in zip(both, results[0]))


@pytest.mark.gpu
def test_c_entry_status_codes_leave_the_outputs_alone():
    """SOT_ERR_NULL_POINTER / SOT_ERR_BAD_SHAPE / SOT_ERR_UNSUPPORTED_SIZE as the header comment names them, with nothing enqueued:
    the output buffers keep their fill."""
    from gpu_util import device, native
    nat = native()
    lib = nat.load()
    dev = device()
    B, n = 3, 40
    x, y = torch.rand(B, n, device=dev), torch.rand(B, n, device=dev)
    pos = torch.rand(B, n, device=dev)
    up = torch.rand(B, 2 * n, device=dev)
    outs = [torch.full((B, n), 7.0, device=dev) for _ in range(4)]

    def call(pr, ws=None):
        return lib.sot_w1d_quantiles_backward(ctypes.byref(pr) if pr is not None else None, up.data_ptr(), up.data_ptr(), up.data_ptr(), None, None,
                                              *[o.data_ptr() for o in outs], None if ws is None else ws.data_ptr(),
                                              0 if ws is None else ws.numel(), nat.stream_ptr(dev))

    flags = nat.FLAG_REQUIRE_SORT
    good = nat.make_problem(x, y, pos, pos, 1.0, flags)
    assert call(None) == nat.SOT_ERR_NULL_POINTER
    pr = nat.make_problem(x, y, pos, pos, 1.0, flags)
    pr.x = None
    assert call(pr) == nat.SOT_ERR_NULL_POINTER
    pr = nat.make_problem(x, y, pos, pos, 1.0, flags)
    pr.m = 0
    assert call(pr) == nat.SOT_ERR_BAD_SHAPE
    pr = nat.make_problem(x, y, pos, pos, 1.0, flags)
    pr.ypos_row_stride = 0                                                     # one side shared, the other per row
    assert call(pr) == nat.SOT_ERR_BAD_SHAPE
    shared = nat.make_problem(x, y, pos[0].contiguous(), pos[1].contiguous(), 1.0, flags)
    assert call(shared) == nat.SOT_ERR_NULL_POINTER                            # shared positions that need their plan, no workspace
    big = nat.make_problem(x, y, pos, pos, 1.0, flags)
    big.n = big.m = 9000                                                       # past the gradient LDS budget: refused on the host, the
    big.x_row_stride = big.y_row_stride = big.xpos_row_stride = big.ypos_row_stride = 9000   # pointers are never followed
    assert call(big) == nat.SOT_ERR_UNSUPPORTED_SIZE
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    assert call(good) == nat.SOT_OK                                            # and the same buffers are written by a good call
    torch.cuda.synchronize()
    assert all(not bool((o == 7.0).any()) for o in outs[:2])
