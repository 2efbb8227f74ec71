"""GPU: the float64 route (include/sot_hip.h, ABI 21; csrc/sot_f64.hip; losses._f64_route_applies).

1. row losses through the C ABI against the longdouble truth of tests/f64_cases.py, every mode, shared and per-row positions, dense rows
   and rows with gaps that start on 8-byte boundaries only, a zero-mass row among the rest;
2. a workgroup's second and later rows: every row of a batch of more than twice the grid's capacity equals, bit for bit, the same row
   evaluated in a batch of one -- forward and backward;
3. the size limits: 4097 + 4097 forward, the first unsupported size, and the module's route beyond it;
4. gradients from Wasserstein1D and wasserstein_1d against torch autograd of the torch-op composition on the CPU, with the same composition
   on the GPU (the route such tensors took before) as the yardstick; torch.autograd.gradcheck;
5. module behaviour: dims, hinge, 3-D inputs, require_sort, no_grad, no warning, replay from a captured graph;
6. the memory contract inside guard bands (tests/guarded.py), refusals, the empty batch.

BOUNDS.  Row losses: e_hip <= 4 E_ref |truth_row| + 4 * 2^-52 |truth_row|, E_ref = the worst relative error, in the same batch, of the package's
CPU float64 route against the truth (the factor 4: what tests/test_eval_metrics_gpu.py grants a restated chain; the second term: the last
rounding).  Gradients: |g_hip - g_cpu| <= 4 max|g_gpu_composition - g_cpu| + (n + m) 2^-52 max|g_row| (the second term: the rounding bound of a
suffix sum of n + m terms).  The cutoff modes run on the recipe rows of tests/f64_cases.py, the others on generic random rows.
"""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import f64_cases as fc
import guarded as gd
from gpu_util import device, native

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 2.0 ** -52
RS, PRE = 8, 16
SOT_OK, SOT_ERR_BAD_SHAPE, SOT_ERR_UNSUPPORTED_SIZE, SOT_ERR_NULL_POINTER, SOT_ERR_INVALID_P = 0, -2, -3, -4, -1
MODE_IDS = [m[0] for m in fc.MODES]


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def stream(nat):
    return nat.stream_ptr(device())


def dev_t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device())


def same_bits(got, want):
    return torch.equal(got.contiguous().view(torch.int64), want.contiguous().view(torch.int64))


def _cpu_rows(x, y, xpos, ypos, mode):
    """the package's CPU float64 route (the torch-op composition) on numpy inputs -> numpy [B]"""
    from sot_amd import _torch_path as tp
    t = torch.tensor
    return tp.module_forward(t(x), t(y), t(xpos), t(ypos), require_sort=False, hinge_on=False, rows_only=True, **fc.mode_kwargs(mode)).numpy()


def _forward(nat, x, y, xp, yp, mode, prenorm=False):
    """sot_w1d_forward_f64 on device tensors (any row stride); the row losses inside guard bands"""
    B = x.shape[0]
    rows, g = gd.guarded((B,), F64, device(), name="row losses")
    pr = nat.make_problem_f64(x, y, xp, yp, mode[1], fc.mode_flags(mode) | (PRE if prenorm else 0))
    rc = nat.load().sot_w1d_forward_f64(ctypes.byref(pr), gd.ptr(rows, g), None, 0, stream(nat))
    assert rc == SOT_OK, rc
    torch.cuda.synchronize()
    g.assert_untouched()
    g.assert_fully_written()
    return rows.clone()


def _check_rows(tag, got, truth, cpu):
    """the bound of the module docstring, per row; prints e_hip and E_ref"""
    truth_abs = np.abs(truth).astype(np.float64)
    nz = truth_abs > 0
    e_ref = float(np.max(np.abs(cpu[nz] - truth[nz]) / np.abs(truth[nz]))) if nz.any() else 0.0
    err = np.abs(got.astype(fc.LD) - truth).astype(np.float64)
    e_hip = float(np.max(err[nz] / truth_abs[nz])) if nz.any() else 0.0
    print(f"{tag}: e_hip {e_hip:.3g}  E_ref {e_ref:.3g}")
    bound = 4.0 * e_ref * truth_abs + 4.0 * EPS * truth_abs
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), f"{tag}: row {worst}: error {err[worst]:.3g} > bound {bound[worst]:.3g} (e_hip {e_hip:.3g}, E_ref {e_ref:.3g})"


# ---- 1. row losses through the C ABI against the truth -------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (257, 257), (300, 300), (1025, 1025), (300, 411), (1, 700)]
LAYOUTS = ("shared-dense", "shared-gaps8", "rowpos-dense", "rowpos-gaps8")
B1 = 12


def _laid_out(a, gaps, pad):
    """a [B, n] numpy array on the device: dense, or rows `pad` elements apart from each other's end with the first one 8 bytes past a
    256-byte boundary -- an odd stride puts every second row on an 8-byte boundary only"""
    if not gaps:
        return dev_t(a)
    view, _ = gd.guarded(a.shape, F64, device(), row_stride=a.shape[1] + pad, offset_bytes=8, fill="poison", name="rows with gaps")
    view.copy_(dev_t(a))
    return view


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,m", SHAPES, ids=[f"{n}x{m}" for n, m in SHAPES])
def test_row_losses_against_the_truth(n, m, layout):
    nat = native()
    rowpos, gaps = layout.startswith("rowpos"), layout.endswith("gaps8")
    rng = np.random.default_rng(1000 + 7 * n + m)
    if rowpos:
        xpos, ypos = fc.sorted_positions(rng, (B1, n)), fc.sorted_positions(rng, (B1, m))
        xp, yp = _laid_out(xpos, gaps, 1), _laid_out(ypos, gaps, 3)
    else:
        xpos, ypos = (fc.grid(n), fc.grid(m)) if n == m else (fc.sorted_positions(rng, (n,)), fc.sorted_positions(rng, (m,)))
        xp, yp = dev_t(xpos), dev_t(ypos)
    for k, mode in enumerate(fc.MODES):
        x, y = fc.rows_for(mode, B1, n, m, seed=50 * n + m + k)
        x[1], y[1] = 0.0, 0.0                                   # a zero-mass row among the rest (the mass guard)
        truth = fc.eval_rows(x, y, xpos, ypos, mode)
        cpu = _cpu_rows(x, y, np.broadcast_to(xpos, (B1, n)).copy(), np.broadcast_to(ypos, (B1, m)).copy(), mode)
        got = _forward(nat, _laid_out(x, gaps, 3), _laid_out(y, gaps, 5), xp, yp, mode).cpu().numpy()
        assert got[1] == 0.0
        _check_rows(f"{n}x{m} {layout} {mode[0]}", got, truth, cpu)


def test_prenormalized_weights_are_used_as_given():
    """SOT_FLAG_PRENORMALIZED (the functional wasserstein_1d): no normalisation, SQUARE and DONT_NORMALIZE ignored"""
    nat = native()
    n, m = 300, 411
    rng = np.random.default_rng(9)
    xpos, ypos = fc.sorted_positions(rng, (n,)), fc.sorted_positions(rng, (m,))
    from sot_amd import _torch_path as tp
    for mode in (("pre_p1", 1.0, True, True, False), ("pre_cut_p2", 2.0, False, False, True)):
        if mode[4]:      # under the cutoff: the recipe rows (x / sum x is exact and its CDF ends at 1.0; y carries 1.2 ... 1.5 times the mass)
            x, y = fc.cutoff_rows(B1, n, m, False, seed=77)
            a, b = x / x.sum(1, keepdims=True), y / x.sum(1, keepdims=True)
        else:
            x, y = fc.plain_rows(B1, n, m, seed=77)
            a, b = x / x.sum(1, keepdims=True), y / y.sum(1, keepdims=True)
        truth = fc.eval_rows(a, b, xpos, ypos, mode, prenormalized=True)
        t = torch.tensor
        cpu = tp.transport_rows(t(xpos).expand(B1, n), t(ypos).expand(B1, m), t(a), t(b), p=mode[1], require_sort=False,
                                limit_quantile_range=mode[4]).numpy()
        got = _forward(nat, dev_t(a), dev_t(b), dev_t(xpos), dev_t(ypos), mode, prenorm=True).cpu().numpy()
        _check_rows(mode[0], got, truth, cpu)


# ---- 2. a workgroup's second and later rows -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [fc.MODES[0], fc.MODES[6], fc.MODES[3]], ids=lambda m: m[0])
def test_second_and_later_rows_of_a_workgroup_equal_a_batch_of_one(mode):
    nat = native()
    n = 64
    B = 2 * 8 * cus() + 5          # a CU holds at most 8 workgroups of 256 threads: more than twice any grid the launch can pick
    x, y = fc.rows_for(mode, B, n, n, seed=31)
    scale = np.random.default_rng(5).uniform(0.01, 50.0, size=(B, 1))
    if not mode[4]:
        x, y = x * scale, y * scale**0.5                       # heterogeneous rows
    x[7], y[7] = 0.0, 0.0
    x, y, pos = dev_t(x), dev_t(y), dev_t(fc.grid(n))
    flags = fc.mode_flags(mode)
    rows = nat.forward_rows_f64(x, y, pos, pos, mode[1], flags)
    w = dev_t(np.random.default_rng(6).uniform(0.5, 2.0, size=B))
    gx, gy = nat.backward_rows_f64(x, y, pos, pos, mode[1], flags, w)
    one_rows = torch.empty_like(rows)
    one_gx, one_gy = torch.empty_like(gx), torch.empty_like(gy)
    for r in range(B):
        one_rows[r:r + 1] = nat.forward_rows_f64(x[r:r + 1], y[r:r + 1], pos, pos, mode[1], flags)
        a, b = nat.backward_rows_f64(x[r:r + 1], y[r:r + 1], pos, pos, mode[1], flags, w[r:r + 1])
        one_gx[r:r + 1], one_gy[r:r + 1] = a, b
    torch.cuda.synchronize()
    assert torch.isfinite(rows).all() and float(rows.max()) > 0
    assert same_bits(rows, one_rows)
    assert same_bits(gx, one_gx) and same_bits(gy, one_gy)


# ---- 3. size limits -------------------------------------------------------------------------------------------------------------------

def test_forward_at_4097_bins_a_side_against_the_truth():
    nat = native()
    n, B = 4097, 3
    for mode in (fc.MODES[0], fc.MODES[6]):
        x, y = fc.rows_for(mode, B, n, n, seed=12)
        pos = fc.grid(n)
        truth = fc.eval_rows(x, y, pos, pos, mode)
        cpu = _cpu_rows(x, y, np.broadcast_to(pos, (B, n)).copy(), np.broadcast_to(pos, (B, n)).copy(), mode)
        got = _forward(nat, dev_t(x), dev_t(y), dev_t(pos), dev_t(pos), mode).cpu().numpy()
        _check_rows(f"4097x4097 {mode[0]}", got, truth, cpu)


def test_first_unsupported_size_is_refused_and_the_module_runs_the_composition(monkeypatch):
    from sot_amd import losses
    nat = native()
    for backward in (False, True):
        k = next(k for k in range(2, 40000) if not nat.f64_supported(k, k, backward=backward))
        assert nat.f64_supported(k - 1, k - 1, backward=backward) and k > (2049 if backward else 4097)
        x, y = dev_t(np.ones((2, k))), dev_t(np.ones((2, k)))
        pos = dev_t(fc.grid(k))
        pr = nat.make_problem_f64(x, y, pos, pos, 2.0, 0)
        out, g = gd.guarded((2, k), F64, device(), name="untouched output")
        if backward:
            rc = nat.load().sot_w1d_backward_f64(ctypes.byref(pr), None, 0, 1.0, gd.ptr(out, g), None, None, 0, stream(nat))
        else:
            rc = nat.load().sot_w1d_forward_f64(ctypes.byref(pr), gd.ptr(out, g), None, 0, stream(nat))
        assert rc == SOT_ERR_UNSUPPORTED_SIZE
        torch.cuda.synchronize()
        g.assert_untouched()
        assert not bool((out.view(torch.int32) != gd.POISON).any())
        if backward:
            continue
        # the module beyond the limit: the composition, with its warning, in float64
        monkeypatch.setattr(losses, "_warned", set())
        mod = losses.Wasserstein1D(p=2, square_dist=True).to(device())
        xs, ys = fc.plain_rows(2, k, k, seed=3)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            val = mod(dev_t(xs), dev_t(ys), x_pos=pos, y_pos=pos.clone())
        assert any("torch-op" in str(w.message) for w in seen)
        assert val.dtype == F64 and val.is_cuda
        want = _cpu_rows(xs, ys, np.broadcast_to(fc.grid(k), (2, k)).copy(), np.broadcast_to(fc.grid(k), (2, k)).copy(), fc.MODES[1]).mean()
        assert abs(float(val) - want) <= 1e-10 * abs(want)


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(9, 300), (5, 1025)]


@functools.lru_cache(maxsize=None)
def _grad_case(mode_idx, B, n):
    """inputs, the CPU autograd gradients of the composition and the GPU composition's (the yardstick): computed once per (mode, shape)"""
    from sot_amd import _torch_path as tp
    mode = fc.MODES[mode_idx]
    x, y = fc.rows_for(mode, B, n, n, seed=200 + mode_idx + n)
    pos = fc.grid(n)
    out = {}
    for where in ("cpu", "gpu"):
        t = (lambda a: torch.tensor(a)) if where == "cpu" else dev_t
        tx, ty = t(x).requires_grad_(True), t(y).requires_grad_(True)
        val = tp.module_forward(tx, ty, t(pos), t(pos), require_sort=True, hinge_on=False, **fc.mode_kwargs(mode))
        val.backward()
        out[where] = (tx.grad.cpu(), ty.grad.cpu(), float(val.detach()))
    return x, y, pos, out


def _check_grad(tag, got, cpu, yard, n, m):
    yardstick = float((yard - cpu).abs().max())
    err = (got.cpu() - cpu).abs()
    bound = 4.0 * yardstick + (n + m) * EPS * cpu.abs().amax(dim=1, keepdim=True)
    print(f"{tag}: max|g_hip - g_cpu| {float(err.max()):.3g}  max|g_gpu_composition - g_cpu| {yardstick:.3g}  max|g| {float(cpu.abs().max()):.3g}")
    assert bool((err <= bound).all()), f"{tag}: {float((err - bound).max()):.3g} over the bound"


@pytest.mark.parametrize("B,n", GRAD_SHAPES, ids=[f"{b}x{n}" for b, n in GRAD_SHAPES])
@pytest.mark.parametrize("mode_idx", range(len(fc.MODES)), ids=MODE_IDS)
def test_module_gradients_against_cpu_autograd(mode_idx, B, n):
    from sot_amd.losses import Wasserstein1D
    native()
    mode = fc.MODES[mode_idx]
    x, y, pos, ref = _grad_case(mode_idx, B, n)
    mod = Wasserstein1D(require_sort=True, **fc.mode_kwargs(mode)).to(device())
    p = dev_t(pos)
    for wrt in ("x", "y", "xy"):
        tx, ty = dev_t(x).requires_grad_("x" in wrt), dev_t(y).requires_grad_("y" in wrt)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            val = mod(tx, ty, x_pos=p, y_pos=p)
            val.backward()
        assert val.dtype == F64 and abs(float(val.detach()) - ref["cpu"][2]) <= 1e-12 * abs(ref["cpu"][2])
        assert (tx.grad is not None) == ("x" in wrt) and (ty.grad is not None) == ("y" in wrt)
        if "x" in wrt:
            assert tx.grad.dtype == F64
            _check_grad(f"{mode[0]} {B}x{n} d/dx ({wrt})", tx.grad, ref["cpu"][0], ref["gpu"][0], n, n)
        if "y" in wrt:
            _check_grad(f"{mode[0]} {B}x{n} d/dy ({wrt})", ty.grad, ref["cpu"][1], ref["gpu"][1], n, n)


@pytest.mark.parametrize("name,p,lim", [("p1", 1, False), ("p3", 3, False), ("cut_p2", 2, True)])
def test_functional_gradients_against_cpu_autograd(name, p, lim):
    """wasserstein_1d: weights used as given (normalised outside, by torch ops on the leaves), per-row sorted positions"""
    from sot_amd import _torch_path as tp
    from sot_amd.losses import wasserstein_1d
    native()
    B, n, m = 9, 300, 411
    rng = np.random.default_rng(17)
    # under the cutoff: the recipe rows (x / sum x is exact, U ends at 1.0; y carries 1.2 ... 1.5 times the mass of x and is divided by it)
    x, y = fc.cutoff_rows(B, n, m, False, seed=23) if lim else fc.plain_rows(B, n, m, seed=23)
    xpos, ypos = fc.sorted_positions(rng, (B, n)), fc.sorted_positions(rng, (B, m))
    w = rng.uniform(0.5, 2.0, size=B)
    grads = {}
    for where in ("cpu", "gpu", "hip"):
        t = (lambda a: torch.tensor(a)) if where == "cpu" else dev_t
        tx, ty = t(x).requires_grad_(True), t(y).requires_grad_(True)
        a = tx / tx.sum(1, keepdim=True)
        b = ty / (tx.sum(1, keepdim=True) if lim else ty.sum(1, keepdim=True))
        if where == "hip":
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                rows = wasserstein_1d(t(xpos), t(ypos), a, b, p=p, require_sort=True, limit_quantile_range=lim)
        else:
            rows = tp.transport_rows(t(xpos), t(ypos), a, b, p=p, require_sort=True, limit_quantile_range=lim)
        assert rows.dtype == F64 and rows.shape == (B,)
        (rows * t(w)).sum().backward()
        grads[where] = (tx.grad.cpu(), ty.grad.cpu(), rows.detach().cpu())
    assert float((grads["hip"][2] - grads["cpu"][2]).abs().max()) <= 1e-12 * float(grads["cpu"][2].abs().max())
    _check_grad(f"functional {name} d/dx", grads["hip"][0], grads["cpu"][0], grads["gpu"][0], n, m)
    _check_grad(f"functional {name} d/dy", grads["hip"][1], grads["cpu"][1], grads["gpu"][1], n, m)


def test_gradcheck_on_small_rows_without_cutoff():
    from sot_amd.losses import Wasserstein1D
    native()
    x, y = fc.plain_rows(2, 17, 17, seed=41)
    pos = dev_t(fc.grid(17))
    for kw in (dict(p=1), dict(p=2, square_dist=True), dict(p=3, dont_normalize=True)):
        mod = Wasserstein1D(**kw).to(device())
        tx, ty = dev_t(x + 0.1).requires_grad_(True), dev_t(y + 0.1).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda a, b: mod.row_losses(a, b, x_pos=pos, y_pos=pos), (tx, ty), eps=1e-6, atol=1e-7, rtol=1e-5)
        assert torch.autograd.gradcheck(lambda a, b: mod(a, b, x_pos=pos, y_pos=pos), (tx, ty), eps=1e-6, atol=1e-7, rtol=1e-5)


# ---- 5. module behaviour --------------------------------------------------------------------------------------------------------------

def _composition(mod_kwargs, x, y, xpos, ypos, **call):
    """the torch-op composition on the CPU (what the module computes for CPU tensors)"""
    from sot_amd.losses import Wasserstein1D
    t = torch.tensor
    return Wasserstein1D(**mod_kwargs)(t(x), t(y), x_pos=t(xpos), y_pos=t(ypos), **call)


def _close(got, want, tol=1e-12):
    got, want = got.detach().cpu(), want.detach()
    assert got.dtype == F64 and got.shape == want.shape
    assert float((got - want).abs().max()) <= tol * max(float(want.abs().max()), 1e-300), float((got - want).abs().max())


def test_module_dims_hinge_3d_inputs_sorting_and_no_grad():
    from sot_amd.losses import Wasserstein1D
    native()
    rng = np.random.default_rng(3)
    n, m = 65, 90
    x, y = rng.random((4, 5, n)), rng.random((4, 5, m))
    xpos, ypos = rng.random(n), rng.random(m)                     # an UNSORTED shared grid
    xrow, yrow = rng.random((4, 5, n)), rng.random((4, 5, m))     # unsorted per-row positions
    sq_dn = dict(p=2, square_dist=True, dont_normalize=True)     # (generic rows: no cutoff, see tests/f64_cases.py)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                            # no warning on the new route
        for kw in (dict(p=1), dict(p=2, square_dist=True), dict(p=1.5, dont_normalize=True), dict(p=3)):
            mod = Wasserstein1D(**kw).to(device())
            for call in (dict(), dict(dims=[0]), dict(dims=[1]), dict(dims=[0, 1])):
                _close(mod(dev_t(x), dev_t(y), x_pos=dev_t(xpos), y_pos=dev_t(ypos), **call), _composition(kw, x, y, xpos, ypos, **call))
                _close(mod(dev_t(x), dev_t(y), x_pos=dev_t(xrow), y_pos=dev_t(yrow), **call), _composition(kw, x, y, xrow, yrow, **call))
            _close(mod.row_losses(dev_t(x), dev_t(y), x_pos=dev_t(xpos), y_pos=dev_t(ypos)),
                   Wasserstein1D(**kw).row_losses(torch.tensor(x), torch.tensor(y), x_pos=torch.tensor(xpos), y_pos=torch.tensor(ypos)))
            # 2-D inputs, the same grid tensor again (served from the sorted-grid cache), and the call keywords of the cutoff
            _close(mod(dev_t(x[0]), dev_t(y[0]), x_pos=dev_t(xpos), y_pos=dev_t(ypos), dont_normalize=True),
                   _composition(kw, x[0], y[0], xpos, ypos, dont_normalize=True))
        # hinge: relu(rows - threshold), threshold from the call
        hk = dict(p=1, hinge=True)
        mod = Wasserstein1D(**hk).to(device())
        thr = float(Wasserstein1D(p=1).row_losses(torch.tensor(x), torch.tensor(y), x_pos=torch.tensor(xpos), y_pos=torch.tensor(ypos)).median())
        got = mod(dev_t(x), dev_t(y), x_pos=dev_t(xpos), y_pos=dev_t(ypos), hinge=thr, dims=[1])
        want = _composition(hk, x, y, xpos, ypos, hinge=thr, dims=[1])
        assert float((got.cpu() - want).abs().max()) <= 1e-12 and float(want.max()) > 0
        # gradients through the sorting gathers: an unsorted shared grid and unsorted per-row positions
        for xp_, yp_ in ((xpos, ypos), (xrow, yrow)):
            ty = dev_t(y).requires_grad_(True)
            Wasserstein1D(**sq_dn).to(device())(dev_t(x), ty, x_pos=dev_t(xp_), y_pos=dev_t(yp_)).backward()
            tc = torch.tensor(y).requires_grad_(True)
            Wasserstein1D(**sq_dn)(torch.tensor(x), tc, x_pos=torch.tensor(xp_), y_pos=torch.tensor(yp_)).backward()
            assert ty.grad.dtype == F64 and float((ty.grad.cpu() - tc.grad).abs().max()) <= 1e-10 * float(tc.grad.abs().max())
        # torch.no_grad: tensors that require a gradient take the plain forward
        ty = dev_t(y).requires_grad_(True)
        with torch.no_grad():
            out = Wasserstein1D(p=2).to(device())(dev_t(x), ty, x_pos=dev_t(xpos), y_pos=dev_t(ypos))
        assert out.dtype == F64 and not out.requires_grad
        _close(out, _composition(dict(p=2), x, y, xpos, ypos))


def test_calls_outside_the_gate_keep_the_composition_and_its_warning(monkeypatch):
    from sot_amd import losses
    native()
    x, y = fc.plain_rows(4, 33, 33, seed=8)
    pos = fc.grid(33)
    mod = losses.Wasserstein1D(p=2).to(device())
    calls = []

    def ran(*args, **kwargs):
        calls.append(args)
        raise AssertionError("the float64 route ran")
    monkeypatch.setattr(losses.nat, "forward_rows_f64", ran)
    for xp in (dev_t(pos).float(), dev_t(pos).requires_grad_(True)):       # float32 positions; a position gradient
        monkeypatch.setattr(losses, "_warned", set())
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = mod(dev_t(x), dev_t(y), x_pos=xp, y_pos=xp)
        assert out.dtype == F64 and any("torch-op" in str(w.message) for w in seen) and not calls
    monkeypatch.setattr(losses, "_warned", set())
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        q = mod(dev_t(x), dev_t(y), x_pos=dev_t(pos), y_pos=dev_t(pos), return_quantiles=True)
    assert len(q) == 5 and all(t.dtype == F64 for t in q) and any("torch-op" in str(w.message) for w in seen) and not calls


def test_replay_from_a_captured_graph_equals_eager():
    """Forward + backward captured into a graph and replayed on two input sets: the eager bits.  As in the other graph tests of the suite,
    every call before the capture runs on a side stream and leaves no autograd graph alive: a leaf's gradient accumulator keeps the stream
    it was created on for as long as a graph holds it, and a captured backward must not hop to the default stream."""
    from sot_amd.losses import Wasserstein1D
    native()
    mode = fc.MODES[6]
    mod = Wasserstein1D(require_sort=True, **fc.mode_kwargs(mode)).to(device())
    pos = dev_t(fc.grid(300))
    x, y = fc.rows_for(mode, 33, 300, 300, seed=19)
    sx, sy = dev_t(x), dev_t(y).requires_grad_(True)

    def step():
        out = mod(sx, sy, x_pos=pos, y_pos=pos)
        out.backward()
        return out.detach()

    side = torch.cuda.Stream(device=device())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                              # (the first call also puts the grid into the sorted-grid cache: one synchronisation)
            sy.grad = None
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    sy.grad = None
    with torch.cuda.graph(graph):
        val = step()
    for seed in (19, 20):
        xa, ya = fc.rows_for(mode, 33, 300, 300, seed=seed)
        with torch.no_grad():
            sx.copy_(dev_t(xa))
            sy.copy_(dev_t(ya))
        graph.replay()
        torch.cuda.synchronize()
        yc = dev_t(ya).requires_grad_(True)
        want = mod(dev_t(xa), yc, x_pos=pos, y_pos=pos)
        want.backward()
        torch.cuda.synchronize()
        assert float(want.detach()) > 0 and same_bits(val, want.detach()) and same_bits(sy.grad, yc.grad)


# ---- 6. memory contract ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowpos", [False, True], ids=["shared", "rowpos"])
def test_memory_contract_inside_guard_bands(rowpos):
    nat = native()
    lib = nat.load()
    B, n, m = 2 * 8 * cus() + 3, 65, 91
    mode = fc.MODES[6]
    flags = fc.mode_flags(mode)
    x, y = fc.cutoff_rows(B, n, m, True, seed=2)
    rng = np.random.default_rng(4)
    xs = dev_t(fc.sorted_positions(rng, (B, n) if rowpos else (n,)))
    ys = dev_t(fc.sorted_positions(rng, (B, m) if rowpos else (m,)))
    w = dev_t(rng.uniform(0.5, 2.0, size=B))
    results = []
    for (xv, gxin), (yv, gyin) in zip(gd.poisoned_pair(dev_t(x), row_stride=n + 3, offset_bytes=8, name="x"),
                                      gd.poisoned_pair(dev_t(y), row_stride=m + 2, offset_bytes=0, name="y")):
        pr = nat.make_problem_f64(xv, yv, xs, ys, mode[1], flags)
        need = lib.sot_w1d_f64_workspace_bytes(ctypes.byref(pr))
        assert need == 0                                          # exact workspace size: the calls use none ...
        ws, gws = gd.workspace(need, 8, device())                 # ... so the guard bands start at the pointer they are handed
        rows, grows = gd.guarded((B,), F64, device(), name="row losses")
        gxo, ggx = gd.guarded((B, n), F64, device(), offset_bytes=8, name="grad x")
        gyo, ggy = gd.guarded((B, m), F64, device(), name="grad y")
        assert lib.sot_w1d_forward_f64(ctypes.byref(pr), gd.ptr(rows, grows), gd.ptr(ws, gws), need, stream(nat)) == SOT_OK
        assert lib.sot_w1d_backward_f64(ctypes.byref(pr), w.data_ptr(), 1, 0.5, gd.ptr(gxo, ggx), gd.ptr(gyo, ggy), gd.ptr(ws, gws), need,
                                        stream(nat)) == SOT_OK
        torch.cuda.synchronize()
        for g in (grows, ggx, ggy, gws):
            g.assert_untouched()
        for g in (grows, ggx, ggy):
            g.assert_fully_written()
        gxin.assert_unchanged()
        gyin.assert_unchanged()
        # a larger workspace than asked for is left alone too; one gradient only: the other buffer is not written
        big, gbig = gd.workspace(4096, 16, device(), name="spare workspace")
        gbig.snapshot()
        only, gonly = gd.guarded((B, m), F64, device(), name="grad y alone")
        assert lib.sot_w1d_backward_f64(ctypes.byref(pr), None, 0, 0.5, None, gd.ptr(only, gonly), gd.ptr(big, gbig), 4096, stream(nat)) == SOT_OK
        torch.cuda.synchronize()
        gbig.assert_unchanged()
        gonly.assert_untouched()
        gonly.assert_fully_written()
        results.append((rows.clone(), gxo.clone(), gyo.clone()))
    for a, b in zip(*results):                                    # nothing outside the rows is read: zeros or NaNs in the gaps, the same bits
        assert same_bits(a, b)
    assert torch.isfinite(results[0][0]).all() and torch.isfinite(results[0][1]).all() and torch.isfinite(results[0][2]).all()


def test_refusals_and_the_empty_batch():
    nat = native()
    lib = nat.load()
    n, m = 40, 50
    x, y = dev_t(np.ones((4, n))), dev_t(np.ones((4, m)))
    xs, ys = dev_t(fc.grid(n)), dev_t(fc.grid(m))
    out, g = gd.guarded((4, m), F64, device(), name="untouched output")
    s = stream(nat)

    def fwd(pr, out_ptr=gd.ptr(out, g), ws=None, nbytes=0):
        return lib.sot_w1d_forward_f64(ctypes.byref(pr) if pr is not None else None, out_ptr, ws, nbytes, s)

    def bwd(pr, gx=None, gy=gd.ptr(out, g), ws=None, nbytes=0, stride=0):
        return lib.sot_w1d_backward_f64(ctypes.byref(pr) if pr is not None else None, None, stride, 1.0, gx, gy, ws, nbytes, s)

    good = lambda **kw: nat.make_problem_f64(x, y, xs, ys, kw.get("p", 2.0), kw.get("flags", 0))   # noqa: E731
    assert fwd(None) == SOT_ERR_NULL_POINTER and bwd(None) == SOT_ERR_NULL_POINTER
    for call in (fwd, bwd):
        assert call(good(p=0.5)) == SOT_ERR_INVALID_P
        assert call(good(flags=RS)) == SOT_ERR_BAD_SHAPE                     # supports arrive sorted
        assert call(good(), ws=None, nbytes=64) == SOT_ERR_NULL_POINTER      # a workspace size without a workspace
        for field in ("x", "y", "xpos", "ypos"):
            pr = good()
            setattr(pr, field, None)
            assert call(pr) == SOT_ERR_NULL_POINTER, field
        for field, value in (("n", 0), ("m", -1), ("B", -1), ("x_row_stride", n - 1), ("y_row_stride", 1), ("xpos_row_stride", n)):
            pr = good()
            setattr(pr, field, value)
            assert call(pr) == SOT_ERR_BAD_SHAPE, field
    assert fwd(good(), out_ptr=None) == SOT_ERR_NULL_POINTER
    assert bwd(good(), stride=2) == SOT_ERR_BAD_SHAPE
    empty = good()
    empty.B = 0
    empty.x = empty.y = None
    assert fwd(empty) == SOT_OK and bwd(empty) == SOT_OK and fwd(empty, out_ptr=None) == SOT_OK
    assert bwd(good(), gx=None, gy=None) == SOT_OK                            # no gradient asked for: nothing to do
    torch.cuda.synchronize()
    g.assert_untouched()
    assert not bool((out.view(torch.int32) != gd.POISON).any())               # no refusal and no empty batch wrote anything
    with pytest.raises(AssertionError):
        nat.forward_rows_f64(x, y, xs, ys, 0.5, 0)
    with pytest.raises(TypeError):
        nat.forward_rows_f64(x.float(), y.float(), xs, ys, 2.0, 0)
    assert nat.forward_rows_f64(x[:0], y[:0], xs, ys, 2.0, 0).shape == (0,)
