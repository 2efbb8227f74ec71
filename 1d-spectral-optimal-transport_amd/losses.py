"""Host-side mirror of the reference's loss interface for the SOT hot path.

Same names, argument meaning and error behaviour as the reference's ``losses`` module
(/root/reference/losses.py): ``Wasserstein1D`` (:89-211), ``quantile_function`` (:214-220),
``wasserstein_1d`` (:223-313), ``Wasserstein1DWithTransform`` (:316-343), ``MixOfLosses`` (:346-362), ``MSSLoss``
(:365-425) and ``utils.safe_divide``
(utils.py:135-142), so ``trainer.py:220/228``, ``metrics.py:148`` and the YAML
``class_path: losses.Wasserstein1D`` keep working unchanged.

All arithmetic on HIP-device tensors runs in the hand-written HIP library (csrc/, C ABI in include/sot_hip.h); this file only reshapes,
marshals pointers and wires autograd.  Which kernels a call reaches is decided once per call by _route(); the table "condition -> route
-> native calls" is DESIGN.md section 1.1.  Tensors outside the library's domain take the reference's own route, torch ops
(_torch_path.py), because the reference is device- and dtype-agnostic (losses.py:129-211) and `accelerator: cpu` has to keep working.
"""
from __future__ import annotations

import typing
import warnings

import torch

from . import _native as nat
from . import _torch_path as tp
from . import ops as _ops_module  # noqa: F401 -- registers the sot_amd:: custom ops

_o = torch.ops.sot_amd                      # the route of a call that torch.compile / torch.export is tracing (ops.py); eager never takes it
_compiling = torch.compiler.is_compiling

# (wasserstein_1d_csr -- ragged supports in CSR form -- is retired from the public surface since round 4: zero-masked dense rows are
#  config 4; the function itself stays for its tests and the C entry point)
__all__ = ["Wasserstein1D", "Wasserstein1DWithTransform", "wasserstein_1d", "quantile_function", "MixOfLosses", "MSSLoss", "safe_divide"]

FLAG_PRENORMALIZED = nat.FLAG_PRENORMALIZED


def safe_divide(numerator, denominator, eps=1e-7):
    """utils.py:135-142 -- kept for API compatibility (the fused kernel applies the same guard)."""
    safe_denominator = torch.where(denominator <= eps,
                                   torch.tensor(eps, dtype=torch.float32, device=denominator.device), denominator)
    return numerator / safe_denominator


_warned = set()


def warn_once(key, message):
    """One warning per distinct situation (e.g. per unsupported transform size), not one per call."""
    if key not in _warned:
        _warned.add(key)
        warnings.warn(message, stacklevel=3)


def _is_hip_tensor(t) -> bool:
    """The one device test of the route decision (tests patch it to run the decision on meta stand-ins)."""
    return t.is_cuda


def _hip_domain(x, y, *positions) -> bool:
    """True when the HIP library takes these tensors (the two weight tensors first, then the positions): all of them on a HIP device, the
    positions float32 and the weights either both float32 or both bfloat16 -- what a model under torch.autocast(dtype=torch.bfloat16)
    hands over; widening a bfloat16 is exact, so such a call is DEFINED as the float32 call on x.float(), y.float() and returns its bits
    (the loss in float32, the gradient of a bfloat16 operand in bfloat16, rounded to nearest even).  CPU tensors (any floating dtype) and
    float64 tensors (any device) go to the torch-op composition instead -- float64 is then float64 arithmetic, as in the reference; a
    float64 GPU tensor says so once.  half GPU tensors (another exponent range), a float32 / bfloat16 mix and bfloat16 positions are
    refused (TypeError), not upcast."""
    ts = [t for t in (x, y) + positions if t is not None]
    on_hip = [_is_hip_tensor(t) for t in ts]
    if all(on_hip) and all(t.dtype == torch.float32 for t in positions if t is not None):
        if x.dtype == y.dtype and x.dtype in (torch.float32, torch.bfloat16):
            return True
    for t, hip in zip(ts, on_hip):
        if hip and t.dtype in (torch.float16, torch.bfloat16):
            raise TypeError(f"sot_amd computes in float32; got {t.dtype} (convert with .float())")
    if any(on_hip):
        warn_once("not-hip-f32", "sot_amd: tensors that are not all float32 on the GPU (float64, or CPU and GPU mixed) run the torch-op "
                                 "composition in their own dtype, like the reference; the HIP kernels take float32 GPU tensors")
    return False


class _RowsToF32(torch.autograd.Function):
    """[rows, n] bfloat16 -> float32 (sot_rows_bf16_to_f32); the gradient comes back narrowed to bfloat16 (sot_rows_f32_to_bf16)."""

    @staticmethod
    def forward(ctx, rows):
        return nat.rows_to_f32(rows)

    @staticmethod
    def backward(ctx, g):
        return nat.rows_to_bf16(g.float())


def _widen(t):
    """A bfloat16 weight tensor of any leading shape as float32, attached to autograd through the narrowing kernel."""
    rows = t.reshape(-1, t.shape[-1])
    out = _o.rows_to_f32(rows) if _compiling() else _RowsToF32.apply(rows)
    return out.reshape(t.shape)


def _typed_forward_applies(x, y, xpos, ypos, return_quantiles=False, mixed=None) -> bool:
    """bfloat16 weights: does the call take the typed forward (sot_w1d_forward_bf16 / sot_w1d_loss_bf16 -- 16-bit row loads in the kernel on
    the headline and paper shapes, widening inside the call elsewhere)?  Calls that need no gradient do: torch.no_grad, inference_mode,
    operands without requires_grad.  Calls that need one take the typed training calls where _typed_training_applies holds; the others,
    return_quantiles and the mixed-supports route widen x and y first (_widen) and follow the float32 path unchanged.  mixed: the answer of
    mixed_route_applies where the caller has it already (_route)."""
    if return_quantiles or (mixed_route_applies(x, y, xpos, ypos) if mixed is None else mixed):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, xpos, ypos)))


def _typed_training_applies(x, y, xpos, ypos, return_quantiles=False, flags=0, p=1.0, mixed=None) -> bool:
    """bfloat16 weights that ask for a gradient: does the call take the typed backward / training form (sot_w1d_backward_bf16 /
    sot_w1d_loss_and_grad_bf16 -- 16-bit row loads and 16-bit gradient stores inside the backward kernels, no float32 image of a spectrum or
    of a gradient)?  It does when x or y requires a gradient and neither position tensor does, outside return_quantiles, the mixed-supports
    route and compiled calls, on the problems those kernels exist for (nat.bf16_native: shared positions, 512 / 1024 / 2048 / 4096 bins,
    16-byte aligned rows, not the opt-in tie-free form).  Everything else keeps the _widen route: there the C call would widen on the forward
    AND on the backward, two conversions more than _widen's.  A function of dtypes, shapes, strides, requires_grad, the grad mode, the flag
    word and the alignment of the two data pointers: no device is touched.  mixed: as in _typed_forward_applies."""
    if _compiling() or x.dtype is not torch.bfloat16 or y.dtype is not torch.bfloat16 or not torch.is_grad_enabled():
        return False
    if not (x.requires_grad or y.requires_grad) or xpos.requires_grad or ypos.requires_grad:
        return False
    if return_quantiles or xpos.ndim != 1 or ypos.ndim != 1 or (mixed_route_applies(x, y, xpos, ypos) if mixed is None else mixed):
        return False
    if x.ndim < 2 or y.ndim < 2 or x.shape[-1] != xpos.shape[0] or y.shape[-1] != ypos.shape[0]:
        return False    # (the general path says what is wrong with such a call)
    x2 = nat.rows_view(x.detach().reshape(-1, x.shape[-1]))   # the rows as _marshal hands them to the native call
    y2 = nat.rows_view(y.detach().reshape(-1, y.shape[-1]))
    return nat.bf16_native(x2, y2, xpos, ypos, p, flags)


ROW_SIDE_LIMIT = 16384    # points of ONE side (csrc/sot_launch.hpp pick_cfg: at most 1024 threads x 16 points per row)
ROW_POINT_LIMIT = 18000   # n + m of the longest row pair the kernels take for sure (one pair's working set lives in ONE CU's 160 KiB
                          # of LDS; include/sot_hip.h: SOT_ERR_UNSUPPORTED_SIZE beyond ~19000 forward / ~13000 backward)


def _beyond_one_cu(x, y, *positions) -> bool:
    """Rows too long for the LDS-resident kernels (n_fft >= 32768): the reference has no size limit (losses.py:223-313), so such GPU
    tensors run the package's torch-op composition -- said once -- instead of failing.  No paper configuration comes near."""
    n, m = x.shape[-1], y.shape[-1]
    if any(t is not None and t.ndim >= 2 and not (t.shape[0] > 1 and t.stride(0) == 0) for t in positions):
        # per-row positions are sorted in LDS on power-of-two arrays (csrc/sot_rows.hpp make_layout, rowpos)
        n, m = 1 << max(n - 1, 0).bit_length(), 1 << max(m - 1, 0).bit_length()
    wants_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, y) + tuple(positions))
    limit = ROW_POINT_LIMIT if not wants_grad else 12000
    if n + m <= limit and max(n, m) <= ROW_SIDE_LIMIT:   # the kernels also cap each side (pick_cfg: 1024 threads x 16 points)
        return False
    warn_once("row-too-long", f"sot_amd: rows of {n} + {m} points exceed what one CU's LDS holds; this call runs the torch-op composition "
                              "on the GPU instead of the HIP kernels")
    return True


def _fresh_grid_ok(pos, x, width) -> bool:
    """A caller-made position tensor the fresh-positions branch of Wasserstein1D.forward can hand to the C++ host path as it is."""
    return (pos.ndim == 1 and pos.shape[0] == width and pos.dtype is torch.float32 and pos.is_cuda and pos.device == x.device
            and pos.stride(0) == 1)


def _flags(square_dist, dont_normalize, limit_quantile_range, require_sort, prenormalized=False):
    return ((nat.FLAG_SQUARE if square_dist else 0) | (nat.FLAG_DONT_NORMALIZE if dont_normalize else 0)
            | (nat.FLAG_LIMIT_Q if limit_quantile_range else 0) | (nat.FLAG_REQUIRE_SORT if require_sort else 0)
            | (FLAG_PRENORMALIZED if prenormalized else 0))


def _position_grads(x, y, xpos, ypos, p, flags, plan, grad_rows, need_x, need_y, perm_in=None):
    """d sum_r grad_rows[r] * loss_r / d positions (losses.py:287-313: the positions enter through torch.sort and
    take_along_dim, both differentiable).  No reference call site asks for it; autograd supplies it, and so does
    this package: ONE deterministic HIP kernel (sot_w1d_position_grad: the merge walk accumulates
        d loss / d xs[i] = sum over the merged levels k whose x-rank is i of  delta_k * p |uq_k - vq_k|^(p-1) sign(uq_k - vq_k)
    and minus that for ys, no atomics) plus the fixed-order batch sum for a position row shared by all rows (sot_column_sum)."""
    try:
        return nat.position_grads(x, y, xpos, ypos, p, flags, grad_rows, need_x, need_y, plan, perm_in=perm_in)
    except nat.SotError as err:   # rows whose gradient layout + per-thread tails exceed one CU's LDS (n + m beyond ~12 000)
        if err.status != nat.SOT_ERR_UNSUPPORTED_SIZE:
            raise
        warn_once("posgrad-too-long", "sot_amd: position gradients of rows this long run as torch ops (atomic adds)")
        return _position_grads_torch(x, y, xpos, ypos, p, flags, plan, grad_rows, need_x, need_y)


def _position_grads_torch(x, y, xpos, ypos, p, flags, plan, grad_rows, need_x, need_y):
    """The same gradient from the quantile kernel's outputs with torch ops (searchsorted + scatter_add_): only for rows beyond the
    position-gradient kernel's LDS budget."""
    uq, vq, levels, cdf_x, cdf_y = nat.quantiles(x, y, xpos, ypos, p, flags, plan)
    rows, n = x.shape
    m = y.shape[1]
    delta = torch.diff(levels, dim=1, prepend=torch.zeros(rows, 1, device=x.device))
    if flags & nat.FLAG_LIMIT_Q:
        delta = torch.where(levels > 1, torch.zeros_like(delta), delta)
    d = uq - vq
    slope = torch.sign(d) if p == 1 else p * d.abs().pow(p - 1) * torch.sign(d)
    w = delta * slope * grad_rows.reshape(-1, 1)
    out = []
    for need, pos, cdf, width, sgn in ((need_x, xpos, cdf_x, n, 1.0), (need_y, ypos, cdf_y, m, -1.0)):
        if not need:
            out.append(None)
            continue
        rank = torch.searchsorted(cdf, levels).clamp_(max=width - 1)          # quantile_function, losses.py:214-220
        g_sorted = torch.zeros(rows, width, device=x.device).scatter_add_(1, rank, sgn * w)
        pos2 = pos if pos.ndim == 2 else pos.unsqueeze(0)
        if flags & nat.FLAG_REQUIRE_SORT:                                       # back through torch.sort (losses.py:286-288)
            order = torch.sort(pos2, dim=1)[1].expand(rows, width)
            g = torch.zeros_like(g_sorted).scatter_(1, order, g_sorted)
        else:
            g = g_sorted
        out.append(g.sum(0) if pos.ndim == 1 else g)
    return out


# element type of the weight rows -> (forward, backward, dtype of the row cotangents) of _RowLoss.  The functions are looked up on `nat` by
# name at call time (tests wrap them there).
_ROW_CALLS = {torch.float32: ("forward_rows", "backward_rows", torch.float32),
              torch.bfloat16: ("forward_rows_bf16", "backward_rows_bf16", torch.float32),
              torch.float64: ("forward_rows_f64", "backward_rows_f64", torch.float64)}


def _forward_rows(x, y, xpos, ypos, p, flags, plan, perm_out=None):
    """The plain row-loss call of x's element type (the float64 call takes sorted supports and no plan; only float32 rows leave permutations)."""
    fn = getattr(nat, _ROW_CALLS[x.dtype][0])
    if x.dtype is torch.float64:
        return fn(x, y, xpos, ypos, p, flags)
    return fn(x, y, xpos, ypos, p, flags, plan) if perm_out is None else fn(x, y, xpos, ypos, p, flags, plan, perm_out=perm_out)


class _RowLoss(torch.autograd.Function):
    """rows[B] = W_p^p per spectrum pair in the element type of the weight rows (_ROW_CALLS); backward = the closed-form HIP kernel of that
    type, only the gradients asked for.  bfloat16 rows come here where _typed_training_applies holds and float64 rows where
    _f64_route_applies does, so row permutations and position gradients are float32-only: per-row positions (the `torch.sort(u_values, 1)`
    of losses.py:286-288 on every row) are sorted ONCE per step -- the forward leaves each row's permutations in a uint16 buffer and the
    backward / position-gradient kernels gather through them (sot_problem.row_perm_out / row_perm_in)."""

    @staticmethod
    def forward(ctx, x, y, xpos, ypos, p, flags, plan):
        perm = None
        if x.dtype is torch.float32 and plan is None and any(ctx.needs_input_grad[:4]):
            perm = nat.row_permutations(x, y, xpos, ypos, flags)
        rows = _forward_rows(x, y, xpos, ypos, p, flags, plan, perm)
        ctx.save_for_backward(x, y, xpos, ypos, *([perm] if perm is not None else []))
        ctx.p, ctx.flags, ctx.plan = p, flags, plan
        return rows

    @staticmethod
    def backward(ctx, grad_rows):
        x, y, xpos, ypos, *perm = ctx.saved_tensors
        _, backward, cotangent = _ROW_CALLS[x.dtype]
        grad_rows = grad_rows.to(cotangent)
        extra = {} if x.dtype is torch.float64 else {"plan": ctx.plan}
        if perm:
            extra["perm_in"] = perm[0]
        gx = gy = gxp = gyp = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx, gy = getattr(nat, backward)(x, y, xpos, ypos, ctx.p, ctx.flags, grad_rows, need_gx=ctx.needs_input_grad[0],
                                            need_gy=ctx.needs_input_grad[1], **extra)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            gxp, gyp = _position_grads(x, y, xpos, ypos, ctx.p, ctx.flags, ctx.plan, grad_rows, ctx.needs_input_grad[2],
                                       ctx.needs_input_grad[3], perm_in=extra.get("perm_in"))
        return gx, gy, gxp, gyp, None, None, None


class _RowLossBF16(_RowLoss):
    """_RowLoss under the grad_fn name the typed training route has always shown (tests/golden/host_routes.json pins it)."""


class _RowLossF64(_RowLoss):
    """_RowLoss under the grad_fn name of the float64 route."""


_ROW_NODES = {torch.float32: _RowLoss, torch.bfloat16: _RowLossBF16, torch.float64: _RowLossF64}


F64_ROUTE = True   # module switch (tools/bench_f64.py times both routes): False = float64 GPU tensors run the torch-op composition as before
_F64_FLAGS = nat.FLAG_SQUARE | nat.FLAG_DONT_NORMALIZE | nat.FLAG_LIMIT_Q | nat.FLAG_PRENORMALIZED   # what the float64 kernels honour


def _f64_route_applies(x, y, xpos, ypos, return_quantiles=False) -> bool:
    """Does a call take the float64 kernels (sot_w1d_forward_f64 / sot_w1d_backward_f64)?  It does when all four tensors are float64 on ONE
    HIP device, neither position tensor asks for a gradient, the call is not return_quantiles, not the mixed-supports case (a shared grid
    against per-row positions) and not being traced, and the rows fit the kernels (nat.f64_supported: one pair's working set in one CU's
    LDS; the backward's when a gradient is asked for).  Everything else -- float32 positions, position gradients, quantiles, mixed supports,
    long rows, compiled calls -- keeps the torch-op composition and its one-time warning.  A function of dtypes, devices, shapes, strides,
    requires_grad and the grad mode: no device is touched."""
    if not F64_ROUTE or _compiling() or return_quantiles:
        return False
    ts = (x, y, xpos, ypos)
    if any(t is None or t.dtype is not torch.float64 or not _is_hip_tensor(t) or t.device != x.device for t in ts):
        return False
    grad_on = torch.is_grad_enabled()
    if grad_on and (xpos.requires_grad or ypos.requires_grad):
        return False
    if not (2 <= x.ndim <= 3 and x.ndim == y.ndim) or x.shape[:-1] != y.shape[:-1] or xpos.ndim > 3 or ypos.ndim > 3:
        return False
    n, m = x.shape[-1], y.shape[-1]
    if n < 1 or m < 1 or xpos.shape[-1] != n or ypos.shape[-1] != m:
        return False    # (the general path says what is wrong with such a call)
    shared = _is_shared_row(xpos)
    if shared != _is_shared_row(ypos):
        return False
    if not shared:
        rows = x.numel() // n
        if xpos.numel() != rows * n or ypos.numel() != rows * m:
            return False
    return nat.f64_supported(n, m, backward=grad_on and (x.requires_grad or y.requires_grad), per_row=not shared)


class _SortedGridCache:
    """Stable sorts of shared float64 position rows, keyed by tensor identity + version like _PlanCache: (sorted row, permutation), with the
    permutation None when the row was sorted already -- decided once per tensor version with one host synchronisation, outside stream
    capture (inside a capture of a grid not seen before, the sort and the gather are enqueued and nothing is remembered)."""

    def __init__(self, capacity=8):
        self.capacity = capacity
        self.entries = []   # (key, tensor ref, sorted row, permutation or None)

    def get(self, pos):
        key = (pos.data_ptr(), pos.numel(), _version_of(pos), pos.device)
        for k, _, srt, perm in self.entries:
            if k == key:
                return srt, perm
        row = pos.detach().contiguous()
        srt, perm = torch.sort(row, stable=True)
        if torch.cuda.is_current_stream_capturing():
            return srt, perm
        if bool((perm == torch.arange(perm.numel(), device=perm.device)).all()):
            srt, perm = row, None
        self.entries.append((key, pos, srt, perm))   # the tensor ref pins the storage behind data_ptr
        if len(self.entries) > self.capacity:
            self.entries.pop(0)
        return srt, perm


_f64_grids = _SortedGridCache()


def _f64_row_losses(route, x, y, xpos, ypos, p, flags):
    """The float64 route behind Wasserstein1D and wasserstein_1d (_f64_route_applies holds): flat [rows] float64 losses.  The kernels take
    sorted supports, so SOT_FLAG_REQUIRE_SORT is served here: a shared grid is sorted once per tensor version (_SortedGridCache; a grid
    that is sorted already -- the common case -- adds no torch kernel in front of the HIP call), per-row positions per call; the weights
    follow through differentiable gathers."""
    n, m = x.shape[-1], y.shape[-1]
    x2 = nat.rows_view(x.reshape(-1, n))
    y2 = nat.rows_view(y.reshape(-1, m))
    sort = bool(flags & nat.FLAG_REQUIRE_SORT)
    if _is_shared_row(xpos):
        xp = xpos if xpos.ndim == 1 else xpos.reshape(-1, n)[0]
        yp = ypos if ypos.ndim == 1 else ypos.reshape(-1, m)[0]
        if sort:
            xp, xperm = _f64_grids.get(xp)
            yp, yperm = _f64_grids.get(yp)
            if xperm is not None:
                x2 = x2.index_select(1, xperm)
            if yperm is not None:
                y2 = y2.index_select(1, yperm)
        else:
            xp, yp = xp.detach().contiguous(), yp.detach().contiguous()
    else:
        xp, yp = xpos.detach().reshape(-1, n), ypos.detach().reshape(-1, m)
        if sort:
            xp, xi = torch.sort(xp, dim=1, stable=True)
            yp, yi = torch.sort(yp, dim=1, stable=True)
            x2, y2 = torch.gather(x2, 1, xi), torch.gather(y2, 1, yi)
        else:
            xp, yp = xp.contiguous(), yp.contiguous()
    return _flat_rows(route, x2, y2, xp, yp, float(p), int(flags) & _F64_FLAGS, None)   # (the positions are detached: only x2, y2 can ask for a gradient)


MIXED_ROUTE = True   # module switch (tests and tools/bench_mixed.py compare both routes): False = mixed supports are materialised as before


def _is_shared_row(t) -> bool:
    """One position row for every batch row: a 1-D tensor, or a stride-0 expansion of one row (losses.py:167-170)."""
    if t.ndim == 1:
        return True
    lead = [(size, stride) for size, stride in zip(t.shape[:-1], t.stride()[:-1]) if size > 1]
    return len(lead) > 0 and all(stride == 0 for _, stride in lead)   # (len(): Dynamo does not trace bool() of a list)


def mixed_route_applies(x, y, xpos, ypos, return_quantiles=False) -> bool:
    """Does a call take the native mixed-supports route (sot_w1d_mixed_*: a shared grid on one side, [batch, (time,) K] positions per row
    on the other, nothing materialised)?  A function of shapes, strides, requires_grad, the grad mode and MIXED_ROUTE alone -- no device is
    touched.  Everything else keeps the materialising route: both sides of one kind, return_quantiles (the quantile kernels have no mixed
    form), a shared grid that itself needs a gradient (the mixed position gradient covers the per-row side only), a per-row side of more
    than nat.MIXED_ROW_SIDE_LIMIT points, and pairs beyond the kernels' LDS budget (include/sot_hip.h)."""
    if not MIXED_ROUTE or return_quantiles:
        return False
    x_shared = _is_shared_row(xpos)
    if x_shared == _is_shared_row(ypos):
        return False
    grid, rows = (xpos, ypos) if x_shared else (ypos, xpos)
    if rows.ndim not in (2, 3) or (torch.is_grad_enabled() and grid.requires_grad):
        return False
    n, m = x.shape[-1], y.shape[-1]
    k = m if x_shared else n
    pow2 = lambda v: 1 << max(v - 1, 0).bit_length()   # noqa: E731
    return 1 <= k <= nat.MIXED_ROW_SIDE_LIMIT and pow2(n) + pow2(m) <= nat.MIXED_POINT_LIMIT


def _marshal_mixed(x, y, xpos, ypos):
    """2-D weight rows, the shared side as its one 1-D row, the per-row side as contiguous [rows, K] (mixed_route_applies holds)."""
    x = nat.rows_view(x.reshape(-1, x.shape[-1]))
    y = nat.rows_view(y.reshape(-1, y.shape[-1]))
    if x.shape[0] != y.shape[0]:
        raise RuntimeError(f"row count mismatch: {x.shape[0]} vs {y.shape[0]}")
    if xpos.shape[-1] != x.shape[1] or ypos.shape[-1] != y.shape[1]:
        raise RuntimeError("positions and weights must have the same number of features")

    def one_side(pos):
        if _is_shared_row(pos):
            return pos.reshape(-1, pos.shape[-1])[0].contiguous() if pos.ndim > 1 else pos.contiguous()
        pos = pos.reshape(-1, pos.shape[-1]).contiguous()
        if pos.shape[0] != x.shape[0]:
            raise RuntimeError("per-row positions must have one row per weight row")
        return pos
    return x, y, one_side(xpos), one_side(ypos)


class _MixedRowLoss(torch.autograd.Function):
    """rows[B] = W_p^p per pair with ONE side on a shared grid and the other on per-row positions (sot_w1d_mixed_forward): the shared row
    is neither expanded nor sorted per row.  Backward: weight gradients of both sides (sot_w1d_mixed_backward) and the position gradient
    of the per-row side (sot_w1d_mixed_position_grad); the kernels sort the short per-row side again.  plan: the shared grid's
    PositionPlan (or None without require_sort).  The shared grid receives no gradient here (mixed_route_applies sends such calls to
    the materialising route)."""

    @staticmethod
    def forward(ctx, x, y, xpos, ypos, p, flags, plan):
        rows = nat.mixed_forward_rows(x, y, xpos, ypos, p, flags, plan)
        ctx.save_for_backward(x, y, xpos, ypos)
        ctx.p, ctx.flags, ctx.plan = p, flags, plan
        return rows

    @staticmethod
    def backward(ctx, grad_rows):
        x, y, xpos, ypos = ctx.saved_tensors
        x_shared = xpos.ndim == 1
        if ctx.needs_input_grad[2 if x_shared else 3]:
            raise RuntimeError("sot_amd: the mixed-supports route has no gradient for the shared grid")
        gx = gy = gpos = None
        g = grad_rows.float()
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx, gy = nat.mixed_backward_rows(x, y, xpos, ypos, ctx.p, ctx.flags, g, need_gx=ctx.needs_input_grad[0],
                                             need_gy=ctx.needs_input_grad[1], plan=ctx.plan)
        if ctx.needs_input_grad[3 if x_shared else 2]:
            gpos = nat.mixed_position_grad(x, y, xpos, ypos, ctx.p, ctx.flags, g, plan=ctx.plan)
        return gx, gy, (None if x_shared else gpos), (gpos if x_shared else None), None, None, None


def _mixed_row_losses(x, y, xpos, ypos, p, flags, plans):
    """The mixed-supports route behind Wasserstein1D.row_losses and wasserstein_1d; plans: the caller's _PlanCache (the shared grid is
    planned once per tensor version, as on the all-shared route)."""
    x, y, xpos, ypos = _marshal_mixed(x, y, xpos, ypos)
    grid = xpos if xpos.ndim == 1 else ypos
    if _compiling():
        return _o.w1d_rows(x, y, xpos, ypos, float(p), flags)
    plan = plans.get(grid, grid) if (flags & nat.FLAG_REQUIRE_SORT) else None
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, xpos, ypos)):
        return _MixedRowLoss.apply(x, y, xpos, ypos, float(p), flags, plan)
    return nat.mixed_forward_rows(x, y, xpos, ypos, float(p), flags, plan)


class _Quantiles(torch.autograd.Function):
    """The five return_quantiles tensors (uq, vq, Q, U, V: losses.py:198-201, 299-300) with their vector-Jacobian product
    (sot_w1d_quantiles_backward: one HIP kernel, one merge walk for weights and positions).  In the reference these tensors come from
    plain ATen ops and stay attached to autograd -- they are its extension point for a ground cost other than |uq - vq|^p.  Per-row
    positions are sorted once: the forward leaves the rows' permutations behind and the backward gathers through them, as in _RowLoss."""

    @staticmethod
    def forward(ctx, x, y, xpos, ypos, p, flags, plan):
        perm = nat.row_permutations(x, y, xpos, ypos, flags) if plan is None else None
        out = nat.quantiles(x, y, xpos, ypos, p, flags, plan, perm_out=perm)
        ctx.save_for_backward(x, y, xpos, ypos, *([perm] if perm is not None else []))
        ctx.p, ctx.flags, ctx.plan = p, flags, plan
        ctx.set_materialize_grads(False)   # an output the caller's loss does not use arrives as None -> NULL: no traffic
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        x, y, xpos, ypos, *perm = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:4])
        if all(g is None for g in grads):
            return (None,) * 7
        grads = [None if g is None else g.float() for g in grads]
        gx, gy, gxp, gyp = nat.quantiles_backward(x, y, xpos, ypos, ctx.p, ctx.flags, grads, need, ctx.plan,
                                                  perm_in=perm[0] if perm else None)
        return gx, gy, gxp, gyp, None, None, None


EARLY_GRADIENT = True   # module switch for the loss-and-gradient form below (tests compare both forms)


class _FusedMeanLoss(torch.autograd.Function):
    """losses.py:129-211 with dims=None behind ONE native call (forward kernel + fixed-order batch-mean kernel); the backward feeds the
    scalar upstream gradient to the HIP backward kernel as a broadcast value scaled by 1/B.

    When only y needs a gradient (the training step: x is the target spectrum) the gradient of the mean is computed
    together with the loss (sot_w1d_loss_and_grad: one pass over the rows instead of forward + backward) and only rescaled
    by the upstream scalar in backward (a no-op kernel for a plain ``loss.backward()``)."""

    @staticmethod
    def forward(ctx, x, y, xpos, ypos, p, flags, plan):
        """Shared by _FusedMeanLossBF16: the calls of the rows' element type, looked up on `nat` by name at call time."""
        typed = "_bf16" if x.dtype is torch.bfloat16 else ""
        ctx.p, ctx.flags, ctx.plan = p, flags, plan
        ctx.early_gy = None
        if ctx.needs_input_grad[1] and not ctx.needs_input_grad[0] and EARLY_GRADIENT:
            mean, _, ctx.early_gy = getattr(nat, "loss_and_grad" + typed)(x, y, xpos, ypos, p, flags, plan)
        else:
            mean = getattr(nat, "loss_fused" + typed)(x, y, xpos, ypos, p, flags, plan)[0]
        ctx.save_for_backward(x, y, xpos, ypos)
        return mean

    @staticmethod
    def backward(ctx, g):
        x, y, xpos, ypos = ctx.saved_tensors
        gxp = gyp = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            gxp, gyp = _position_grads(x, y, xpos, ypos, ctx.p, ctx.flags, ctx.plan, (g.float() / x.shape[0]).expand(x.shape[0]),
                                       ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        if ctx.early_gy is not None:   # consumed once: a second backward through a retained graph recomputes below
            gy, ctx.early_gy = ctx.early_gy, None
            return None, nat.scale_inplace(gy, g.float().contiguous()), gxp, gyp, None, None, None
        gx = gy = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx, gy = nat.backward_rows(x, y, xpos, ypos, ctx.p, ctx.flags, g.float(), need_gx=ctx.needs_input_grad[0],
                                       need_gy=ctx.needs_input_grad[1], plan=ctx.plan, grad_scale=1.0 / x.shape[0])
        return gx, gy, gxp, gyp, None, None, None


class _FusedMeanLossBF16(_FusedMeanLoss):
    """_FusedMeanLoss for bfloat16 weights where _typed_training_applies holds: its forward, a backward of its own.  The training step (only y asks for a gradient) is ONE node on
    16-bit data: its forward is sot_w1d_loss_and_grad_bf16, which stores d mean / d y in bfloat16 before the upstream gradient is known; its
    backward calls the typed backward in fix-up mode on that buffer with the upstream scalar -- an empty launch for a plain loss.backward(),
    a recomputation into the buffer for a weighted loss -- which returns the float32 node's bits rounded once: rne(early gradient * upstream).
    Otherwise (x differentiated, EARLY_GRADIENT off, a second backward through a retained graph): the typed forward + mean, and the typed
    backward with the float32 node's late arguments."""

    @staticmethod
    def backward(ctx, g):
        x, y, xpos, ypos = ctx.saved_tensors
        scale = 1.0 / x.shape[0]
        if ctx.early_gy is not None:   # consumed once, as in _FusedMeanLoss
            gy, ctx.early_gy = ctx.early_gy, None
            nat.backward_rows_bf16(x, y, xpos, ypos, ctx.p, ctx.flags, None, need_gx=False, need_gy=True, plan=ctx.plan, grad_scale=scale,
                                   rescale=g.float().reshape(1), gy_out=gy)
            return None, gy, None, None, None, None, None
        gx, gy = nat.backward_rows_bf16(x, y, xpos, ypos, ctx.p, ctx.flags, g.float(), need_gx=ctx.needs_input_grad[0],
                                        need_gy=ctx.needs_input_grad[1], plan=ctx.plan, grad_scale=scale)
        return gx, gy, None, None, None, None, None


class _RowMean(torch.autograd.Function):
    """losses.py:211 with dims=None: fixed-order fp64 accumulation on the GPU."""

    @staticmethod
    def forward(ctx, rows):
        ctx.count = rows.numel()
        return nat.reduce_mean(rows)

    @staticmethod
    def backward(ctx, g):
        return (g / ctx.count).expand(ctx.count)


def _version_of(t):
    try:
        return t._version
    except RuntimeError:  # inference tensors (metrics.py:144 runs under inference_mode) are immutable
        return -1


class _PlanCache:
    """Position plans keyed by tensor identity+version, so a persistent grid is sorted once."""

    def __init__(self, capacity=4):
        self.capacity = capacity
        self.entries = []  # (key, xpos_ref, ypos_ref, plan)

    def get(self, xpos, ypos):
        key = (xpos.data_ptr(), ypos.data_ptr(), xpos.numel(), ypos.numel(), _version_of(xpos), _version_of(ypos),
               xpos.device)
        for k, _, _, plan in self.entries:
            if k == key:
                return plan
        plan = nat.PositionPlan(xpos.detach(), ypos.detach())
        self.entries.append((key, xpos, ypos, plan))  # tensor refs pin the storage behind data_ptr
        if len(self.entries) > self.capacity:
            self.entries.pop(0)
        return plan


_functional_plans = _PlanCache()


class _Route(typing.NamedTuple):
    """Where one call goes, decided once by _route() (DESIGN.md section 1.1 has the table)."""
    family: str                    # "torch": the torch-op composition; "f64": the float64 kernels; "mixed": mixed supports; "rows": the row kernels
    dtype: torch.dtype             # element type of the weight rows the native call sees (float32 / bfloat16; float64 on "f64")
    widen: bool = False            # bfloat16 operands are widened first: by _widen on "mixed" / "rows", by .float() on "torch"
    typed_training: bool = False   # bfloat16 rows that ask for a gradient on the typed training calls (_typed_training_applies)


_ROUTE_F64 = _Route("f64", torch.float64)


def _route(x, y, xpos, ypos, p, flags, return_quantiles=False) -> _Route:
    """The gates in their one order, each asked at most once: the float64 gate before _hip_domain can warn, _hip_domain (which refuses half,
    dtype mixes and bfloat16 positions), _beyond_one_cu, mixed supports, then -- for bfloat16 weights -- the typed forward, the typed
    training calls, or widening.  Every device test goes through _is_hip_tensor, so meta stand-ins answer too."""
    if x.dtype is torch.float64 and _f64_route_applies(x, y, xpos, ypos, return_quantiles):
        return _ROUTE_F64
    if not _hip_domain(x, y, xpos, ypos):
        return _Route("torch", x.dtype)
    bf16 = x.dtype is torch.bfloat16
    if _beyond_one_cu(x, y, xpos, ypos):
        return _Route("torch", torch.float32, widen=bf16)   # (rows beyond one CU's LDS: the composition on the upcast weights)
    mixed = mixed_route_applies(x, y, xpos, ypos, return_quantiles)
    typed_forward = bf16 and _typed_forward_applies(x, y, xpos, ypos, return_quantiles, mixed)
    training = bf16 and not typed_forward and _typed_training_applies(x, y, xpos, ypos, return_quantiles, flags, p, mixed)
    # quantiles, mixed supports, position gradients, rows without 16-bit backward kernels: the float32 path, gradients narrowed
    widen = bf16 and not typed_forward and not training
    return _Route("mixed" if mixed else "rows", torch.bfloat16 if bf16 and not widen else torch.float32, widen, training)


def _marshal_rows(x, y, xpos, ypos, flags, plans, functional=False):
    """What the native row calls take: 2-D weight rows, matching positions and the position plan of a shared grid that is to be sorted
    (traced: the op plans).  The module flattens [batch, time, bins] operands and materialises stride-0 expanded positions per row; the
    functional form takes 2-D rows only and passes expanded positions (losses.py:167-170) down as one shared row.  Both habits are
    older than this function and pinned by tests/golden/host_routes.json, so they are kept apart."""
    if functional:
        xpos, ypos = [t[0] if (t.ndim == 2 and t.shape[0] > 1 and t.stride(0) == 0) else t for t in (xpos, ypos)]
    else:
        x, y, xpos, ypos = [t.reshape(-1, t.shape[-1]) if t.ndim == 3 else t for t in (x, y, xpos, ypos)]
    if x.ndim != 2 or y.ndim != 2:
        raise ValueError(f"expected 2-D [rows, features] weights, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[0] != y.shape[0]:
        raise RuntimeError(f"row count mismatch: {x.shape[0]} vs {y.shape[0]}")
    x, y = nat.rows_view(x), nat.rows_view(y)
    if xpos.shape[-1] != x.shape[1] or ypos.shape[-1] != y.shape[1]:
        raise RuntimeError("positions and weights must have the same number of features")
    if (xpos.ndim == 1) != (ypos.ndim == 1):  # mixed supports outside the mixed route: materialise the shared row for every batch row
        if xpos.ndim == 1:
            xpos = xpos.unsqueeze(0).expand_as(x)
        else:
            ypos = ypos.unsqueeze(0).expand_as(y)
    if xpos.ndim == 2 and (xpos.shape[0] != x.shape[0] or ypos.shape[0] != y.shape[0]):
        raise RuntimeError("per-row positions must have one row per weight row")
    xpos, ypos = xpos.contiguous(), ypos.contiguous()
    plan = plans.get(xpos, ypos) if (flags & nat.FLAG_REQUIRE_SORT and xpos.ndim == 1 and not _compiling()) else None
    return x, y, xpos, ypos, plan


def _flat_rows(route, x, y, xpos, ypos, p, flags, plan):
    """The one ladder of the flat row losses, on marshalled rows of the route's element type: the op of a call that is being traced, the
    autograd node where a gradient can be asked for, the plain native call otherwise."""
    if _compiling():
        return (_o.w1d_rows_bf16 if route.dtype is torch.bfloat16 else _o.w1d_rows)(x, y, xpos, ypos, p, flags)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, xpos, ypos)):
        return _ROW_NODES[route.dtype].apply(x, y, xpos, ypos, p, flags, plan)
    return _forward_rows(x, y, xpos, ypos, p, flags, plan)


def _native_row_losses(route, x, y, xpos, ypos, p, flags, plans, functional=False):
    """Flat [rows] losses of a call whose route is not the composition: behind wasserstein_1d, Wasserstein1D.row_losses and the dims /
    hinge tail of Wasserstein1D.forward."""
    if route.family == "f64":
        return _f64_row_losses(route, x, y, xpos, ypos, p, flags)
    if route.widen:
        x, y = _widen(x), _widen(y)
    if route.family == "mixed":   # a shared grid against per-row positions: nothing is materialised
        return _mixed_row_losses(x, y, xpos, ypos, p, flags, plans)
    x, y, xpos, ypos, plan = _marshal_rows(x, y, xpos, ypos, flags, plans, functional)
    return _flat_rows(route, x, y, xpos, ypos, float(p), flags, plan)


def _native_quantiles(route, x, y, xpos, ypos, p, flags, plans, functional=False):
    """return_quantiles on the row kernels (the gates send such a call to no other native family), five [rows, .] tensors: the op of a
    traced call, through autograd when a gradient can be asked for, the plain native call otherwise."""
    if route.widen:
        x, y = _widen(x), _widen(y)
    x, y, xpos, ypos, plan = _marshal_rows(x, y, xpos, ypos, flags, plans, functional)
    if _compiling():
        return _o.w1d_quantiles(x, y, xpos, ypos, float(p), flags)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, y, xpos, ypos)):
        return _Quantiles.apply(x, y, xpos, ypos, float(p), flags, plan)
    return nat.quantiles(x, y, xpos, ypos, float(p), flags, plan)


def quantile_function(qs, cws, xs):
    """losses.py:214-220.  Compatibility helper only: inside this package the inverse-CDF lookup is
    fused into the merge kernel and this function is never called on the hot path."""
    n = xs.shape[1]
    idx = torch.searchsorted(cws, qs)
    return torch.take_along_dim(xs, torch.clamp(idx, 0, n - 1), dim=1)


def wasserstein_1d(u_values, v_values, u_weights=None, v_weights=None, p=1, require_sort=True,
                   return_quantiles=False, limit_quantile_range=False):
    """losses.py:223-313: W_p^p per row of two discrete measures (weights used as given)."""
    assert p >= 1, f"The OT loss is only valid for p>=1, {p} was given"
    n, m = u_values.shape[1], v_values.shape[1]
    if u_weights is None:
        u_weights = torch.full(u_values.shape, 1.0 / n, device=u_values.device, dtype=u_values.dtype)
    if v_weights is None:
        v_weights = torch.full(v_values.shape, 1.0 / m, device=v_values.device, dtype=v_values.dtype)
    flags = _flags(False, False, limit_quantile_range, require_sort, prenormalized=True)
    route = _route(u_weights, v_weights, u_values, v_values, p, flags, return_quantiles)
    if route.family == "torch":
        if route.widen:
            u_weights, v_weights = u_weights.float(), v_weights.float()
        return tp.transport_rows(u_values, v_values, u_weights, v_weights, p=p, require_sort=require_sort,
                                 return_quantiles=return_quantiles, limit_quantile_range=limit_quantile_range)
    if return_quantiles:
        return _native_quantiles(route, u_weights, v_weights, u_values, v_values, p, flags, _functional_plans, functional=True)
    return _native_row_losses(route, u_weights, v_weights, u_values, v_values, p, flags, _functional_plans, functional=True)


def _csr_to_padded(weights, positions, offsets, width):
    """CSR entries -> [rows, width] weights (zeros behind each row's entries: zero-weight points are inert) and positions (the
    row's last position repeated), plus the mask of real entries (row-major = CSR order)."""
    starts, ends = offsets[:-1, None], offsets[1:, None]
    idx = starts + torch.arange(width, device=offsets.device)[None, :]
    valid = idx < ends
    idx = torch.minimum(idx, (ends - 1).clamp_min(0)).clamp_(0, max(weights.numel() - 1, 0))
    return torch.where(valid, weights[idx], torch.zeros((), device=weights.device)), positions[idx], valid


class _CsrRowLoss(torch.autograd.Function):
    """Row losses of the CSR form (sot_w1d_forward_csr).  Backward: the rows are padded with zero-weight points to
    [rows, max_n] / [rows, max_m] with per-row positions and go through the dense backward kernel (the same function of the kept
    weights, hence the same gradient); the gradients of the kept points are gathered back into CSR order."""

    @staticmethod
    def forward(ctx, xw, xp, xoff, yw, yp, yoff, max_n, max_m, p, flags):
        rows = nat.forward_rows_csr(xw, xp, xoff, yw, yp, yoff, max_n, max_m, p, flags)
        ctx.save_for_backward(xw, xp, xoff, yw, yp, yoff)
        ctx.cfg = (max_n, max_m, p, flags)
        return rows

    @staticmethod
    def backward(ctx, grad_rows):
        xw, xp, xoff, yw, yp, yoff = ctx.saved_tensors
        max_n, max_m, p, flags = ctx.cfg
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[4]:
            raise NotImplementedError("gradients w.r.t. support positions are not implemented (no reference call site uses them)")
        xd, xpd, xvalid = _csr_to_padded(xw, xp, xoff, max_n)
        yd, ypd, yvalid = _csr_to_padded(yw, yp, yoff, max_m)
        gx, gy = nat.backward_rows(xd, yd, xpd.contiguous(), ypd.contiguous(), p, flags, grad_rows.float(),
                                   need_gx=ctx.needs_input_grad[0], need_gy=ctx.needs_input_grad[3])
        return (gx[xvalid] if gx is not None else None, None, None, gy[yvalid] if gy is not None else None, None, None,
                None, None, None, None)


def wasserstein_1d_csr(x_weights, x_positions, x_offsets, y_weights, y_positions, y_offsets, max_n, max_m, p=1,
                       square_dist=False, dont_normalize=False, limit_quantile_range=False, require_sort=True,
                       prenormalized=False):
    """Per-row SOT loss for RAGGED supports in CSR form (no reference counterpart: the reference is fed zero-masked
    dense rows, which give the same value because zero-weight points are inert -- BASELINE config 4).
    Row r owns entries [offsets[r], offsets[r+1]); normalisation etc. follow Wasserstein1D's keyword arguments.
    Returns the [rows] tensor of W_p^p; differentiable w.r.t. the weights (see _CsrRowLoss)."""
    assert p >= 1, f"The OT loss is only valid for p>=1, {p} was given"
    flags = _flags(square_dist, dont_normalize, limit_quantile_range, require_sort, prenormalized)
    if torch.is_grad_enabled() and (x_weights.requires_grad or y_weights.requires_grad):
        return _CsrRowLoss.apply(x_weights, x_positions, x_offsets, y_weights, y_positions, y_offsets, int(max_n), int(max_m),
                                 float(p), flags)
    return nat.forward_rows_csr(x_weights, x_positions, x_offsets, y_weights, y_positions, y_offsets, max_n, max_m,
                                float(p), flags)


class _HotCall(typing.NamedTuple):
    """What Wasserstein1D.forward remembers of its last default call (round-5 review: a 13-slot positional tuple before)."""
    x_pos: torch.Tensor          # the position tensors of that call, by identity ...
    y_pos: torch.Tensor
    x_version: int               # ... and their in-place-modification counters then
    y_version: int
    settings: tuple              # Wasserstein1D._settings() then
    plan: object                 # the position plan (sorted grids, permutations, identity flags)
    flag_word: int               # the call's flag word as the library takes it (with SOT_FLAG_SAME_GRID where the plan says so)
    glue: object                 # the C++ host path (_sot_glue)
    n: int                       # row lengths
    m: int
    fresh_ok: bool               # the fresh-positions branch applies: caller-passed positions (not the fixed_x buffer) and the extension has mean_loss_fresh
    flags_no_same_grid: int      # the flag word without the same-grid bit (two fresh tensors: the C++ side puts it back when both are one tensor)
    area_ok: bool                # the merge-free kernel may be asked for (p = 1, no cutoff)


class Wasserstein1D(torch.nn.Module):
    """Drop-in for losses.Wasserstein1D (losses.py:89-211); see that docstring for the arguments."""

    def __init__(self, p=1, fixed_x=None, require_sort=True, log_scaled_x=False, **kwargs):
        super().__init__()
        self.p = p
        self.require_sort = require_sort
        self.log_scaled_x = log_scaled_x  # flag only, like the reference (trainer.py:187 reads it)
        self.dont_normalize = kwargs.get("dont_normalize", False)
        self.limit_quantile_range = kwargs.get("limit_quantile_range", False)
        self.hinge = kwargs.get("hinge", False)
        self.square_dist = kwargs.get("square_dist", False)
        # NOT a reference argument (default: the reference's behaviour).  True: for p = 1 on one grid the gradient w.r.t. y comes from the
        # merge-free training form -- the derivative of the loss in the CDF values, which is what float64 autograd of the reference
        # returns; at exactly tied float32 levels the reference's float32 autograd returns a tie-order artefact instead
        self.tie_free_gradient = bool(kwargs.get("tie_free_gradient", False))
        # unknown kwargs (e.g. cumsum_only from the paper YAMLs) are accepted and ignored, losses.py:96
        if fixed_x is not None:
            self.register_buffer("fixed_x", torch.linspace(0, 1, fixed_x))
        else:
            self.register_buffer("fixed_x", None)
        self._plans = _PlanCache()
        self._hot = None   # the last default call, a _HotCall: see forward

    def __getstate__(self):
        # the caches hold device events and the extension module: a copy / pickle of the module (copy.deepcopy for an EMA model,
        # torch.save(model)) starts with empty ones
        state = self.__dict__.copy()
        state["_plans"] = None
        state["_hot"] = None
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plans = _PlanCache()
        self._hot = None

    def _positions(self, x_pos, y_pos):
        if (x_pos is None or y_pos is None) and self.fixed_x is None:
            raise ValueError("If fixed_x is not provided, x_pos and y_pos must be provided")
        assert self.p >= 1, f"The OT loss is only valid for p>=1, {self.p} was given"  # losses.py:271
        return (self.fixed_x if x_pos is None else x_pos), (self.fixed_x if y_pos is None else y_pos)

    def _flag_word(self, kwargs):
        dont_normalize = bool(kwargs.get("dont_normalize", False) or self.dont_normalize)
        limit_q = bool(kwargs.get("limit_quantile_range", False) or self.limit_quantile_range)
        flags = _flags(self.square_dist, dont_normalize, limit_q, self.require_sort)
        if getattr(self, "tie_free_gradient", False):
            flags |= nat.FLAG_TIE_FREE_GRADIENT
        return flags

    def _marshal(self, x, y, x_pos, y_pos, kwargs):
        """HIP-domain tensors -> what the native calls take: 2-D rows, positions, flag word, position plan (and the leading shape)."""
        x_pos_, y_pos_ = self._positions(x_pos, y_pos)
        flags = self._flag_word(kwargs)
        x2, y2, x_pos_, y_pos_, plan = _marshal_rows(x, y, x_pos_, y_pos_, flags, self._plans)
        return x2, y2, x_pos_, y_pos_, flags, plan, x.shape[:-1]

    def _torch_forward(self, route, x, y, x_pos_, y_pos_, kwargs, rows_only=False):
        """CPU / float64 tensors: the torch-op composition (_torch_path.py), same keyword handling as the HIP route."""
        if route.widen:   # (bfloat16 rows beyond one CU's LDS: on the upcast weights)
            x, y = x.float(), y.float()
        return tp.module_forward(
            x, y, x_pos_, y_pos_, p=self.p, square_dist=self.square_dist,
            dont_normalize=bool(kwargs.get("dont_normalize", False) or self.dont_normalize),
            limit_quantile_range=bool(kwargs.get("limit_quantile_range", False) or self.limit_quantile_range),
            require_sort=self.require_sort, hinge_on=bool(self.hinge), hinge_value=kwargs.get("hinge", 0.0),
            dims=(0 if rows_only else kwargs.get("dims", None)), return_quantiles=(not rows_only) and kwargs.get("return_quantiles", False),
            rows_only=rows_only)

    def _rows(self, route, x, y, x_pos_, y_pos_, flags, kwargs):
        """The flat row losses of a routed call after the optional hinge."""
        if route.family == "torch":
            return self._torch_forward(route, x, y, x_pos_, y_pos_, kwargs, rows_only=True)
        loss = _native_row_losses(route, x, y, x_pos_, y_pos_, self.p, flags, self._plans)
        if self.hinge:
            loss = torch.nn.functional.relu(loss - kwargs.get("hinge", 0.0))
        return loss

    def row_losses(self, x, y, x_pos=None, y_pos=None, **kwargs):
        """Flat [rows] tensor of W_p^p per spectrum pair (after the optional hinge, before the mean):
        what losses.py:186-205 holds before its reshape/mean.  Used by the row-sharded multi-GPU path."""
        x_pos_, y_pos_ = self._positions(x_pos, y_pos)
        flags = self._flag_word(kwargs)
        return self._rows(_route(x, y, x_pos_, y_pos_, self.p, flags), x, y, x_pos_, y_pos_, flags, kwargs)

    def _fused_mean(self, route, x, y, x_pos_, y_pos_, flags, fresh_grids, kwargs):
        """Default reduction on the row kernels: forward and the mean over every row (losses.py:211) in one native call.  fresh_grids: both
        position tensors came with the call (not the fixed_x buffer)."""
        if route.widen:
            x, y = _widen(x), _widen(y)
        x2, y2, x_pos_, y_pos_, plan = _marshal_rows(x, y, x_pos_, y_pos_, flags, self._plans)
        p, typed = float(self.p), route.dtype is torch.bfloat16   # typed: _typed_training_applies held, or no gradient is asked for
        grad_on = torch.is_grad_enabled()
        if _compiling():   # the native calls below, as ops: the training form when only y (and positions) ask for a gradient
            if typed:
                return _o.w1d_mean_bf16(x2, y2, x_pos_, y_pos_, p, flags)
            if grad_on and EARLY_GRADIENT and y2.requires_grad and not x2.requires_grad:
                return _o.w1d_mean_and_grad(x2, y2, x_pos_, y_pos_, p, flags)[0]
            return _o.w1d_mean(x2, y2, x_pos_, y_pos_, p, flags)
        glue = nat.glue() if (plan is not None and EARLY_GRADIENT and not typed) else None
        if glue is not None and not (grad_on and (x2.requires_grad or x_pos_.requires_grad or y_pos_.requires_grad)):
            # the hot call (trainer.py:220-228: gradient for the estimate's spectrum only; metrics.py:148: none): C++ host path
            plan.use_on_current_stream(x2.device)
            fl = nat.problem_flags(self.p, flags, plan)
            # remember the hot call (see forward) -- not from inside a stream capture, where plan.same_grid() answers "no" without
            # remembering it and the flag word frozen here would lack SOT_FLAG_SAME_GRID for good
            if (not kwargs and x_pos_.ndim == 1 and y_pos_.ndim == 1 and x2.shape[1] + y2.shape[1] <= 12000
                    and not torch.cuda.is_current_stream_capturing()):
                self._hot = _HotCall(
                    x_pos=x_pos_, y_pos=y_pos_, x_version=_version_of(x_pos_), y_version=_version_of(y_pos_), settings=self._settings(), plan=plan,
                    flag_word=fl, glue=glue, n=x2.shape[1], m=y2.shape[1],
                    fresh_ok=fresh_grids and hasattr(glue, "mean_loss_fresh"), flags_no_same_grid=int(flags),
                    area_ok=self.p == 1 and not (flags & (nat.FLAG_LIMIT_Q | nat.FLAG_NO_AREA | nat.FLAG_PRENORMALIZED)))
            return glue.mean_loss(x2, y2, plan.xpos_sorted, plan.ypos_sorted, plan.xperm, plan.yperm, plan.ident, p, fl)
        if grad_on and any(t.requires_grad for t in (x2, y2, x_pos_, y_pos_)):
            return (_FusedMeanLossBF16 if route.typed_training else _FusedMeanLoss).apply(x2, y2, x_pos_, y_pos_, p, flags, plan)
        return getattr(nat, "loss_fused_bf16" if typed else "loss_fused")(x2, y2, x_pos_, y_pos_, p, flags, plan)[0]

    def _settings(self):
        return (self.p, self.square_dist, self.dont_normalize, self.limit_quantile_range, self.require_sort, self.hinge,
                getattr(self, "tie_free_gradient", False))

    def forward(self, x, y, x_pos=None, y_pos=None, **kwargs):
        # The hot call, recognised before anything else is looked at: the SAME position tensors as last time (a persistent grid or the
        # fixed_x buffer), no call keywords, float32 GPU rows -> straight into the C++ host path with the cached plan and flag word.
        # Everything the general path below would re-derive per call (domain check, reshapes of positions, flags, plan lookup) was
        # derived when the entry was made; the C++ side checks the weight tensors themselves.
        hot = None if _compiling() else self._hot
        if (hot is not None and EARLY_GRADIENT and not kwargs and x.dtype is torch.float32 and y.dtype is torch.float32 and x.is_cuda
                and y.is_cuda):
            xp = self.fixed_x if x_pos is None else x_pos
            yp = self.fixed_x if y_pos is None else y_pos
            if (xp is hot.x_pos and yp is hot.y_pos and _version_of(xp) == hot.x_version and _version_of(yp) == hot.y_version and self._settings() == hot.settings
                    and 2 <= x.ndim <= 3 and x.ndim == y.ndim):
                x2 = x if x.ndim == 2 else x.reshape(-1, x.shape[-1])
                y2 = y if y.ndim == 2 else y.reshape(-1, y.shape[-1])
                if (x2.stride(1) == 1 and y2.stride(1) == 1 and x2.shape[1] == hot.n and y2.shape[1] == hot.m
                        and not (torch.is_grad_enabled() and (x2.requires_grad or xp.requires_grad or yp.requires_grad))):
                    plan = hot.plan
                    plan.use_on_current_stream(x2.device)
                    return hot.glue.mean_loss(x2, y2, plan.xpos_sorted, plan.ypos_sorted, plan.xperm, plan.yperm, plan.ident, float(self.p), hot.flag_word)
            elif (x_pos is not None and y_pos is not None and self._settings() == hot.settings and 2 <= x.ndim <= 3 and x.ndim == y.ndim
                  and hot.fresh_ok and _fresh_grid_ok(xp, x, hot.n) and _fresh_grid_ok(yp, x, hot.m)):
                # FRESH position tensors of the shapes seen last time -- the reference's trainer rebuilds its grid on every step
                # (trainer.py:187-197: x_pos = torch.tensor(freqs).to(device) / max, y_pos = x_pos.clone()).  Their content cannot be
                # compared on the host without a synchronisation, so the call gets its own plan, but inside the SAME C++ call as the loss
                # (one allocation, one two-workgroup launch in front of the row kernel): no Python plan object, no cache bookkeeping, no
                # general path.  flags_no_same_grid: the flag word WITHOUT the same-grid bit (whether two fresh tensors hold one grid is device-side
                # knowledge; the C++ side puts it back when both arguments are one tensor).
                x2 = x if x.ndim == 2 else x.reshape(-1, x.shape[-1])
                y2 = y if y.ndim == 2 else y.reshape(-1, y.shape[-1])
                if (x2.stride(1) == 1 and y2.stride(1) == 1 and x2.shape[1] == hot.n and y2.shape[1] == hot.m
                        and not (torch.is_grad_enabled() and (x2.requires_grad or xp.requires_grad or yp.requires_grad))):
                    return hot.glue.mean_loss_fresh(x2, y2, xp, yp, float(self.p), hot.flags_no_same_grid | (nat.FLAG_SAME_GRID if (xp is yp and hot.area_ok) else 0))
        x_pos_, y_pos_ = self._positions(x_pos, y_pos)
        flags = self._flag_word(kwargs)
        quantiles = kwargs.get("return_quantiles", False)
        route = _route(x, y, x_pos_, y_pos_, self.p, flags, quantiles)
        if route.family == "torch":
            return self._torch_forward(route, x, y, x_pos_, y_pos_, kwargs)
        if quantiles:
            out = _native_quantiles(route, x, y, x_pos_, y_pos_, self.p, flags, self._plans)
            return [t.reshape(x.shape[:-1] + (-1,)) for t in out]
        dims = kwargs.get("dims", None)
        if route.family == "rows" and dims is None and not self.hinge:
            return self._fused_mean(route, x, y, x_pos_, y_pos_, flags, x_pos is not None and y_pos is not None, kwargs)
        loss = self._rows(route, x, y, x_pos_, y_pos_, flags, kwargs)
        if dims is None and route.family != "f64":   # (float64 row losses: the mean stays a torch op, losses.py:203-211)
            return _o.row_mean(loss) if _compiling() else _RowMean.apply(loss)  # torch.mean over every row -> 0-d tensor (losses.py:211)
        return torch.mean(loss.reshape(x.shape[:-1]), dim=dims)


class _MultiScaleSpectral(torch.autograd.Function):
    """MSSLoss behind ONE autograd node: per FFT size two STFT-magnitude kernels and the spectral-distance kernels
    (include/sot_hip.h: sot_stft_mag_*, sot_spec_distance_*); the backward walks the scales again (distance backward ->
    STFT backward) and accumulates the audio gradients."""

    @staticmethod
    def forward(ctx, target_audio, audio, fft_sizes, mag_weight, logmag_weight, l2, per_item=False):
        from . import spectra
        ctx.per_item = per_item   # one value per clip (`dims` = the two spectrogram axes) instead of the scalar
        target_audio, audio = target_audio.contiguous(), audio.contiguous()
        total = None
        saved, specs = [], []
        for size in fft_sizes:
            hop = int(size * (1.0 - 0.75))                      # compute_mag's default overlap (features.py:214-216)
            win = spectra._cached_window(None, size, audio.device)   # window=None -> hann (features.py:203-204)
            cplx = None
            if target_audio.shape == audio.shape:
                if ctx.needs_input_grad[1] and spectra.SAVE_SPECTRUM:   # + the estimate's complex spectrum for the backward
                    t, v, cplx = nat.stft_mag_forward_pair(target_audio, audio, win, size, hop, want_spec_b=True)
                else:
                    t, v = nat.stft_mag_forward_pair(target_audio, audio, win, size, hop)   # one launch for both signals
            else:
                t, v = nat.stft_mag_forward(target_audio, win, size, hop), nat.stft_mag_forward(audio, win, size, hop)
            total = nat.spec_distance_forward(t, v, mag_weight, logmag_weight, 1e-5, l2, accumulate_into=total, per_row=per_item)   # total += d
            saved += [t, v]
            specs.append(cplx)
        have = [c is not None for c in specs]
        ctx.save_for_backward(target_audio, audio, *saved, *[c for c in specs if c is not None])
        ctx.cfg = (tuple(fft_sizes), mag_weight, logmag_weight, l2, have)
        return total

    @staticmethod
    def backward(ctx, g):
        from . import spectra
        target_audio, audio, *saved = ctx.saved_tensors
        fft_sizes, mag_weight, logmag_weight, l2, have = ctx.cfg
        cplx_list = saved[2 * len(fft_sizes):]
        cplx_iter = iter(cplx_list)
        cplx = [next(cplx_iter) if h else None for h in have]
        need_t, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = g.float().reshape(-1).contiguous()   # one element, or one per clip
        grad_t = grad_v = None   # the first scale's kernel writes the gradient, the later ones add to it
        for i, size in enumerate(fft_sizes):
            hop = int(size * (1.0 - 0.75))
            win = spectra._cached_window(None, size, audio.device)
            t, v = saved[2 * i], saved[2 * i + 1]
            gt, gv = nat.spec_distance_backward(t, v, mag_weight, logmag_weight, g, 1.0, 1e-5, l2, need_target=need_t, need_value=need_v,
                                                per_row=ctx.per_item)
            if need_v:
                grad_v = nat.stft_mag_backward(audio, win, size, hop, gv, accumulate_into=grad_v, spec=cplx[i])
            if need_t:
                grad_t = nat.stft_mag_backward(target_audio, win, size, hop, gt, accumulate_into=grad_t)
        return grad_t, grad_v, None, None, None, None, None


MSS_FUSED = True   # module switch (tests compare both forms): MSSLoss on the GPU as TWO launches (sot_mss_loss_and_grad) instead of 36


class _MultiScaleSpectralFused(torch.autograd.Function):
    """MSSLoss as one call (include/sot_hip.h: sot_mss_loss_and_grad, csrc/sot_mss.hip): the loss of all scales AND its gradient w.r.t.
    the estimate's audio come out of the forward (no spectrogram is ever stored); the backward multiplies by the upstream gradient.
    Only the estimate is differentiated (trainer.py:206-221: the target is data); a target that asks for a gradient takes
    _MultiScaleSpectral."""

    @staticmethod
    def forward(ctx, target_audio, audio, fft_sizes, mag_weight, logmag_weight, l2, per_item=False):
        from . import spectra
        windows = [spectra._cached_window(None, size, audio.device) for size in fft_sizes]   # window=None -> hann (features.py:203-204)
        want = ctx.needs_input_grad[1]
        loss, grad = nat.mss_loss_and_grad(target_audio, audio, fft_sizes, windows, mag_weight, logmag_weight, 1e-5, l2, per_item, want)
        ctx.per_item = per_item
        if want:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[1]:
            return (None,) * 7
        (grad,) = ctx.saved_tensors
        g = g.float()
        return None, grad * (g.reshape(-1, 1) if ctx.per_item else g), None, None, None, None, None


class MSSLoss(torch.nn.Module):
    """Multi-scale spectrogram loss, the reference's `losses.MSSLoss` (losses.py:365-425): for each FFT
    size the magnitude STFT (hann window, 75 % overlap, end-padded, normalized: features.compute_mag) of target and estimate,
    `mag_weight * mean D(t - v) + logmag_weight * mean D(safe_log t - safe_log v)` with D = |.| ('L1') or (.)^2 ('L2'),
    summed over the sizes.  On the GPU everything runs in HIP kernels behind one autograd node (also with `dims` = the two spectrogram
    axes: one value per clip); any other `dims`, FFT sizes the kernels do not cover and CPU tensors take the same composition on torch ops."""

    def __init__(self, fft_sizes=(2048, 1024, 512, 256, 128, 64), loss_type="L1", mag_weight=0.0, logmag_weight=0.0):
        super().__init__()
        self.fft_sizes = tuple(fft_sizes)
        self.loss_type = loss_type
        self.mag_weight = mag_weight
        self.logmag_weight = logmag_weight

    def forward(self, target_audio, audio, **kwargs):
        from . import spectra
        kind = self.loss_type.upper()
        if kind not in ("L1", "L2"):
            raise ValueError("Loss type ({}), must be " '"L1", "L2" '.format(kind))   # losses.py:36
        dims = kwargs.get("dims", None)
        # `dims` = the two spectrogram axes of [batch, freq, frames] (one value per clip): the per-row distance kernels.  (Any other
        # subset keeps an axis whose length differs from scale to scale -- with more than one FFT size the reference's `loss +=` fails.)
        per_item = (dims is not None and not isinstance(dims, int) and all(isinstance(d, int) and -3 <= d < 3 for d in dims)
                    and sorted(d % 3 for d in dims) == [1, 2])
        native_ok = (audio.is_cuda and target_audio.is_cuda and (dims is None or per_item) and audio.ndim == 2 and audio.shape == target_audio.shape and
                     audio.shape[0] > 0 and (self.mag_weight > 0 or self.logmag_weight > 0) and   # (an empty batch: torch's mean of nothing, NaN)
                     all(spectra.hip_stft_supported(s, int(s * 0.25), audio.shape[1]) for s in self.fft_sizes))
        if audio.is_cuda and not native_ok:
            warn_once(("mss", dims is not None, self.fft_sizes),
                      "MSSLoss: this call runs the torch composition instead of the HIP kernels (`dims` other than the two spectrogram axes, FFT sizes outside "
                      "64..4096, shapes that differ, or both weights zero)")
        if native_ok and MSS_FUSED and len(self.fft_sizes) <= 8 and all(int(s) in nat.MSS_FUSED_SIZES for s in self.fft_sizes) and \
                not (torch.is_grad_enabled() and target_audio.requires_grad):
            sizes = tuple(int(s) for s in self.fft_sizes)
            if _compiling():
                return _o.mss_loss(target_audio.float(), audio.float(), list(sizes), float(self.mag_weight), float(self.logmag_weight), kind == "L2",
                                   per_item, 1.0, torch.is_grad_enabled() and audio.requires_grad)[0]
            # rows the kernels can address: an expanded target (row stride 0) or an overlapping view is copied, as the reference's ops would
            target_audio, audio = nat.rows_view(target_audio), nat.rows_view(audio)
            glue = nat.glue() if (audio.dtype == torch.float32 and target_audio.dtype == torch.float32 and audio.stride(1) == 1 and
                                  target_audio.stride(1) == 1 and audio.shape[0] > 0) else None
            if glue is not None:   # ONE C++ call and a C++ autograd node (csrc/sot_torch_glue.cpp: MssLoss)
                wins = spectra._cached_windows(None, sizes, audio.device)
                return glue.mss_loss(target_audio, audio, wins, list(sizes), float(self.mag_weight), float(self.logmag_weight), kind == "L2", per_item)
            return _MultiScaleSpectralFused.apply(target_audio.float(), audio.float(), sizes, float(self.mag_weight),
                                                  float(self.logmag_weight), kind == "L2", per_item)
        if native_ok and not _compiling():   # (traced: the composition below, whose transforms are the HIP STFT op)
            return _MultiScaleSpectral.apply(target_audio.float(), audio.float(), self.fft_sizes, float(self.mag_weight),
                                             float(self.logmag_weight), kind == "L2", per_item)
        loss = 0.0
        for size in self.fft_sizes:
            hop = int(size * (1.0 - 0.75))
            t = spectra.stft_magnitude(target_audio, size, hop, None).permute(0, 2, 1)   # [batch, freq, frames] as compute_mag
            v = spectra.stft_magnitude(audio, size, hop, None).permute(0, 2, 1)
            for weight, a, b in ((self.mag_weight, t, v), (self.logmag_weight, _safe_log(t), _safe_log(v))):
                if weight > 0:
                    diff = a - b
                    red = list(range(diff.ndim)) if dims is None else dims
                    loss = loss + weight * (torch.mean(torch.abs(diff), dim=red) if kind == "L1" else torch.mean(diff ** 2, dim=red))
        return loss


def _safe_log(x, eps=1e-5):
    """utils.py:145-151."""
    e = torch.tensor(eps, device=x.device)
    return torch.log(torch.where(x <= e, e, x))


class Wasserstein1DWithTransform(torch.nn.Module):
    """The reference's audio-in form (losses.py:316-343): both signals go through the transform that
    ``features.get_transform(transform_kwargs, sample_rate)`` names, the transform's bin frequencies scaled to [0, 1]
    become the positions of both sides, and ``Wasserstein1D`` (attribute ``wasserstein``) compares the spectra.
    Built here for the STFT transform (``{"type": "stft", "n_fft", "hop_length", "window", "log", "sr"}``, the reference's
    ``features.TorchSTFT``, features.py:85-113: hann window unless a scipy window name is given; defaults n_fft 1024, hop
    256, sr 16000).  ``"cqt"`` (nnAudio) and ``"identity"`` (no bin frequencies in the reference either) raise.
    On the GPU the STFT, the loss and their backward are the HIP kernels of spectra.training_step_slice."""

    def __init__(self, p=1, fixed_x=None, require_sort=True, log_scaled_x=False, transform_kwargs=None, **kwargs):
        super().__init__()
        self.wasserstein = Wasserstein1D(p=p, fixed_x=fixed_x, require_sort=require_sort, log_scaled_x=log_scaled_x, **kwargs)
        if not isinstance(transform_kwargs, dict):
            raise AttributeError("transform_kwargs must be a dict (the reference pops 'sr' from it)")
        tk = dict(transform_kwargs)
        self.sr = tk.pop("sr", 16000)
        name = tk.pop("type")
        if name != "stft":
            raise ValueError(f"Unknown transform {name}" if name not in ("cqt", "identity") else
                             f"transform {name!r} is not built here (only 'stft')")
        self.n_fft = int(tk.pop("n_fft", 1024))
        hop_length = tk.pop("hop_length", 256)
        self.log = bool(tk.pop("log", False))
        self.window = tk.pop("window", None)
        overlap = 1 - hop_length / self.n_fft                 # features.py:99, then features.py:194
        self.hop = int(self.n_fft * (1.0 - overlap))
        assert self.n_fft * overlap % 2.0 == 0.0              # features.py:199

    def forward(self, x, y, **kwargs):
        from . import spectra
        if not self.log and not kwargs:
            return spectra.training_step_slice(self.wasserstein, x, y, n_fft=self.n_fft, hop=self.hop, sample_rate=float(self.sr),
                                               window=self.window)
        spec_x = spectra.stft_magnitude(x, self.n_fft, self.hop, self.window)
        spec_y = spectra.stft_magnitude(y, self.n_fft, self.hop, self.window)
        if self.log:
            spec_x, spec_y = _safe_log(spec_x), _safe_log(spec_y)
        if _compiling() and x.is_cuda:
            pos = _o.unit_frequencies(x.detach(), self.n_fft, float(self.sr))
        else:
            pos = spectra.unit_frequencies(self.n_fft, float(self.sr), x.device)
        return self.wasserstein(spec_x, spec_y, x_pos=pos, y_pos=pos.clone(), **kwargs)


class MixOfLosses(torch.nn.Module):
    """losses.py:346-362: weighted dict of losses keyed by class name."""

    def __init__(self, losses, weights=None):
        super().__init__()
        self.losses = losses
        self.weights = weights

    def forward(self, x, y, **kwargs):
        loss = {}
        for loss_fn, weight in zip(self.losses, self.weights):
            loss_ = loss_fn(x, y, **kwargs) * weight
            loss[loss_fn.__class__.__name__] = loss_
        return loss


# ---- the other operands a MixOfLosses configuration of the reference may name (losses.py:7-86).  Not on the OT path and not HIP: plain
# ---- torch-op compositions with the reference's call signature, so that a configuration that mixes them with Wasserstein1D loads.

def mean_difference(target, value, loss_type="L1", weights=None, dims=None):
    """losses.py:7-36: mean over `dims` (all axes when None) of |d·w| ("L1") or d²·w ("L2"), d = target − value."""
    kind = loss_type.upper()
    if kind not in ("L1", "L2"):
        raise ValueError('Loss type ({}), must be "L1", "L2" '.format(kind))
    delta = target - value
    w = 1.0 if weights is None else weights
    term = (delta * w).abs() if kind == "L1" else delta ** 2 * w
    return torch.mean(term, dim=list(range(term.ndim)) if dims is None else dims)


class MeanDifference(torch.nn.Module):
    """losses.py:39-54: mean_difference of the two inputs, optionally after sorting each along its last axis."""

    def __init__(self, loss_type="L1"):
        super().__init__()
        self.loss_type = loss_type

    def forward(self, x, y, weights=None, sort=False, **kwargs):
        if sort:
            x, y = torch.sort(x, dim=-1)[0], torch.sort(y, dim=-1)[0]
        return mean_difference(x, y, loss_type=self.loss_type, weights=weights, dims=kwargs.get("dims", None))


class KL(torch.nn.Module):
    """losses.py:57-86: rows normalised to unit mass (safe_divide), KL(input ‖ target) = Σ a·(log(a + eps) − log(b + eps)) per row
    (`reverse` swaps the roles), mean over `dims`."""

    def __init__(self, eps=1e-10, **kwargs):
        super().__init__()
        self.eps = eps
        self.reverse = kwargs.get("reverse", False)

    def forward(self, input, target, **kwargs):
        lead = input.shape[:-1]
        rows = lambda t: t.reshape(-1, t.shape[-1]) if t.ndim == 3 else t   # noqa: E731
        a, b = rows(input), rows(target)
        if self.reverse:
            a, b = b, a
        a = safe_divide(a, a.sum(dim=-1, keepdim=True))
        b = safe_divide(b, b.sum(dim=-1, keepdim=True))
        per_row = (a * (torch.log(a + self.eps) - torch.log(b + self.eps))).sum(dim=-1)
        return torch.mean(per_row.reshape(lead), dim=kwargs.get("dims", None))
