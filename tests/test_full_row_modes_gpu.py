"""-m gpu: every cost / cutoff / square_dist mode through every mode switch of the full-row kernels.

The full-row dispatch functions (csrc/sot_full_fwd.hpp, csrc/sot_full_bwd.hpp) map (p, LIMIT_Q, SQUARE) to the template arguments
<PM, LIM, SQ> through ONE function, with_mode (csrc/sot_launch.hpp).  This test runs all 12 modes -- p in {1, 2, 3} x cutoff on / off x
square_dist on / off -- through each of the eight routes that use it, at the smallest shape that reaches the route, and compares with the
oracle on every row (8192 x 129: the first and the last 64 rows) and with the generic kernel (SOT_FLAG_NO_SPECIALIZE) on all rows.

DONT_NORMALIZE is always set and y is scaled by 2: the quantile cutoff only bites where y's mass exceeds x's, so without this a kernel
with LIM swapped for !LIM would return the same numbers.  That the inputs do tell the 12 modes apart is asserted, on the oracle's
values: on EVERY row of the small shapes the row losses of any two modes differ by >= 1e-3 relative, a hundred times the tolerance of
the comparison (measured on the CPU for these inputs: >= 1.59e-3 at 5 x 200, 5.7e-3 at 3 x 1024, 1.6e-2 at 3 x 512 with per-row
positions, 2.4e-2 at 5 x 512).  8192 x 129 cannot meet that on every row: among 8192 rows of 129 peaky weights 173 have a y whose mass
does not exceed x's even when doubled (cutoff on and off are then the same function: separation exactly 0), or two modes' losses
meet by chance; of the 128 checked rows these are row 6 (cutoff pairs, 0) and row 56 (p = 2 cutoff against p = 3 cutoff + square:
3.3e-4).  For that shape the assertion is what the comparison needs: every other mode differs by >= 1e-3 on at least one checked row
(measured: on at least 127 of the 128).

Tolerances are those of the tests of the same routes in test_gpu_parity.py: 1e-5 relative to the oracle (forward), 1e-5 of the row's
largest gradient entry (backward); against the generic kernel bit for bit on the compile-time routes of rows that fill their geometry
with p in {1, 2} (test_full_row_kernel_matches_generic, test_full_row_backward_matches_generic_and_oracle), 2e-6 elsewhere.

These shapes stay in a workgroup's first row: its second and later rows are tested in tests/test_row_loop_gpu.py, where a new row kernel adds a
line to CASES.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from gpu_util import device, native

pytestmark = pytest.mark.gpu
RTOL = 1e-5
MODES = list(itertools.product((1.0, 2.0, 3.0), (False, True), (False, True)))   # (p, LIMIT_Q, SQUARE)

# route -> (B, N, per-row positions, backward, need_gx, bit-equal to the generic kernel for p in {1, 2})
ROUTES = {
    "fwd": (5, 512, False, False, True, True),            # compile-time forward
    "fwd_rt": (5, 200, False, False, True, False),        # run-time-length forward
    "fwd_half": (8192, 129, False, False, True, False),   # half-wave forward (from 8192 rows of 129 bins)
    "fwd_rowpos": (3, 512, True, False, True, True),      # per-row-position forward
    "bwd": (5, 512, False, True, True, True),             # both-gradient backward
    "bwd_y_slim": (3, 1024, False, True, False, True),    # y-only backward in the layout without U gradient slots
    "bwd_rt": (5, 200, False, True, True, False),         # run-time-length backward
    "bwd_rowpos": (3, 512, True, True, True, True),       # per-row-position backward
}


def mode_flags(lim, sq):
    """oracle flags of one mode (DONT_NORMALIZE always)"""
    return 2 | (4 if lim else 0) | (1 if sq else 0)


@functools.lru_cache(maxsize=None)
def inputs(B, N, rowpos):
    """The inputs of one shape, and the oracle's row losses of all 12 modes on the rows the tests check: computed once, never written to."""
    from oracle import sot_oracle as so
    from oracle.inputs import gen_inputs
    x, y = gen_inputs("peaky", B, N, N, 4321 + N)
    y = y * 2.0
    lin = torch.linspace(0, 1, N)
    if rowpos:   # a copy of the grid per row, perturbed by up to two cells: unsorted, and another order on every row
        g = torch.Generator().manual_seed(N)
        xpos = lin + (torch.rand(B, N, generator=g) - 0.5) * (4.0 / N)
        ypos = lin + (torch.rand(B, N, generator=g) - 0.5) * (4.0 / N)
    else:
        xpos = ypos = lin
    rows = np.arange(B) if B <= 128 else np.concatenate((np.arange(64), np.arange(B - 64, B)))
    xc, yc = x.numpy()[rows], y.numpy()[rows]
    xpc, ypc = (xpos.numpy()[rows], ypos.numpy()[rows]) if rowpos else (xpos.numpy(), ypos.numpy())
    sort = 8 if rowpos else 0
    losses = {(p, lim, sq): so.forward(xc, yc, xpc, ypc, p=p, flags=mode_flags(lim, sq) | sort) for p, lim, sq in MODES}
    return x, y, xpos, ypos, rows, (xc, yc, xpc, ypc), losses


@pytest.mark.parametrize("p,lim,sq", MODES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_mode_through_every_full_row_switch(route, p, lim, sq):
    from oracle import sot_oracle as so
    nat = native()
    dev = device()
    B, N, rowpos, backward, need_gx, fill = ROUTES[route]
    x, y, xpos, ypos, rows, (xc, yc, xpc, ypc), losses = inputs(B, N, rowpos)

    # the inputs tell the modes apart: a kernel of another mode cannot pass the comparisons below
    mine = losses[(p, lim, sq)].astype(np.float64)
    for other, vals in losses.items():
        if other != (p, lim, sq):
            vals = vals.astype(np.float64)
            sep = np.abs(mine - vals) / np.maximum(np.abs(mine), np.abs(vals))
            assert (sep.min() if B <= 128 else sep.max()) >= 1e-3, (other, float(sep.min()), float(sep.max()))

    oflags = mode_flags(lim, sq) | (8 if rowpos else 0)
    flags = oflags | (nat.FLAG_NO_AREA if p == 1.0 else 0)   # p = 1: the merge kernel, not the merge-free one
    xd, yd, xpd, ypd = x.to(dev), y.to(dev), xpos.to(dev), ypos.to(dev)
    if not rowpos:
        ypd = xpd.clone()
    exact = fill and p in (1.0, 2.0)
    if not backward:
        spec = nat.forward_rows(xd, yd, xpd, ypd, p, flags)
        gen = nat.forward_rows(xd, yd, xpd, ypd, p, flags | nat.FLAG_NO_SPECIALIZE)
        print(route, (p, lim, sq), "oracle rel", float(np.max(np.abs(spec.cpu().numpy()[rows] - losses[(p, lim, sq)]) / np.abs(losses[(p, lim, sq)]))),
              "generic rel", float(((spec - gen).abs() / gen.abs()).max()))
        if exact:
            assert torch.equal(spec, gen), float((spec - gen).abs().max())
        else:
            torch.testing.assert_close(spec, gen, rtol=2e-6, atol=1e-12)
        np.testing.assert_allclose(spec.cpu().numpy()[rows], losses[(p, lim, sq)], rtol=RTOL)
        return
    g = torch.linspace(0.5, 1.5, B)
    sx, sy = nat.backward_rows(xd, yd, xpd, ypd, p, flags, g.to(dev), need_gx=need_gx, grad_scale=0.25)
    gx, gy = nat.backward_rows(xd, yd, xpd, ypd, p, flags | nat.FLAG_NO_SPECIALIZE, g.to(dev), grad_scale=0.25)
    wx, wy = so.backward(xc, yc, xpc, ypc, (0.25 * g).numpy()[rows], p=p, flags=oflags)
    assert (sx is None) == (not need_gx)
    for name, got, ref, want in (("gx", sx, gx, wx), ("gy", sy, gy, wy)):
        if got is None:
            continue
        scale = ref.abs().amax(dim=1, keepdim=True) + 1e-30
        wscale = np.abs(want).max(axis=1, keepdims=True) + 1e-30
        print(route, (p, lim, sq), name, "oracle", float(np.max(np.abs(got.cpu().numpy()[rows] - want) / wscale)),
              "generic", float(((got - ref).abs() / scale).max()))
        if exact:
            assert torch.equal(got, ref), float((got - ref).abs().max())
        else:
            assert float(((got - ref).abs() / scale).max()) <= 2e-6
        assert np.max(np.abs(got.cpu().numpy()[rows] - want) / wscale) <= 1e-5
