"""-m gpu: the two row loops of the merge-free p = 1 kernel (sot_area_full_kernel) and the wave-total prefix of the shared CDF builder.

On 2048-bin rows the plain launch (identity permutations, normalised rows, row losses wanted, no mean tail) takes a loop compiled for it,
with one workgroup barrier less per row and the row loss stored one row late; every other launch takes the general loop.  Both must give the same
bits.  fused_mean=True hands the kernel its completion counters, which selects the general loop on the same inputs.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import device, native

pytestmark = pytest.mark.gpu

# (N, B): 2048 bins -- the geometry that carries the plain loop (kAreaPlainLoop) -- with grids smaller than the chip (1, 3), full (1024) and
# with one row more for some workgroups (1025, 2051); the other geometries keep one loop, so both calls must agree there all the more:
# 1024 bins (two rows per workgroup), 512 bins (four one-wave rows per workgroup: no workgroup barrier), 1025 bins, run-time length 2000
SHAPES = [(2048, 1), (2048, 3), (2048, 1024), (2048, 1025), (2048, 2051), (1024, 5), (512, 7), (1025, 9), (2000, 9)]
KINDS = ["uniform", "peaky"]
P1_FLAGS = 8   # require_sort; normalised, no square_dist: the reference's p = 1 call


@functools.lru_cache(maxsize=None)
def case(N, B, kind):
    """Inputs of one shape on the device (computed once, never modified): a row of zeros and a row with a single non-zero bin included
    where the batch has room for them; the grid, its plan and the row losses of the default call (the plain loop)."""
    from sot_amd.bench_inputs import spectrum_pairs
    nat = native()
    x, y = spectrum_pairs(kind, B, N, N, 1000 + N + B)
    if B >= 3:
        x[B - 1] = 0.0                               # all zeros (mass guard)
        y[B - 2] = 0.0
        y[B - 2, (7 * N) // 11] = 0.75               # a single non-zero bin
    xd, yd = x.to(device()), y.to(device())
    pos = torch.linspace(0, 1, N).to(device())
    pos2 = pos.clone()
    plan = nat.PositionPlan(pos, pos2)
    assert plan.same_grid()
    mean, rows, _ = nat.loss_fused(xd, yd, pos, pos2, 1.0, P1_FLAGS, plan, fused_mean=False)
    torch.cuda.synchronize()
    return xd, yd, pos, pos2, plan, rows, mean


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,B", SHAPES)
def test_plain_loop_equals_general_loop_bit_for_bit(N, B, kind):
    nat = native()
    xd, yd, pos, pos2, plan, rows, mean = case(N, B, kind)
    mean_g, rows_g, _ = nat.loss_fused(xd, yd, pos, pos2, 1.0, P1_FLAGS, plan, fused_mean=True)
    assert torch.isfinite(rows).all()
    assert torch.equal(rows, rows_g), float((rows - rows_g).abs().max())
    assert torch.equal(mean, mean_g)
    assert torch.equal(nat.forward_rows(xd, yd, pos, pos2, 1.0, P1_FLAGS, plan), rows)   # the forward alone: the plain loop again


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,B", SHAPES)
def test_plain_loop_against_merge_kernel(N, B, kind):
    """Per row against the merge kernel (FLAG_NO_AREA), at the tolerance of tests/test_gpu_parity.py for this pair."""
    nat = native()
    xd, yd, pos, pos2, plan, rows, _ = case(N, B, kind)
    area = rows.cpu().numpy().astype(np.float64)
    merge = nat.forward_rows(xd, yd, pos, pos2, 1.0, P1_FLAGS | nat.FLAG_NO_AREA, plan).cpu().numpy().astype(np.float64)
    bound = 2e-6 * np.maximum(np.abs(merge), 1e-12) + 1e-12
    assert np.all(np.abs(area - merge) <= bound), float(np.max(np.abs(area - merge) / np.maximum(np.abs(merge), 1e-12)))


@pytest.mark.parametrize("N,B,slices", [(2048, 2051, [(0, 1), (5, 3), (1000, 1025), (2050, 1)]), (1024, 5, [(1, 3), (4, 1)]), (512, 7, [(2, 5), (6, 1)]),
                                        (1025, 9, [(3, 4)]), (2000, 9, [(1, 7)])])
def test_plain_loop_on_slices_of_the_batch(N, B, slices):
    """A row's loss does not depend on which workgroup takes it, on the rows next to it or on its place in the workgroup's sequence."""
    nat = native()
    xd, yd, pos, pos2, plan, rows, _ = case(N, B, "peaky")
    for i, k in slices:
        part = nat.forward_rows(xd[i:i + k], yd[i:i + k], pos, pos2, 1.0, P1_FLAGS, plan)
        assert torch.equal(part, rows[i:i + k]), (i, k, float((part - rows[i:i + k]).abs().max()))


PAPER_FLAGS = 1 | 2 | 4 | 8   # square_dist, dont_normalize, limit_quantile_range, require_sort; p = 2
PREFIX_SHAPES = (2048, 1025)
PREFIX_ROWS = 16
PREFIX_GRAD_COLS = 64


def shared_prefix_outputs(nat, N):
    """Paper-mode outputs of the kernels that share the CDF builder with the merge-free kernel (tools/make_golden_prefix.py stores them)."""
    from sot_amd.bench_inputs import spectrum_pairs
    x, y = spectrum_pairs("peaky", PREFIX_ROWS, N, N, 4000 + N)
    xd, yd = x.to(device()), y.to(device())
    if N % 2:
        pos = torch.fft.rfftfreq(2 * (N - 1), 1 / 16000.0)
        pos = (pos / pos.max()).float().to(device())
    else:
        pos = torch.linspace(0, 1, N).to(device())
    pos2 = pos.clone()
    plan = nat.PositionPlan(pos, pos2)
    fwd = nat.forward_rows(xd, yd, pos, pos2, 2.0, PAPER_FLAGS, plan)
    mean, rows, gy = nat.loss_and_grad(xd, yd, pos, pos2, 2.0, PAPER_FLAGS, plan)
    return {f"n{N}_forward_rows": fwd.cpu().numpy(), f"n{N}_lg_mean": mean.cpu().numpy().reshape(1), f"n{N}_lg_rows": rows.cpu().numpy(),
            f"n{N}_lg_grad": gy[:, :PREFIX_GRAD_COLS].contiguous().cpu().numpy()}


@pytest.mark.parametrize("N", PREFIX_SHAPES)
def test_shared_cdf_builder_outputs_unchanged(N):
    """forward_rows and loss_and_grad in paper mode (merge forward, training form) against the arrays the build before the loop-free
    wave-total prefix produced: bit for bit."""
    want = np.load(os.path.join(GOLDEN, "area_fast_loop_prefix.npz"))
    got = shared_prefix_outputs(native(), N)
    for key, val in got.items():
        assert val.dtype == want[key].dtype and val.shape == want[key].shape, key
        assert np.array_equal(val.view(np.uint32), want[key].view(np.uint32)), (key, float(np.abs(val - want[key]).max()))
