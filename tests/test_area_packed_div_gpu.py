"""-m gpu: the plain row loop of the merge-free p = 1 kernel at 2048 bins (sot_area_full_kernel<256, 8, 1>) after its VALU diet: the division by
the row mass on pairs of adjacent elements, the cheap operand screen in front of the exact one, the differences of the area term on pairs.

Every row is pinned bit for bit to the build BEFORE those changes (tests/golden/area_valu_diet.npz, written by tools/make_golden_area_diet.py on
that build's library) and must equal the general loop (fused_mean=True hands the kernel its completion counters, which selects the loop that
keeps the scalar division and the per-element screen) on the same inputs.

The rows aim at both halves of a packed pair and at the IEEE fallback, which a wave takes when one of its operands is non-zero and at most
2^-78 or a row mass is above 2^40.  A thread owns 8 adjacent elements, a wave 512: wave 2 holds elements 1024 ... 1535.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import device, native

pytestmark = pytest.mark.gpu

N = 2048
P1_FLAGS = 8   # require_sort; normalised, no square_dist: the reference's p = 1 call
KINDS = ("tiny_even", "tiny_odd", "denormal", "zeros_even", "zeros_odd", "mass_2p42", "mass_below_guard", "all_zero", "single_bin")
# (B, first kind, side that carries the stress rows): B = 1, 3 and 9 rows, every kind at least once on either side
SMALL_CASES = [(1, 0, "x"), (1, 1, "x"), (3, 2, "x"), (3, 5, "x"), (9, 0, "x"),
               (1, 0, "y"), (1, 1, "y"), (3, 2, "y"), (3, 5, "y"), (9, 0, "y")]
BIG_B = 1025   # a full grid of 1024 workgroups, and workgroup 0 takes a second row


def base_rows(B, seed):
    """Ordinary rows: weights in [0.05, 1), far above the screen's bound."""
    return (0.05 + 0.95 * np.random.RandomState(seed).random_sample((B, N))).astype(np.float32)


def stress_row(kind, base):
    w = base.copy()
    if kind == "tiny_even":
        w[1200] = np.float32(2.0 ** -80)          # below 2^-78, even element, inside wave 2 only: that wave alone takes the fallback
    elif kind == "tiny_odd":
        w[1201] = np.float32(2.0 ** -80)          # the other half of a pair
    elif kind == "denormal":
        w[1301] = np.float32(2.0 ** -130)
    elif kind == "zeros_even":
        w[0::2] = 0.0                             # exact zeros stay on the fast path: the cheap screen fires, the exact one does not
    elif kind == "zeros_odd":
        w[1::2] = 0.0
    elif kind == "mass_2p42":
        w[:] = np.float32(2.0 ** 31)              # row mass 2^42 > 2^40: every wave takes the fallback
    elif kind == "mass_below_guard":
        w[:] = np.float32(2.0 ** -40)             # row mass 2^-29 < 1e-7: the guard replaces it
    elif kind == "all_zero":
        w[:] = 0.0
    elif kind == "single_bin":
        w[:] = 0.0
        w[(7 * N) // 11] = 0.75
    else:
        raise ValueError(kind)
    return w


def small_inputs(B, first, side):
    """B rows: kinds first ... first + B - 1 on `side`, ordinary rows on the other side."""
    plain, other = base_rows(B, 100 + 10 * first + B), base_rows(B, 200 + 10 * first + B)
    stressed = np.stack([stress_row(KINDS[first + i], plain[i]) for i in range(B)])
    return (stressed, other) if side == "x" else (other, stressed)


def big_inputs():
    """1025 ordinary rows with the x-side stress rows in rows 0 ... 8 (first rows of their workgroups) and the y-side ones in rows 1016 ... 1024
    (row 1024 is workgroup 0's second row)."""
    x, y = base_rows(BIG_B, 31), base_rows(BIG_B, 32)
    for i, kind in enumerate(KINDS):
        x[i] = stress_row(kind, x[i])
        y[BIG_B - len(KINDS) + i] = stress_row(kind, y[BIG_B - len(KINDS) + i])
    x[BIG_B - 1] = stress_row("tiny_odd", x[BIG_B - 1])   # the second row of a workgroup takes the fallback too
    return x, y


@functools.lru_cache(maxsize=None)
def grid():
    nat = native()
    pos = torch.linspace(0, 1, N).to(device())
    pos2 = pos.clone()
    plan = nat.PositionPlan(pos, pos2)
    assert plan.same_grid()
    return pos, pos2, plan


def run(nat, x, y, fused_mean):
    pos, pos2, plan = grid()
    xd, yd = torch.from_numpy(x).to(device()), torch.from_numpy(y).to(device())
    mean, rows, _ = nat.loss_fused(xd, yd, pos, pos2, 1.0, P1_FLAGS, plan, fused_mean=fused_mean)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), mean.cpu().numpy().reshape(1)


def key(B, first, side):
    return f"b{B}_k{first}_{side}"


def golden_outputs(nat):
    """What tools/make_golden_area_diet.py stores: row losses and mean of the plain loop for every small case."""
    out = {}
    for B, first, side in SMALL_CASES:
        rows, mean = run(nat, *small_inputs(B, first, side), fused_mean=False)
        out[key(B, first, side) + "_rows"] = rows
        out[key(B, first, side) + "_mean"] = mean
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("B,first,side", SMALL_CASES)
def test_rows_unchanged_against_the_build_before(B, first, side):
    want = np.load(os.path.join(GOLDEN, "area_valu_diet.npz"))
    rows, mean = run(native(), *small_inputs(B, first, side), fused_mean=False)
    assert np.isfinite(rows).all()
    assert same_bits(rows, want[key(B, first, side) + "_rows"]), (rows, want[key(B, first, side) + "_rows"])
    assert same_bits(mean, want[key(B, first, side) + "_mean"]), (mean, want[key(B, first, side) + "_mean"])


@pytest.mark.parametrize("B,first,side", SMALL_CASES)
def test_plain_loop_equals_general_loop(B, first, side):
    nat = native()
    x, y = small_inputs(B, first, side)
    rows, mean = run(nat, x, y, fused_mean=False)
    rows_g, mean_g = run(nat, x, y, fused_mean=True)
    assert same_bits(rows, rows_g), (rows, rows_g)
    assert same_bits(mean, mean_g)


def test_plain_loop_equals_general_loop_on_a_full_grid_plus_one_row():
    nat = native()
    x, y = big_inputs()
    rows, mean = run(nat, x, y, fused_mean=False)
    rows_g, mean_g = run(nat, x, y, fused_mean=True)
    assert np.isfinite(rows).all()
    bad = np.flatnonzero(rows.view(np.uint32) != rows_g.view(np.uint32))
    assert bad.size == 0, (bad[:8], rows[bad[:8]], rows_g[bad[:8]])
    assert same_bits(mean, mean_g)
    # a row's loss does not depend on its place in the batch: the stress rows again, each as a batch of its own kind's small case
    k = len(KINDS)
    rows_x, _ = run(nat, x[:k], y[:k], fused_mean=False)
    rows_y, _ = run(nat, x[BIG_B - k:], y[BIG_B - k:], fused_mean=False)
    assert same_bits(rows_x, rows[:k]) and same_bits(rows_y, rows[BIG_B - k:])
