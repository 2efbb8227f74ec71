"""Mixed supports (a shared 1-D grid on one side, per-row positions on the other): what can be checked without a GPU -- the ABI
constants, the four entry points in header, binding and library, the routing predicate on the edges of its domain, and the host logic
of the module on CPU tensors.  The kernels themselves: tests/test_mixed_supports_gpu.py."""
import ctypes
import os
import re

import torch

from conftest import ROOT

MIXED_SYMBOLS = ("sot_w1d_mixed_forward", "sot_w1d_mixed_backward", "sot_w1d_mixed_position_grad", "sot_w1d_mixed_workspace_bytes")


def _header():
    with open(os.path.join(ROOT, "include", "sot_hip.h")) as f:
        return f.read()


def test_abi_version_in_header_library_and_binding():
    from sot_amd import _native as nat
    version = int(re.search(r"#define SOT_ABI_VERSION (\d+)", _header()).group(1))
    assert version == nat.ABI_VERSION >= 17
    handle = ctypes.CDLL(nat.library_path())
    handle.sot_abi_version.restype = ctypes.c_int
    assert handle.sot_abi_version() == version


def test_entry_points_are_declared_bound_and_exported():
    from sot_amd import _native as nat
    header = _header()
    handle = ctypes.CDLL(nat.library_path())
    for name in MIXED_SYMBOLS:
        assert re.search(r"\b(int|size_t) %s\(const sot_problem \*prob" % name, header), name
        assert name in nat.EXPORTS
        getattr(handle, name)
    assert nat.EXPORTS["sot_w1d_mixed_workspace_bytes"][0] is ctypes.c_size_t


def test_c_entry_points_refuse_bad_problems_on_the_host():
    """Validation happens before any pointer is followed, so it runs without a GPU: the pointers below are never dereferenced."""
    from sot_amd import _native as nat
    lib = nat.load(build_if_missing=False)

    def problem(n, m, xps, yps, p=1.0, fake=0x1000):
        pr = nat.SotProblem()
        pr.x = pr.y = pr.xpos = pr.ypos = fake
        pr.B, pr.n, pr.m = 4, n, m
        pr.x_row_stride, pr.y_row_stride, pr.xpos_row_stride, pr.ypos_row_stride = n, m, xps, yps
        pr.p, pr.flags = p, nat.FLAG_REQUIRE_SORT
        return pr

    def forward(pr):
        return lib.sot_w1d_mixed_forward(ctypes.byref(pr), 0x1000, None, 0, None)

    assert lib.sot_w1d_mixed_forward(None, 0x1000, None, 0, None) == nat.SOT_ERR_NULL_POINTER
    assert forward(problem(1025, 8, 0, 0)) == nat.SOT_ERR_BAD_SHAPE            # both shared
    assert forward(problem(1025, 8, 1025, 8)) == nat.SOT_ERR_BAD_SHAPE         # both per row
    assert forward(problem(1025, 8, 0, 7)) == nat.SOT_ERR_BAD_SHAPE            # per-row stride shorter than the row
    assert forward(problem(1025, 8, 0, 8, p=0.5)) == nat.SOT_ERR_INVALID_P
    assert forward(problem(1025, 2049, 0, 2049)) == nat.SOT_ERR_UNSUPPORTED_SIZE
    assert forward(problem(2049, 8, 2049, 0)) == nat.SOT_ERR_UNSUPPORTED_SIZE
    assert forward(problem(16384, 2048, 0, 2048)) == nat.SOT_ERR_UNSUPPORTED_SIZE   # past the LDS budget
    assert forward(problem(1025, 8, 0, 8, fake=None)) == nat.SOT_ERR_NULL_POINTER
    assert forward(problem(1025, 2048, 0, 2048)) == nat.SOT_ERR_NULL_POINTER       # in the domain: the missing workspace is what is refused
    # the workspace: needed when the call has to plan the shared row itself, sized for that row; 0 for a refused problem
    assert lib.sot_w1d_mixed_workspace_bytes(ctypes.byref(problem(1025, 8, 0, 8))) >= 2 * 4 * 1025
    assert lib.sot_w1d_mixed_workspace_bytes(ctypes.byref(problem(1025, 8, 0, 0))) == 0
    unsorted_ok = problem(1025, 8, 0, 8)
    unsorted_ok.flags = 0
    assert lib.sot_w1d_mixed_workspace_bytes(ctypes.byref(unsorted_ok)) == 0
    # every size the Python predicate lets through is inside the C domain (the predicate is the narrower of the two)
    for n, m in ((8192, 2048), (2048, 8192), (4097, 2048), (1, 1), (2048, 2048)):
        pr = problem(n, m, 0, m) if m <= 2048 else problem(n, m, n, 0)
        pr.flags = 0
        pr.B = 0
        assert forward(pr) == nat.SOT_OK, (n, m)


def test_routing_predicate_on_the_edges_of_its_domain():
    from sot_amd import losses
    B, n = 3, 1025
    x = torch.rand(B, n)
    grid = torch.linspace(0, 1, n)

    def applies(k, xpos=None, ypos=None, **kw):
        y = torch.rand(B, k)
        return losses.mixed_route_applies(x, y, grid if xpos is None else xpos, torch.rand(B, k) if ypos is None else ypos, **kw)

    assert applies(8) and applies(1) and applies(2048)
    assert not applies(2049)                                                        # per-row side past the limit
    assert not applies(8, ypos=torch.rand(8))                                       # both sides shared
    assert not applies(8, xpos=torch.rand(B, n))                                    # both sides per row
    assert applies(8, xpos=grid.unsqueeze(0).expand(B, n))                          # a stride-0 expansion is a shared row
    assert not applies(8, xpos=grid.unsqueeze(0).expand(B, n).contiguous())         # its copy is not
    assert not applies(8, return_quantiles=True)
    assert not applies(8, xpos=grid.clone().requires_grad_(True))                   # a shared grid that needs a gradient
    with torch.no_grad():
        assert applies(8, xpos=grid.clone().requires_grad_(True))                   # ... but not where nobody can ask for it
    assert applies(8, ypos=torch.rand(B, 8).requires_grad_(True))                   # the per-row side may
    # either side may be the per-row one; 3-D [batch, time, K] positions; the LDS budget (pow2(n) + pow2(m) <= 12000)
    assert losses.mixed_route_applies(torch.rand(B, 8), x, torch.rand(B, 8), grid)
    assert not losses.mixed_route_applies(torch.rand(B, 2049), x, torch.rand(B, 2049), grid)
    assert losses.mixed_route_applies(x.reshape(1, B, n), torch.rand(1, B, 8), grid, torch.rand(1, B, 8))
    assert losses.mixed_route_applies(x.reshape(1, B, n), torch.rand(1, B, 8), grid.expand(1, B, n), torch.rand(1, B, 8))
    assert losses.mixed_route_applies(torch.rand(B, 8192), torch.rand(B, 2048), torch.rand(8192), torch.rand(B, 2048))
    assert not losses.mixed_route_applies(torch.rand(B, 8193), torch.rand(B, 2048), torch.rand(8193), torch.rand(B, 2048))
    # the switch restores the materialising route everywhere
    losses.MIXED_ROUTE = False
    try:
        assert not applies(8)
    finally:
        losses.MIXED_ROUTE = True
    assert applies(8)


def test_cpu_module_gives_the_same_rows_for_a_grid_and_its_expansion():
    """CPU tensors take the torch-op composition whatever the switch says: a 1-D grid and its explicit per-row copy are the same rows, for
    either orientation, on the module and on the functional form."""
    from sot_amd.losses import Wasserstein1D, wasserstein_1d
    gen = torch.Generator().manual_seed(3)
    B, n, K = 4, 65, 5
    x, y = torch.rand(B, n, generator=gen), torch.rand(B, K, generator=gen)
    grid = torch.rand(n, generator=gen)                      # unsorted
    rowpos = torch.rand(B, K, generator=gen) * 1.4 - 0.2    # partly outside the grid's range
    for ctor in (dict(p=1), dict(p=2, square_dist=True, dont_normalize=True, limit_quantile_range=True)):
        mod = Wasserstein1D(**ctor)
        want = mod.row_losses(x, y, x_pos=grid.unsqueeze(0).expand(B, n).contiguous(), y_pos=rowpos)
        assert torch.equal(mod.row_losses(x, y, x_pos=grid, y_pos=rowpos), want)
        swapped = mod.row_losses(y, x, x_pos=rowpos, y_pos=grid)
        assert torch.equal(swapped, mod.row_losses(y, x, x_pos=rowpos, y_pos=grid.unsqueeze(0).expand(B, n).contiguous()))
        assert torch.allclose(mod(x, y, x_pos=grid, y_pos=rowpos), want.mean())
    xw, yw = x / x.sum(1, keepdim=True), y / y.sum(1, keepdim=True)
    assert torch.equal(wasserstein_1d(grid.unsqueeze(0).expand(B, n), rowpos, xw, yw, p=2),
                       wasserstein_1d(grid.unsqueeze(0).expand(B, n).contiguous(), rowpos, xw, yw, p=2))
