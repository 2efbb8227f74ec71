"""CPU: the workspace size functions of include/sot_hip.h (host arithmetic, no GPU) and the coverage of tests/test_memory_contract_gpu.py.

sot_workspace_bytes reports room for the per-row pre-sort's permutation image exactly where the pre-sort runs (csrc/sot_launch.hpp:
rowpos_presort_runs, shared with setup_launch; ABI 18) -- before, every per-row problem with SOT_FLAG_REQUIRE_SORT was told to allocate
B (n + m) 2 bytes, 128 MB for 4096 x 8192-point rows, that no kernel read.  Every size function returns 0 for what its header comment says
it refuses.  The memory-contract table has a line for every exported function that enqueues work."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

RS, NS = 8, 32    # SOT_FLAG_REQUIRE_SORT, SOT_FLAG_NO_SPECIALIZE


def _up(v, a=256):
    return (v + a - 1) // a * a


def _problem(nat, B, n, m, flags, rowpos, perm_in=0, perm_out=0):
    pr = nat.SotProblem()
    pr.B, pr.n, pr.m = B, n, m
    pr.x_row_stride, pr.y_row_stride = n, m
    pr.xpos_row_stride, pr.ypos_row_stride = (n, m) if rowpos else (0, 0)
    pr.p, pr.flags = 2.0, flags
    pr.row_perm_in, pr.row_perm_out = perm_in or None, perm_out or None
    pr.x = pr.y = pr.xpos = pr.ypos = 4096      # never followed: the size functions are host arithmetic
    return pr


@pytest.fixture(scope="module")
def nat():
    from sot_amd import _native
    _native.load()
    return _native


def test_abi_version_in_header_library_and_binding(nat):
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    assert int(re.search(r"#define SOT_ABI_VERSION (\d+)", header).group(1)) == nat.ABI_VERSION == nat.load().sot_abi_version() >= 18


SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 2048), (129, 257), (700, 700), (2048, 2048), (2049, 2049), (2048, 2049), (2049, 2), (4096, 8192), (16384, 16384)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_per_row_positions_get_the_image_exactly_where_the_pre_sort_runs(nat, n, m):
    lib = nat.load()
    in_domain = 2 <= n <= 2048 and 2 <= m <= 2048
    for B in (0, 1, 5, 4096):
        image = _up(B * (n + m) * 2)
        for flags in (RS, RS | 1 | 2 | 4, RS | NS, 0, NS):
            for perm_in, perm_out in ((0, 0), (4096, 0), (0, 4096), (4096, 8192)):
                pr = _problem(nat, B, n, m, flags, True, perm_in, perm_out)
                runs = bool(flags & RS) and not (flags & NS) and in_domain and B > 0 and not perm_in    # setup_launch's condition, restated
                want = image if runs and not perm_out else 0
                assert lib.sot_workspace_bytes(ctypes.byref(pr)) == want, (B, n, m, flags, perm_in, perm_out)
                # the binding allocates a workspace exactly when the library has a use for one
                assert nat._needs_workspace(pr, flags, None) == (want > 0), (B, n, m, flags, perm_in, perm_out)


def test_the_issue_example_4096_rows_of_8192_points_allocates_nothing(nat):
    pr = _problem(nat, 4096, 8192, 8192, RS, True)
    assert nat.load().sot_workspace_bytes(ctypes.byref(pr)) == 0


@pytest.mark.parametrize("n,m", SHAPES)
def test_shared_positions_still_get_the_plan_layout(nat, n, m):
    total = 2 * _up(4 * n) + 2 * _up(4 * m) + 256     # csrc/sot_launch.hpp: ws_layout -- sorted x, y, two int32 permutations, two flags
    for B in (0, 3):
        for flags in (RS, RS | NS, 0):
            pr = _problem(nat, B, n, m, flags, False)
            assert nat.load().sot_workspace_bytes(ctypes.byref(pr)) == total
            assert nat._needs_workspace(pr, flags, None) == bool(flags & RS)
            assert not nat._needs_workspace(pr, flags, object())     # a plan: nothing to prepare


def test_size_functions_return_zero_for_what_they_refuse(nat):
    lib = nat.load()
    assert lib.sot_workspace_bytes(None) == 0
    for n, m in ((0, 4), (4, 0), (-1, 4)):
        for rowpos in (False, True):
            assert lib.sot_workspace_bytes(ctypes.byref(_problem(nat, 3, n, m, RS, rowpos))) == 0
    # mixed supports: "0 for a problem the calls refuse, and when no workspace is needed"
    pr = _problem(nat, 3, 257, 37, RS, False)
    pr.ypos_row_stride = 37
    assert lib.sot_w1d_mixed_workspace_bytes(ctypes.byref(pr)) > 0
    for bad in ("both_shared", "both_rows", "p", "row_side_2049", "n0", "no_sort"):
        q = _problem(nat, 3, 257, 37, RS, False)
        q.ypos_row_stride = 37
        if bad == "both_shared":
            q.ypos_row_stride = 0
        elif bad == "both_rows":
            q.xpos_row_stride = 257
        elif bad == "p":
            q.p = 0.5
        elif bad == "row_side_2049":
            q.m, q.y_row_stride, q.ypos_row_stride = 2049, 2049, 2049
        elif bad == "n0":
            q.n = 0
        else:
            q.flags = 0
        assert lib.sot_w1d_mixed_workspace_bytes(ctypes.byref(q)) == 0, bad
    assert lib.sot_w1d_mixed_workspace_bytes(None) == 0
    # STFT backward: batch * groups * span floats, two frames per group
    assert lib.sot_stft_backward_workspace_bytes(2, 3001, 512, 128) == 4 * 2 * 12 * (512 + 128)
    for args in ((0, 3001, 512, 128), (2, 0, 512, 128), (2, 3001, 0, 128), (2, 3001, 512, 0), (-1, 3001, 512, 128)):
        assert lib.sot_stft_backward_workspace_bytes(*args) == 0, args
    # oscillator bank: samples <= 2^20, sinusoids <= 512
    assert lib.sot_oscillator_bank_workspace_bytes(2, 1541, 4) > 0
    for args in ((2, (1 << 20) + 1, 4), (2, 1541, 513), (2, 0, 4), (2, 1541, 0), (-1, 1541, 4)):
        assert lib.sot_oscillator_bank_workspace_bytes(*args) == 0, args
    # synthesiser: samples a multiple of frames, frames < samples
    assert lib.sot_synth_workspace_bytes(2, 2, 512, 4, 0) > 0 and lib.sot_synth_workspace_bytes(2, 2, 512, 4, 1) > 0
    for args in ((2, 2, 513, 4, 1), (2, 0, 512, 4, 1), (2, 2, 512, 513, 1), (2, 2, 512, 0, 1), (2, 512, 512, 4, 1), (-1, 2, 512, 4, 1)):
        assert lib.sot_synth_workspace_bytes(*args) == 0, args
    # fused multi-scale loss and metrics: powers of two in [64, 2048], at most 8 sizes
    def sizes(*v):
        return (ctypes.c_int * len(v))(*v)
    assert lib.sot_mss_workspace_bytes(2, 5000, ctypes.cast(sizes(64, 512, 2048), ctypes.c_void_p), 3) > 0
    for batch, samples, v in ((2, 5000, (32,)), (2, 5000, (4096,)), (2, 5000, (96,)), (2, 0, (64,)), (-1, 5000, (64,)), (2, 5000, (64,) * 9), (2, 5000, ())):
        assert lib.sot_mss_workspace_bytes(batch, samples, ctypes.cast(sizes(*v), ctypes.c_void_p) if v else None, len(v)) == 0, (batch, samples, v)
    assert lib.sot_spec_metrics_workspace_bytes(2, 5000, ctypes.cast(sizes(64, 512), ctypes.c_void_p), 2, 2) > 0
    for batch, samples, v, groups in ((2, 5000, (32,), 1), (2, 5000, (64,), 0), (2, 5000, (64,), 5), (2, 0, (64,), 1), (2, 5000, (64,) * 9, 1), (2, 5000, (), 1)):
        assert lib.sot_spec_metrics_workspace_bytes(batch, samples, ctypes.cast(sizes(*v), ctypes.c_void_p) if v else None, len(v), groups) == 0, (batch, samples, v, groups)
    # FIR: 3 <= n_taps <= 512, 1 <= samples <= 2^20
    assert lib.sot_fir_workspace_bytes(3, 1025, 128) > 0
    for args in ((3, 1025, 2), (3, 1025, 513), (3, 0, 128), (3, (1 << 20) + 1, 128), (-1, 1025, 128)):
        assert lib.sot_fir_workspace_bytes(*args) == 0, args
    assert lib.sot_spec_distance_workspace_bytes() == 8 * 1024


# ---- the coverage of tests/test_memory_contract_gpu.py ----
HOST_ONLY = {"sot_abi_version", "sot_status_string", "sot_stft_frames",   # host arithmetic
             "sot_profile_next_launch", "sot_profile_elapsed_ms"}          # arm / read a timer: they launch nothing


def _declared():
    header = open(os.path.join(ROOT, "include", "sot_hip.h")).read()
    return set(re.findall(r"^(?:int|int64_t|size_t|const char \*)\s*\*?\s*(sot_\w+)\s*\(", header, flags=re.M))


def test_every_enqueueing_function_of_the_header_has_a_memory_contract_case(nat):
    import test_memory_contract_gpu as mc
    declared = _declared()
    assert declared == set(nat.EXPORTS)
    allowed = HOST_ONLY | {name for name in declared if name.endswith("_bytes")}
    assert allowed <= declared
    covered = {entry for case in mc.CASES for entry in case.entries}
    assert covered <= declared, covered - declared
    missing = declared - allowed - covered
    assert not missing, f"no line in tests/test_memory_contract_gpu.py CASES for {sorted(missing)}"
    refused = {entry for r in mc.REFUSALS for entry in r.entries}
    assert declared - allowed <= refused, f"no refusal / empty-batch call for {sorted(declared - allowed - refused)}"


def test_every_row_loop_route_has_a_memory_contract_case():
    import test_memory_contract_gpu as mc
    import test_row_loop_gpu as rl
    have = {case.id for case in mc.CASES}
    for c in rl.CASES:
        assert c.id in have or c.id in mc.LEFT_OUT, c.id
        if c.id in have:
            mine = mc.BY_ID[c.id]
            assert (mine.n, mine.m, mine.cite) == (c.n, c.m, c.cite), c.id     # same lengths, same citations
    assert "fwd129_full" in have      # the 129-bin full kernel below 8192 rows, which the row-loop test cannot reach
    for name, reason in mc.LEFT_OUT.items():
        assert name not in have and len(reason) > 20, name


def test_small_batches_leave_a_partial_last_row_group():
    import test_memory_contract_gpu as mc
    for case in mc.CASES:
        if case.rows is None:
            continue
        B = mc.batch_rows(case)
        assert B >= case.lo and (case.hi is None or B <= case.hi), case.id
        assert B > case.rows and (case.rows == 1 or B % case.rows != 0), (case.id, B)
        assert B == 2 * case.rows + 1 or B in (case.lo + 1, case.lo + 2, mc.kFwd1025OneWaveRows - 1), (case.id, B)
