"""CPU tests of tests/row_kinds.py, the input generator of tests/test_row_loop_gpu.py."""
import numpy as np
import pytest
import torch

import row_kinds as rk


def test_kinds_do_not_follow_the_row_index_modulo_anything_small():
    """The kind must not line up with a grid stride: for every stride up to 64 (and the strides of real grids, 256 CUs x 1 ... 8 workgroups) the
    rows a workgroup visits, w, w + stride, ..., hold more than one kind."""
    B = 49155
    for ids in (rk.weight_kind_ids(B), rk.position_kind_ids(B)):
        for stride in list(range(1, 65)) + [256, 512, 1024, 2048]:
            for w in (0, 1, stride - 1):
                assert torch.unique(ids[w::stride][:64]).numel() > 1, (stride, w)


def test_every_kind_occurs_with_its_share_and_the_sample_holds_every_kind():
    for B, wshare, pshare in ((1539, rk.WEIGHT_SHARE, rk.POSITION_SHARE), (6147, rk.WEIGHT_SHARE, rk.POSITION_SHARE),
                              (49155, rk.WEIGHT_SHARE, rk.POSITION_SHARE), (1539, rk.TIE_FREE_SHARE, rk.TIE_FREE_POSITION_SHARE),
                              (24579, rk.TIE_FREE_SHARE, rk.TIE_FREE_POSITION_SHARE)):
        wk, pk = rk.weight_kind_ids(B, share=wshare), rk.position_kind_ids(B, share=pshare)
        for ids, share in ((wk, wshare), (pk, pshare)):
            got = torch.bincount(ids, minlength=len(share)).double() / B
            want = torch.tensor(share).double() / 32
            assert (got > 0).all() and float((got - want).abs().max()) < 0.03, (B, got.tolist())
        sample = rk.check_sample(B, wk, pk)
        assert set(wk[sample].tolist()) == set(range(len(rk.WEIGHT_KINDS)))
        assert set(pk[sample].tolist()) == set(range(len(rk.POSITION_KINDS)))
        assert set(range(16)) <= set(sample.tolist()) and set(range(B - 16, B)) <= set(sample.tolist())
        assert sample.numel() <= 32 + 2 * (len(rk.WEIGHT_KINDS) + len(rk.POSITION_KINDS))
        assert torch.equal(sample, torch.unique(sample))


def test_generator_is_deterministic_and_finite():
    a = rk.make_weights(777, 64, 70, 5)
    b = rk.make_weights(777, 64, 70, 5)
    c = rk.make_weights(777, 64, 70, 6)
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and not torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])
    p, q = rk.make_positions(777, 64, 9), rk.make_positions(777, 64, 9)
    assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])
    assert a[0].dtype == a[1].dtype == p[0].dtype == torch.float32 and a[0].is_contiguous() and p[0].is_contiguous()
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all() and torch.isfinite(p[0]).all()
    assert float(p[0].min()) >= 0.0 and float(p[0].max()) <= 1.0


def test_rows_are_of_their_kind():
    x, y, kind = rk.make_weights(3000, 64, 64, 1)
    rows = {name: torch.nonzero(kind == k).flatten() for k, name in enumerate(rk.WEIGHT_KINDS)}
    assert (x[rows["x_zero"]] == 0).all() and (y[rows["x_zero"]] > 0).any()
    assert (y[rows["y_zero"]] == 0).all()
    single = y[rows["y_single"]]
    assert ((single != 0).sum(1) == 1).all()
    cols = set(torch.nonzero(single)[:, 1].tolist())
    assert 0 in cols and 63 in cols and len(cols - {0, 63}) >= 1          # first, last and interior columns
    assert 0.8 < float((x[rows["sparse"]] == 0).double().mean()) < 0.97
    assert float(y[rows["y_times_4"]].max()) > 2.0
    assert float(x[rows["tiny"]].sum(1).max()) < 1e-7 and float(x[rows["tiny"]].max()) > 0
    assert float(x[rows["huge"]].max()) > 1e11
    assert float(x[rows["peaky"]].median()) < 0.05 < float(x[rows["uniform"]].median())
    pos, pk = rk.make_positions(3000, 64, 2)
    prow = {name: pos[pk == k] for k, name in enumerate(rk.POSITION_KINDS)}
    assert (prow["sorted"][:, 1:] > prow["sorted"][:, :-1]).all() and (prow["reversed"][:, 1:] < prow["reversed"][:, :-1]).all()
    assert not (prow["random"][:, 1:] > prow["random"][:, :-1]).all(1).any()
    assert (prow["all_equal"] == 0.5).all()
    assert ((prow["two_clusters"] - 0.5).abs() > 0.2).all() and ((prow["two_clusters"] - 0.5).abs() < 0.27).all()
    srt = torch.sort(prow["pairs"], 1)[0]
    assert (srt[:, 0::2] == srt[:, 1::2]).all()


@pytest.fixture(scope="module")
def oracle_rows():
    """The oracle's row losses of the three modes on a heterogeneous batch at N = 64, shared and per-row positions."""
    from oracle import sot_oracle as so
    B, N = 1200, 64
    x, y, kind = rk.make_weights(B, N, N, 3)
    xp, pk = rk.make_positions(B, N, 4)
    yp, _ = rk.make_positions(B, N, 5)
    lin = torch.linspace(0, 1, N).numpy()
    shared = {name: so.forward(x.numpy(), y.numpy(), lin, lin, p=p, flags=flags) for name, p, flags in rk.MODES}
    rowpos = {name: so.forward(x.numpy(), y.numpy(), xp.numpy(), yp.numpy(), p=p, flags=flags) for name, p, flags in rk.MODES}
    return kind, pk, shared, rowpos


def test_oracle_is_finite_on_every_kind_in_all_three_modes(oracle_rows):
    kind, _, shared, rowpos = oracle_rows
    assert set(kind.tolist()) == set(range(len(rk.WEIGHT_KINDS)))
    for losses in (shared, rowpos):
        for name, rows in losses.items():
            assert np.isfinite(rows).all() and (rows >= 0).all(), name


def test_oracle_tells_the_three_modes_apart_on_the_peaky_and_the_times_4_kinds(oracle_rows):
    """As tests/test_full_row_modes_gpu.py: a kernel of another mode cannot pass the comparison with the oracle.  Two modes are two
    different functions of the row, so their losses meet within 1e-3 relative -- a hundred times the tolerance of that comparison -- only
    by chance: about one row in 250 for the closest pair (paper mode against p = 3; counted over eight seeds when this test was written,
    before any kernel ran).  Asserted: on each of the two kinds, for any two modes, at least 98 % of the rows differ by >= 1e-3 and the
    median row by >= 1e-2.  (Rows whose positions are all equal cost exactly 0 in every mode and are left out; the GPU test asserts
    the separation again on the sample rows it compares.)"""
    kind, pk, shared, rowpos = oracle_rows
    spread = (pk != rk.POSITION_KINDS.index("all_equal")).numpy()
    for name in ("peaky", "y_times_4"):
        rows = kind.numpy() == rk.WEIGHT_KINDS.index(name)
        assert rows.sum() >= 50
        for losses, keep in ((shared, rows), (rowpos, rows & spread)):
            names = list(losses)
            for i, a in enumerate(names):
                for b in names[i + 1:]:
                    u, v = losses[a][keep].astype(np.float64), losses[b][keep].astype(np.float64)
                    assert (np.maximum(u, v) > 0).all()
                    sep = np.abs(u - v) / np.maximum(u, v)
                    assert (sep >= 1e-3).mean() >= 0.98 and np.median(sep) >= 1e-2, (name, a, b, float((sep >= 1e-3).mean()), float(np.median(sep)))


@pytest.mark.parametrize("n,m,B", [(300, 300, 24579), (520, 80, 12291), (2100, 90, 1539)])
def test_tie_free_shares_leave_half_of_the_sample_without_a_tie(n, m, B):
    """The comparisons with the CPU route in tests/test_row_loop_gpu.py leave out sample rows with exactly tied merged levels or positions and
    assert that half of the sample remains.  Here the same count on the CPU generator (other random numbers than the device's, the same kinds
    and sample rows), per-row positions, all three modes: at least 52 %, so that the draw on the device has some room."""
    from oracle import torch_restatement as tr
    x, y, wk = rk.make_weights(B, n, m, 7000 + n + m, share=rk.TIE_FREE_SHARE, floor=0.25)
    xp, pk = rk.make_positions(B, n, 100 + n, share=rk.TIE_FREE_POSITION_SHARE)
    yp, _ = rk.make_positions(B, m, 200 + m, share=rk.TIE_FREE_POSITION_SHARE)
    s = rk.check_sample(B, wk, pk)
    for name, p, flags in rk.MODES:
        Q = tr.sot_loss(x[s], y[s], xp[s], yp[s], p=p, square_dist=bool(flags & 1), dont_normalize=bool(flags & 2),
                        limit_quantile_range=bool(flags & 4), return_quantiles=True)[2]
        tied = (Q[:, 1:] == Q[:, :-1]).any(1)
        for pos in (xp[s], yp[s]):
            srt = torch.sort(pos, 1)[0]
            tied |= (srt[:, 1:] == srt[:, :-1]).any(1)
        assert float((~tied).double().mean()) >= 0.52, (name, int((~tied).sum()), len(s))


def test_clip_kinds_follow_each_other_at_every_grid_stride():
    """tests/test_signal_loops_gpu.py: a workgroup's next clip is `stride` clips on; every ordered pair of kinds occurs at the strides the
    capped grids have on 256 and 304 CUs (clips, workgroups of 16 / 8 / 4 frames of 9- and 17-frame clips) and at the small ones."""
    for B, strides in ((513, (1, 2, 3, 7, 64, 256)), (609, (304,)), (2000, (128, 455, 512, 608))):      # 513 = 2 * 256 + 1 clips: the clip kernel's batch
        kind = rk.clip_kind_ids(B)
        assert torch.bincount(kind, minlength=len(rk.CLIP_KINDS)).min() >= B // 10
        for stride in strides:
            pairs = set(zip(kind[:-stride].tolist(), kind[stride:].tolist()))
            assert len(pairs) == len(rk.CLIP_KINDS) ** 2, (B, stride, len(pairs))
    other = rk.clip_kind_ids(B, salt=0x7E57)
    assert 0.05 < float((other == kind).float().mean()) < 0.5      # an independent assignment: a target and an estimate of unlike kinds


def test_clips_are_what_their_kind_says():
    n_fft, hop, samples = 64, 16, 100
    a, kind = rk.make_clips(400, samples, 1, n_fft, hop)
    assert a.dtype == torch.float32 and a.shape == (400, samples) and bool(torch.isfinite(a).all())
    of = lambda name: a[kind == rk.CLIP_KINDS.index(name)]      # noqa: E731
    assert float(of("zeros").abs().max()) == 0.0
    assert 0 < float(of("tiny").abs().max()) < 1e-21 and 1e5 < float(of("huge").abs().max()) <= 5e5
    imp = of("impulse")
    assert bool(((imp != 0).sum(1) == 1).all()) and bool((imp[:, :samples - hop] == 0).all()) and float(imp.max()) == 1.0
    spec = torch.fft.rfft(of("tone")[:, :n_fft].double() * torch.hann_window(n_fft, dtype=torch.float64)).abs()
    top = torch.topk(spec, 2, dim=1)
    assert bool(((top.indices[:, 0] - top.indices[:, 1]).abs() == 1).all())      # between two bins: the two largest are neighbours ...
    assert bool((top.values[:, 1] > 0.5 * top.values[:, 0]).all())               # ... of comparable size
