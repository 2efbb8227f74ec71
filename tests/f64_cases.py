"""Inputs and the truth for the float64 kernels (csrc/sot_f64.hip; tests/test_f64_host.py, tests/test_f64_gpu.py).

TRUTH: SURVEY.md A.1 / A.2 restated in numpy with np.longdouble (x87 extended: 64-bit significand) and sequential sums.  The same
restatement runs in np.float64 with sequential or 64-blocked prefix sums (`dtype`, `block`): two float64 evaluations that differ only in the
order of their sums, which is what separates a kernel's scan from ATen's.

INPUTS.  Without the cutoff (MODES_PLAIN) generic random weights do: the two float64 evaluations agree to ~5e-14.  Under the cutoff
(dont_normalize + limit_quantile_range, MODES_CUTOFF) the level U_{n-1} ~ 1 is kept or dropped by its last bit, and generic
rows move by up to 1e-2 with the order of the prefix sums.  cutoff_rows() builds rows for which they cannot:
  * x holds integer multiples of 2^-5, k / 32 with k in [0, 32), and the mass the call normalises by -- sum x, or sum x^2 under square_dist --
    is a power of two: the quotients are k / T (k^2 / T), every partial sum is a multiple of 1 / T below 2^53 / T, so U is exact in every
    summation order and U_{n-1} == 1.0, never above;
  * how: draw k, keep SPARE bins at zero, and bring the mass to a power of two T: the next one above when the spare bins can hold the deficit,
    else the one below -- drawn bins are zeroed (in a random order) until the mass is <= T; the deficit (< 31, < 31^2 squared) then goes into
    the spare bins, greedily with integer squares in the squared case;
  * y holds generic random weights, scaled to 1.2 ... 1.5 times the mass of x: part of V lies above 1, so the cutoff acts; no level of V sits
    on the edge and none ties with a level of U.
"""
import numpy as np

LD = np.longdouble
SPARE = 8

# (name, p, square_dist, dont_normalize, limit_quantile_range)
MODES_PLAIN = (("p1", 1.0, False, False, False), ("p2_sq", 2.0, True, False, False), ("dn", 2.0, False, True, False),
               ("p3", 3.0, False, False, False), ("p1.5", 1.5, False, False, False))
MODES_CUTOFF = (("cut_p1", 1.0, False, True, True), ("paper", 2.0, True, True, True), ("cut_p3", 3.0, False, True, True))
MODES = MODES_PLAIN + MODES_CUTOFF


def mode_flags(mode):
    _, _, sq, dn, lim = mode
    return (1 if sq else 0) | (2 if dn else 0) | (4 if lim else 0)


def mode_kwargs(mode):
    """constructor arguments of Wasserstein1D for a mode (supports arrive sorted: require_sort is the caller's)"""
    _, p, sq, dn, lim = mode
    return dict(p=p, square_dist=sq, dont_normalize=dn, limit_quantile_range=lim)


def _scan(a, block):
    """inclusive prefix sums along the last axis in a's dtype: sequential, or blocks of `block` (block-local scans + a scan of the block sums)"""
    if block is None:
        return np.cumsum(a, axis=-1, dtype=a.dtype)
    n = a.shape[-1]
    out = np.empty_like(a)
    offset = np.zeros(a.shape[:-1], dtype=a.dtype)
    for lo in range(0, n, block):
        part = np.cumsum(a[..., lo:lo + block], axis=-1, dtype=a.dtype)
        out[..., lo:lo + block] = part + offset[..., None]
        offset = offset + part[..., -1]
    return out


def eval_rows(x, y, xpos, ypos, mode, dtype=LD, block=None, prenormalized=False):
    """[B] row losses W_p^p of SURVEY.md A.1 / A.2 in `dtype` (np.longdouble: the truth), sums sequential or blocked.  xpos / ypos: [n] / [m]
    shared or [B, n] / [B, m]; sorted."""
    _, p, sq, dn, lim = mode
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    B, n = x.shape
    m = y.shape[1]
    xs = np.broadcast_to(np.asarray(xpos, dtype=dtype), (B, n))
    ys = np.broadcast_to(np.asarray(ypos, dtype=dtype), (B, m))
    if prenormalized:
        a, b = x, y
    else:
        if sq:
            x, y = x * x, y * y
        eps = dtype(np.float32(1e-7))   # utils.py:135-142: a float32 1e-7, widened
        sx = _scan(x, block)[:, -1]
        sy = _scan(y, block)[:, -1]
        gx = np.where(sx <= 1e-7, eps, sx)
        gy = gx if dn else np.where(sy <= 1e-7, eps, sy)
        a, b = x / gx[:, None], y / gy[:, None]
    U, V = _scan(a, block), _scan(b, block)
    out = np.empty(B, dtype=dtype)
    pw = dtype(p)
    for r in range(B):
        Q = np.sort(np.concatenate((U[r], V[r])), kind="stable")
        iu = np.minimum(np.searchsorted(U[r], Q, side="left"), n - 1)
        iv = np.minimum(np.searchsorted(V[r], Q, side="left"), m - 1)
        delta = np.diff(Q, prepend=dtype(0))
        if lim:
            delta = np.where(Q > 1, dtype(0), delta)
        gap = np.abs(xs[r][iu] - ys[r][iv])
        cost = gap if p == 1 else (gap * gap if p == 2 else gap ** pw)
        out[r] = np.cumsum(delta * cost, dtype=dtype)[-1] if Q.size else dtype(0)
    return out


def grid(n):
    return np.linspace(0.0, 1.0, n)


def sorted_positions(rng, shape):
    return np.sort(rng.random(shape), axis=-1)


def plain_rows(B, n, m, seed, zero_row=None):
    """generic random weights in [0, 1); zero_row: that row of x AND of y is all zero (the mass guard)"""
    rng = np.random.default_rng(seed)
    x, y = rng.random((B, n)), rng.random((B, m))
    if zero_row is not None:
        x[zero_row] = 0.0
        y[zero_row] = 0.0
    return x, y


def _greedy_squares(deficit):
    out = []
    while deficit > 0:
        k = min(31, int(np.floor(np.sqrt(deficit))))
        while k * k > deficit:
            k -= 1
        out.append(k)
        deficit -= k * k
    return out


def _dyadic_row(rng, n, squared):
    """integers k[n] in [0, 32) with sum k (sum k^2 when squared) a power of two"""
    if n <= SPARE:   # tiny rows: 1, 2 or 4 bins of 16 / 32 (sum and sum of squares are both powers of two)
        k = np.zeros(n, dtype=np.int64)
        k[rng.permutation(n)[:max(c for c in (1, 2, 4) if c <= n)]] = 16
        return k
    spare = SPARE
    k = rng.integers(0, 32, size=n)
    free = rng.permutation(n)
    spare_at, drawn_at = free[:spare], free[spare:]
    k[spare_at] = 0
    unit = (lambda v: v * v) if squared else (lambda v: v)
    mass = int(unit(k).sum())
    if mass == 0:
        k[drawn_at[0]] = 1
        mass = 1
    target = 1 << (mass - 1).bit_length()          # the next power of two >= mass
    if target - mass > (31 * 31 - 1 if squared else 31 * spare):   # more than the spare bins hold for sure: the power of two below
        target //= 2
        for at in drawn_at:
            if mass <= target:
                break
            mass -= int(unit(k[at]))
            k[at] = 0
    fill = _greedy_squares(target - mass) if squared else [min(31, target - mass - 31 * i) for i in range((target - mass + 30) // 31)]
    assert len(fill) <= spare, (n, target, mass, fill)
    for at, v in zip(spare_at, fill):
        k[at] = v
    assert int(unit(k).sum()) == target and k.min() >= 0 and k.max() <= 31
    return k


def cutoff_rows(B, n, m, squared, seed):
    """(x, y) for the cutoff modes, see the module docstring; squared: the mass that is a power of two is sum x^2"""
    rng = np.random.default_rng(seed)
    x = np.stack([_dyadic_row(rng, n, squared) for _ in range(B)]).astype(np.float64) / 32.0
    y = rng.random((B, m)) + 1e-3
    ratio = rng.uniform(1.2, 1.5, size=(B, 1))
    if squared:
        y *= np.sqrt(ratio * (x * x).sum(1, keepdims=True) / (y * y).sum(1, keepdims=True))
    else:
        y *= ratio * x.sum(1, keepdims=True) / y.sum(1, keepdims=True)
    return x, y


def rows_for(mode, B, n, m, seed, zero_row=None):
    """the inputs a mode is tested on: the recipe under the cutoff, generic rows otherwise"""
    if mode[4]:
        return cutoff_rows(B, n, m, mode[2], seed)
    return plain_rows(B, n, m, seed, zero_row)
