"""Heterogeneous batches for tests/test_row_loop_gpu.py: row r of a batch gets its nature -- a WEIGHT kind, and for per-row positions a POSITION
kind -- from a fixed multiplicative hash of r, so that in a persistent kernel a row follows rows of another nature, whatever the grid stride
(r % k would line up with a stride that shares a factor with k).  Everything is generated on the device the caller names, from a seeded
torch.Generator of that device; all kinds are finite.

Two tables of shares (out of 32 hash buckets).  WEIGHT_SHARE is the balanced one.  TIE_FREE_SHARE serves the comparisons with the CPU
route (position gradients, gradients of the quantile tensors), which leave rows with exactly tied CDF levels out and need at least half of
the check sample: there most rows are of the kind whose mass is under the guard, because a NORMALISED row is tied more often than not
whatever its weights -- both CDFs end at 1 up to a few ulp, so their last levels are equal in ~37 % of the rows (counted on the CPU), and
only a row that the guard leaves un-normalised escapes that; with `floor` the tie-free kinds also keep their weights away from 0, where
squared weights vanish under the ulp of the running sum and two neighbouring levels of ONE side tie."""
import torch

# kind -> buckets out of 32.  "tie-free" is a statement about the typical row (no runs of equal CDF levels), not a guarantee.
WEIGHT_KINDS = ("peaky", "uniform", "x_zero", "y_zero", "y_single", "sparse", "y_times_4", "tiny", "huge")
WEIGHT_SHARE = (5, 8, 2, 2, 2, 3, 4, 3, 3)
TIE_FREE_SHARE = (1, 3, 1, 1, 1, 1, 1, 22, 1)
POSITION_KINDS = ("sorted", "reversed", "random", "all_equal", "two_clusters", "pairs")
POSITION_SHARE = (8, 7, 11, 2, 2, 2)
TIE_FREE_POSITION_SHARE = (9, 8, 11, 1, 2, 1)
assert sum(WEIGHT_SHARE) == sum(TIE_FREE_SHARE) == sum(POSITION_SHARE) == sum(TIE_FREE_POSITION_SHARE) == 32

_MASK = 0xFFFFFFFF


def row_hash(rows, salt=0):
    """32-bit hash of the row indices (int64 tensor): a Knuth multiplication followed by two xor-shift-multiply rounds.  Every product
    stays below 2^63."""
    h = ((rows + salt) * 0x9E3779B1) & _MASK
    h = (((h >> 16) ^ h) * 0x45D9F3B) & _MASK
    h = (((h >> 16) ^ h) * 0x45D9F3B) & _MASK
    return (h >> 16) ^ h


def _kind_ids(B, share, salt, device):
    table = torch.tensor([k for k, s in enumerate(share) for _ in range(s)], dtype=torch.int64, device=device)
    return table[(row_hash(torch.arange(B, dtype=torch.int64, device=device), salt) >> 7) % 32]


def weight_kind_ids(B, device="cpu", share=WEIGHT_SHARE):
    """[B] int64: index into WEIGHT_KINDS of every row"""
    return _kind_ids(B, share, 0, device)


def position_kind_ids(B, device="cpu", share=POSITION_SHARE):
    """[B] int64: index into POSITION_KINDS of every row (another salt: independent of the weight kind)"""
    return _kind_ids(B, share, 0x51ED27, device)


def make_weights(B, n, m, seed, device="cpu", share=WEIGHT_SHARE, floor=0.0):
    """(x [B, n], y [B, m], kind ids [B]) float32 on `device`.  floor: the tie-free kinds draw their weights from [floor, 1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.rand(B, n, generator=g, device=device)
    y = torch.rand(B, m, generator=g, device=device)
    thin_x = torch.rand(B, n, generator=g, device=device) < 0.1
    thin_y = torch.rand(B, m, generator=g, device=device) < 0.1
    kind = weight_kind_ids(B, device, share)
    rows = torch.arange(B, dtype=torch.int64, device=device)

    def is_(name):
        return (kind == WEIGHT_KINDS.index(name))[:, None]

    if floor:
        lifted = is_("uniform") | is_("y_times_4") | is_("tiny") | is_("huge")
        x = torch.where(lifted, floor + (1.0 - floor) * x, x)
        y = torch.where(lifted, floor + (1.0 - floor) * y, y)

    x = torch.where(is_("peaky"), x ** 8, x)
    y = torch.where(is_("peaky"), y ** 8, y)
    x = torch.where(is_("x_zero"), torch.zeros_like(x), x)
    y = torch.where(is_("y_zero") | is_("y_single"), torch.zeros_like(y), y)
    x = torch.where(is_("sparse") & ~thin_x, torch.zeros_like(x), x)   # 90 % zeros: runs of tied levels
    y = torch.where(is_("sparse") & ~thin_y, torch.zeros_like(y), y)
    y = torch.where(is_("y_times_4"), y * 4.0, y)                      # levels pass 1: the cutoff and the clamp of the last rank bite
    scale = torch.where(is_("tiny"), 1e-12, 1.0) * torch.where(is_("huge"), 1e12, 1.0)   # tiny: mass under the 1e-7 guard of safe_divide
    x, y = x * scale.float(), y * scale.float()
    # a single non-zero bin whose column cycles through first, last and interior
    single = rows[kind == WEIGHT_KINDS.index("y_single")]
    h = row_hash(single, 0x2F0B1)
    interior = (1 + (h >> 3) % max(m - 2, 1)).clamp(max=m - 1)
    col = torch.stack((torch.zeros_like(single), torch.full_like(single, m - 1), interior))[torch.arange(single.numel(), device=device) % 3,
                                                                                          torch.arange(single.numel(), device=device)]
    y[single, col] = 0.75
    return x.contiguous(), y.contiguous(), kind


def make_positions(B, n, seed, device="cpu", share=POSITION_SHARE):
    """(positions [B, n] in [0, 1], kind ids [B]).  The kind of a row is the same for every n and seed, so the x and the y side of a row
    share it."""
    g = torch.Generator(device=device).manual_seed(seed)
    base = (torch.arange(n, device=device)[None, :] + 0.9 * torch.rand(B, n, generator=g, device=device)) / n   # sorted, distinct
    perm = torch.argsort(torch.rand(B, n, generator=g, device=device), dim=1)
    side = torch.rand(B, n, generator=g, device=device) < 0.5
    kind = position_kind_ids(B, device, share)

    def is_(name):
        return (kind == POSITION_KINDS.index(name))[:, None]

    pos = torch.where(is_("reversed"), base.flip(1), base)
    pos = torch.where(is_("random"), torch.gather(base, 1, perm), pos)
    pos = torch.where(is_("all_equal"), torch.full_like(base, 0.5), pos)
    pos = torch.where(is_("two_clusters"), torch.where(side, 0.25, 0.75) + 1e-2 * base, pos)   # (distinct: base's cells are 1e-2 / n apart)
    twin = base[:, (torch.arange(n, device=device) // 2) * 2]                      # every value twice
    pos = torch.where(is_("pairs"), torch.gather(twin, 1, perm), pos)
    return pos.float().contiguous(), kind


def check_sample(B, *kind_ids):
    """Sorted row indices (int64, CPU) of the check sample: the first 16 rows, the last 16, and for every kind of every given kind tensor
    the first and the last row of that kind."""
    picks = [torch.arange(min(16, B)), torch.arange(max(B - 16, 0), B)]
    for ids in kind_ids:
        ids = ids.cpu()
        for k in range(int(ids.max()) + 1):
            at = torch.nonzero(ids == k).flatten()
            if at.numel():
                picks.append(at[[0, -1]])
    return torch.unique(torch.cat(picks))


# The three modes every case runs: (name, p, flags of oracle/sot_oracle.py -- the library's low four bits are the same).
MODES = (("p1", 1.0, 8), ("paper", 2.0, 1 | 2 | 4 | 8), ("p3_dn", 3.0, 2 | 8))


# ---- audio clips for tests/test_signal_loops_gpu.py: the same hash, one kind per clip ---------------------------------------------------
# "tiny" is noise scaled by 1e-21 (magnitudes below the plain range of |.|: the careful path), "huge" by 1e6; the impulse sits in the clip's
# last hop, so that only the end-padded frames see it; the tone lies half-way between two bins of the transform and stands on a noise floor
# of 10 % of its amplitude.  The pure tone was measured first: at n_fft 64 its far bins sit at the rounding floor of ANY float32 FFT, where the
# direction X / |X| of the gradient is noise -- one clip of 100 samples came out at 3.57e-4 of its gradient's peak from float64 with the HIP slot
# kernels and 2.15e-4 with torch's float32 (1.66 x, against the 1.5 x + 1.5e-5 that tests/test_stft_producer.py establishes on the fixtures); roll
# and ends were bit-exact.  On a floor of 1 % the same clip met the max but not the rms figure once torch's float32 ran on the CPU (4.4e-6 against 2.1e-6: 2.1 x,
# the rule is 1.5 x + 1e-6).  The bound stays and the kind got its floor, as the 5000-point row of tests/test_row_loop_gpu.py moved.
CLIP_KINDS = ("noise", "tone", "impulse", "zeros", "tiny", "huge")
CLIP_SHARE = (6, 6, 5, 5, 5, 5)
assert sum(CLIP_SHARE) == 32


def clip_kind_ids(B, device="cpu", salt=0xC11B5):
    """[B] int64: index into CLIP_KINDS of every clip"""
    return _kind_ids(B, CLIP_SHARE, salt, device)


def make_clips(B, samples, seed, n_fft, hop, device="cpu", salt=0xC11B5):
    """(audio [B, samples] float32, kind ids [B]).  Another salt gives another assignment of kinds to clips (a target and an estimate)."""
    g = torch.Generator(device=device).manual_seed(seed)
    noise = torch.rand(B, samples, generator=g, device=device) - 0.5
    kind = clip_kind_ids(B, device, salt)
    rows = torch.arange(B, dtype=torch.int64, device=device)
    t = torch.arange(samples, dtype=torch.float64, device=device)[None, :]

    def is_(name):
        return (kind == CLIP_KINDS.index(name))[:, None]

    k = 2 + row_hash(rows, salt + 1) % max(n_fft // 2 - 4, 1)                       # the bin below the tone
    phase = (row_hash(rows, salt + 2) % 1024).double() / 1024.0
    tone = (0.5 * torch.sin(2.0 * torch.pi * ((k.double()[:, None] + 0.5) / n_fft * t + phase[:, None]))).float()
    at = samples - 1 - row_hash(rows, salt + 3) % min(hop, samples)                 # a sample of the last hop
    impulse = torch.zeros(B, samples, device=device)
    impulse[rows, at] = 1.0
    a = torch.where(is_("tone"), tone + 0.1 * noise, noise)      # (a floor under the tone: see CLIP_KINDS)
    a = torch.where(is_("impulse"), impulse, a)
    a = torch.where(is_("zeros"), torch.zeros_like(a), a)
    a = torch.where(is_("tiny"), noise * 1e-21, a)
    a = torch.where(is_("huge"), noise * 1e6, a)
    return a.contiguous(), kind
