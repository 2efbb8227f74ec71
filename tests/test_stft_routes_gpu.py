"""-m gpu: the ROUTE TABLE of the STFT producer (csrc/sot_stft.hip: pick_forward_route, pick_backward_route), pinned at its boundaries.

The routes of n_fft 2048 are different factorisations of one transform and agree to a few ulp only, so a threshold that is off by one moves
calls to another kernel without any tolerance noticing.  What does notice: a frame's result does not depend on which other frames share
the launch, and a clip's gradient does not depend on the rest of the batch -- so a result is torch.equal to the one the same data gives in
a call well inside a route if and only if the same kernel served both.  Every test runs a call on one side of a boundary, asserts bitwise
equality with the reference call of the route the table names, and asserts that the two references it tells apart are NOT bitwise equal
on its input (a test that could not tell them apart would prove nothing).

Forward references are calls of 16-frame clips (4096 samples at hop 256): 8 clips per call = 128 frames for the slot route, 64 clips =
1024 frames for wavew, 384 clips = 6144 frames for wave2.  A call of longer clips is compared through 16-frame WINDOWS of its clips:
window (b, s) = samples [256 s, 256 s + 4096) of clip b; its frames 0 .. 7 see the samples frames s .. s + 7 of the clip see, and the
window that ends with the clip (s = frames - 16) shares the clip's end padding too, so all 16 of its frames count.
Backward references are calls of the same clips (with the spectrum one forward call stored): 4 clips per call for the slot route, the
clips repeated to 128 for the clip route (16-frame clips) and to at least 2048 frame groups for wave2."""
import pytest
import torch

from gpu_util import device, native

pytestmark = pytest.mark.gpu

N_FFT, NB = 2048, 1025
# the thresholds of csrc/sot_stft.hip, mirrored: kFwdWavewMinFrames, kWave2MinFrames, kBwdClipMinClips, kBwdClipMaxFrames, kBwdWave2MinGroups
WAVEW_MIN, WAVE2_MIN, CLIP_MIN_CLIPS, CLIP_MAX_FRAMES, BWD_WAVE2_MIN_GROUPS = 512, 3072, 64, 16, 1024
REF_SLOT, REF_WAVEW, REF_WAVE2 = 8, 64, 384      # 16-frame clips per forward reference call
assert REF_SLOT * 16 < WAVEW_MIN <= REF_WAVEW * 16 < WAVE2_MIN <= REF_WAVE2 * 16


def _audio(batch, samples, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(batch, samples, generator=g) * 2 - 1).to(device())


def _window():
    return torch.hann_window(N_FFT, periodic=True, dtype=torch.float32).to(device())


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
def _windows(audio, frames, hop=256):
    """the 16-frame windows of every clip: (clips [n, 16 hop], rows of the call's frames, rows of the windows' frames) -- see the module text"""
    assert frames >= 16 and audio.shape[1] == frames * hop
    clips, ti, ri = [], [], []
    for b in range(audio.shape[0]):
        for s in list(range(0, frames - 16, 8)) + [frames - 16]:
            for j in range(16 if s == frames - 16 else 8):
                ti.append(b * frames + s + j)
                ri.append(len(clips) * 16 + j)
            clips.append(audio[b, s * hop:(s + 16) * hop])
    assert sorted(set(ti)) == list(range(audio.shape[0] * frames))   # every frame of the call is compared
    return torch.stack(clips), torch.tensor(ti, device=audio.device), torch.tensor(ri, device=audio.device)


def _forward_ref(nat, clips, window, per_call):
    """magnitudes and spectra of the 16-frame clips, from calls of exactly per_call clips each (the last one filled up from the front)"""
    n = clips.shape[0]
    mags, specs = [], []
    for start in range(0, n, per_call):
        idx = torch.tensor([(start + i) % n for i in range(per_call)], device=clips.device)
        mag, spec = nat.stft_mag_forward(clips[idx], window, N_FFT, 256, want_spec=True)
        keep = min(per_call, n - start)
        mags.append(mag[:keep]); specs.append(spec[:keep])
    return torch.cat(mags).flatten(0, 1), torch.cat(specs).flatten(0, 1)


def _same(got, ref, ti, ri):
    return torch.equal(got[0][ti], ref[0][ri]) and torch.equal(got[1][ti], ref[1][ri])


def _forward_case(batch, frames, served_by, other):
    """one call of batch x frames frames: bitwise the reference of route `served_by`, which differs from the reference of route `other`"""
    nat, window = native(), _window()
    audio = _audio(batch, frames * 256, seed=1000 + batch * frames)
    mag, spec = nat.stft_mag_forward(audio, window, N_FFT, 256, want_spec=True)
    got = (mag.flatten(0, 1), spec.flatten(0, 1))
    clips, ti, ri = _windows(audio, frames)
    ref = {per_call: _forward_ref(nat, clips, window, per_call) for per_call in (served_by, other)}
    all_rows = torch.arange(ref[served_by][0].shape[0], device=audio.device)
    assert not _same(ref[served_by], ref[other], all_rows, all_rows), "the two reference routes agree bitwise on this input: no power"
    assert _same(got, ref[served_by], ti, ri), "the call was not served by the kernel the route table names"
    assert not _same(got, ref[other], ti, ri)


def test_forward_511_frames_slot():
    batch, frames = 1, 511
    assert batch * frames == WAVEW_MIN - 1
    _forward_case(batch, frames, served_by=REF_SLOT, other=REF_WAVEW)


def test_forward_512_frames_wavew():
    batch, frames = 1, 512
    assert batch * frames == WAVEW_MIN
    _forward_case(batch, frames, served_by=REF_WAVEW, other=REF_SLOT)


def test_forward_3071_frames_wavew():
    batch, frames = 83, 37
    assert batch * frames == WAVE2_MIN - 1
    _forward_case(batch, frames, served_by=REF_WAVEW, other=REF_WAVE2)


def test_forward_3072_frames_wave2():
    batch, frames = 192, 16
    assert batch * frames == WAVE2_MIN
    _forward_case(batch, frames, served_by=REF_WAVE2, other=REF_WAVEW)


@pytest.mark.parametrize("each, served_by, alone", [(16, REF_WAVEW, REF_SLOT), (96, REF_WAVE2, REF_WAVEW)], ids=["2x256", "2x1536"])
def test_forward_pair_counts_both_signals(each, served_by, alone):
    """the pair form of 2 x `each` clips of 16 frames: the route of 2 x each x 16 frames, not the one a signal alone would take (`alone`)"""
    frames = 16
    assert 2 * each * frames in (WAVEW_MIN, WAVE2_MIN)
    assert (alone == REF_SLOT and each * frames < WAVEW_MIN) or (alone == REF_WAVEW and WAVEW_MIN <= each * frames < WAVE2_MIN)
    nat, window = native(), _window()
    a, b = _audio(each, frames * 256, seed=2000 + each), _audio(each, frames * 256, seed=3000 + each)
    mag_a, mag_b, spec_b = nat.stft_mag_forward_pair(a, b, window, N_FFT, 256, want_spec_b=True)
    ref = {per_call: _forward_ref(nat, torch.cat([a, b]), window, per_call) for per_call in (served_by, alone)}
    assert not (torch.equal(ref[served_by][0], ref[alone][0]) and torch.equal(ref[served_by][1], ref[alone][1])), "no power"
    mags = torch.cat([mag_a, mag_b]).flatten(0, 1)
    assert torch.equal(mags, ref[served_by][0]) and torch.equal(spec_b.flatten(0, 1), ref[served_by][1][each * frames:])
    assert not (torch.equal(mags, ref[alone][0]) and torch.equal(spec_b.flatten(0, 1), ref[alone][1][each * frames:]))


# ---- backward from the stored spectrum ---------------------------------------------------------------------------------------------------
class _Clips:
    """`batch` clips of `frames` frames with the spectrum ONE forward call stored and an upstream gradient; gradient of any selection of them"""

    def __init__(self, batch, frames, hop, seed):
        self.nat, self.window, self.hop, self.batch, self.frames = native(), _window(), hop, batch, frames
        self.audio = _audio(batch, frames * hop, seed)
        self.spec = self.nat.stft_mag_forward(self.audio, self.window, N_FFT, hop, want_spec=True)[1]
        g = torch.Generator().manual_seed(seed + 1)
        self.grad_mag = torch.randn(batch, frames, NB, generator=g).to(device())
        self.groups = (frames + 1) // 2                                  # kFramesPerGroup = 2

    def grad(self, idx):
        idx = torch.tensor(idx, device=self.audio.device)
        return self.nat.stft_mag_backward(self.audio[idx], self.window, N_FFT, self.hop, self.grad_mag[idx], spec=self.spec[idx].contiguous())

    def whole(self):
        return self.grad(list(range(self.batch)))

    def ref(self, per_call):
        """every clip's gradient from calls of exactly per_call clips each (filled up with further clips of the same set)"""
        out = []
        for start in range(0, self.batch, per_call):
            out.append(self.grad([(start + i) % self.batch for i in range(per_call)])[:min(per_call, self.batch - start)])
        return torch.cat(out)

    def route(self, per_call):
        """the route of a call of per_call of these clips, by the table of csrc/sot_stft.hip: pick_backward_route"""
        if 1 <= self.frames <= CLIP_MAX_FRAMES and self.hop % 2 == 0 and per_call >= CLIP_MIN_CLIPS:
            return "clip"
        if per_call * self.groups >= BWD_WAVE2_MIN_GROUPS and self.hop in (256, 512):
            return "wave2"
        return "slot"


REF_BWD_SLOT = 4


def _backward_case(batch, frames, hop, served_by, other_per_call):
    """the call of all `batch` clips is bitwise the reference of route `served_by` and differs from the calls of other_per_call clips,
    which another route serves"""
    c = _Clips(batch, frames, hop, seed=5000 + 97 * batch + frames + hop)
    assert c.route(batch) == served_by
    per_call = {"slot": REF_BWD_SLOT, "clip": 128, "wave2": -(-2048 // c.groups)}
    assert c.route(per_call[served_by]) == served_by and c.route(other_per_call) != served_by
    ref, other = c.ref(per_call[served_by]), c.ref(other_per_call)
    assert not torch.equal(ref, other), "the two reference routes agree bitwise on this input: no power"
    got = c.whole()
    assert torch.equal(got, ref), "the call was not served by the kernel the route table names"
    assert not torch.equal(got, other)


def test_backward_63_clips_slot():
    batch, frames = CLIP_MIN_CLIPS - 1, 16
    assert batch * (frames // 2) < BWD_WAVE2_MIN_GROUPS
    _backward_case(batch, frames, 256, "slot", other_per_call=128)


def test_backward_64_clips_clip():
    batch, frames = CLIP_MIN_CLIPS, 16
    _backward_case(batch, frames, 256, "clip", other_per_call=REF_BWD_SLOT)


def test_backward_64_clips_of_17_frames_not_clip():
    batch, frames = CLIP_MIN_CLIPS, CLIP_MAX_FRAMES + 1
    assert batch * 9 < BWD_WAVE2_MIN_GROUPS                              # 9 groups per clip: not wave2 either
    _backward_case(batch, frames, 256, "slot", other_per_call=-(-2048 // 9))   # (17 frames never take the clip route: the other is wave2)


def test_backward_1023_groups_slot():
    batch, frames = 33, 62
    assert batch * (frames // 2) == BWD_WAVE2_MIN_GROUPS - 1 and batch < CLIP_MIN_CLIPS
    _backward_case(batch, frames, 256, "slot", other_per_call=2 * batch)


def test_backward_1024_groups_wave2():
    batch, frames = 32, 64
    assert batch * (frames // 2) == BWD_WAVE2_MIN_GROUPS and batch < CLIP_MIN_CLIPS
    _backward_case(batch, frames, 256, "wave2", other_per_call=REF_BWD_SLOT)


def test_backward_hop_512_wave2():
    batch, frames = 32, 64
    assert batch * (frames // 2) >= BWD_WAVE2_MIN_GROUPS
    _backward_case(batch, frames, 512, "wave2", other_per_call=REF_BWD_SLOT)


def test_backward_hop_128_slot():
    """hop 128 has no route but the slot kernel's (its clips of 64 frames are too long for the clip route), so there is no second reference
    to differ from: the call of 1024 groups is bitwise the calls of 4 clips.  (What a wrong hop predicate would run, the wave2 kernel with
    the register offset of another hop, is not a different rounding but a different result.)"""
    batch, frames, hop = 32, 64, 128
    c = _Clips(batch, frames, hop, seed=7000)
    assert batch * c.groups >= BWD_WAVE2_MIN_GROUPS and c.route(batch) == "slot" and c.route(REF_BWD_SLOT) == "slot"
    assert torch.equal(c.whole(), c.ref(REF_BWD_SLOT))
