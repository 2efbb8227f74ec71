"""-m gpu: the SECOND AND LATER ROUNDS of the capped grids of the signal objects (csrc/sot_stft.hip, csrc/sot_osc.hip, csrc/sot_mss.hip) --
what tests/test_row_loop_gpu.py does for the row kernels.

These kernels start a capped number of workgroups and each walks its units of work -- frames, groups of two frames, clips, blocks of
elements -- with a stride of the grid, through the same LDS buffers and with lane-derived addresses carried across iterations.  A stale
buffer, a missing barrier between two units or a partial last round shows from a workgroup's second unit on, and depends on what the
previous unit was.  The batch forces the rounds from the device's CU count alone: for a capped_grid(groups, per_cu) launch a round is
CUs * per_cu workgroups, and the batch holds 2 rounds + 1 workgroups' worth of work with a partial last unit; for the grids capped by a
constant (65535 clips in gridDim.y, 64 blocks in gridDim.x, kDistBlocks, 8192, 16384, 4096 workgroups) the constant takes the place of the round.

Clips are heterogeneous (tests/row_kinds.py: CLIP_KINDS -- noise, a tone between two bins on a 10 % noise floor, an impulse in the last hop, zeros, noise * 1e-21,
noise * 1e6 -- drawn per clip from a hash of its index, so every kind follows every other at every grid stride: tests/test_row_kinds.py).

Each line of CASES asserts, in the order of tests/test_row_loop_gpu.py:
  1. ROLL INVARIANCE, bit for bit: the call on the batch rolled along dim 0 by 1 and by B // 2 + 1, rolled back, equals the first call on every
     output -- the backward with accumulate = 1 onto a random base and a device grad_scale.
  2. ENDS ALONE: the first and the last min(CUs, 64) clips as calls of their own: bit for bit where the same kernel serves them; where the
     line's `ends` column cites the dispatch line that sends the small call to another kernel, within the bound
     test_one_wave_per_frame_kernels_of_large_batches (tests/test_stft_producer.py) uses between the two factorisations: 1e-6 of the peak
     forward, 2e-5 of the gradient's peak backward.
  3. FLOAT64 on the check sample (rk.check_sample: first and last 16 clips, first and last clip of every kind), by the rule the existing test
     of the same object applies, PER CLIP (each clip against its own peak, so that the 1e6 clips do not hide the others):
       STFT magnitudes   within 2e-6 of the peak of torch.stft in float64 (tests/test_stft_producer.py); zeros exactly 0; the 1e-21 clips within
                         1e-5 (the `rel5` figure of test_one_wave_per_frame_kernels_of_large_batches for the careful |.| path);
       STFT spectra      within 2e-5 of the peak (test_stored_spectrum... in tests/test_stft_producer.py);
       STFT gradients    error against float64 (max, median, rms over the clip, of its peak) <= 1.5 x the error of torch's float32 evaluation
                         + 1.5e-5 / 1e-6 / 1e-6 (test_hip_gradients_are_as_close_to_float64_as_the_reference_float32);
       envelopes         the bits of tests/synth_model.py (its envelopes are a bit-exact model);
       spec distances    2e-6 relative forward, 1e-5 of the gradient's peak backward (test_spec_distance_kernels_against_torch), against float64;
       MSS per clip      loss within 1e-5, gradient norm error <= 1.5 x the float32 reference's + 5e-6, median <= 1.5 x + 1e-8 (tests/test_mss_fused.py: _check);
       metrics per clip  e_new <= 4 max(e_ref, e_stft) + 1e-6 |f64| (tests/test_eval_metrics_gpu.py: _accuracy).

NOT REACHABLE by this method (asserted in test_what_no_batch_can_reach, which fails on a device where the arithmetic turns):
  * stft_mag_forward_wavew_kernel serves 512 ... 3071 frames (csrc/sot_stft.hip pick_forward_route) on capped_grid(frames / 4, 3) (launch_forward_wavew): a round is
    3 CUs workgroups of 4 frames = 12 CUs frames = 3072 on 256 CUs, one more than the largest batch the kernel takes.  No workgroup runs
    a second frame group; below 256 CUs some would.
  * stft_mag_forward_persistent_kernel serves fewer than 512 frames of n_fft 2048, one frame per workgroup (pick_forward_route, launch_forward_persistent), on the resident
    grid of an occupancy query; amdgpu_waves_per_eu(6, 8) and 16.6 KB of LDS per 256-thread workgroup make that at least 6 CUs workgroups,
    so a second round needs 511 > 6 CUs: fewer than 86 CUs.  Its loop runs once per workgroup on every MI300-class part.
"""
import collections
import functools

import numpy as np
import pytest
import torch

import row_kinds as rk
import test_row_loop_gpu as rl
from gpu_util import device, native

pytestmark = pytest.mark.gpu

STFT, OSC, MSS = "csrc/sot_stft.hip", "csrc/sot_osc.hip", "csrc/sot_mss.hip"
kWave2Waves, kBwdWave2Waves, kFwdwWaves = 16, 8, 4      # csrc/sot_stft_wave2.hpp kWave2Waves, kBwdWave2Waves; csrc/sot_stft_wfft.hpp kFwdwWaves
kDistBlocks, kDistBwdBlocks, kThreads = 1024, 8192, 256   # csrc/sot_spec_distance.hip kDistBlocks, kGradBlocks, kThreads
kGridY, kOlaGridX = 65535, 64                               # csrc/sot_stft.hip sot_stft_mag_backward_spec: the overlap-add grid
kMssFinishBlocks, kMetricFinishBlocks, kFinishThreads = 16384, 4096, 256      # csrc/sot_mss.hip:747, :831, :435

Case = collections.namedtuple("Case", "id kernel cite unit n_fft hop samples clips route ends")
WAVEW_ENDS = STFT + " pick_forward_route: wavew serves the 64-clip calls (576 frames < 3072): another FFT"
SLOT_ENDS = STFT + " pick_backward_route: slot from spectrum, stft_mag_backward_spec_kernel<10>, serves the 64-clip calls (576 groups < 1024): another FFT"


def _clips_for(units_per_wg, units_per_clip, must_not_divide=True):
    def clips(cus):
        n = -(-(2 * cus * units_per_wg + 1) // units_per_clip)
        while must_not_divide and (n * units_per_clip) % units_per_wg == 0:
            n += 1
        return n
    return clips


# id, kernel, the launch line that caps its grid, the unit of work, n_fft, hop, samples, clips(CUs), route, ends ("bits" or the citation)
CASES = [
    Case("wave2_fwd", "stft_mag_forward_wave2_kernel", STFT + " launch_forward_wave2: capped_grid(frames / 16, 1)", "a workgroup's 16 frames", 2048, 512, 4096 + 77,
         _clips_for(kWave2Waves, 9), "fwd", WAVEW_ENDS),
    Case("wave2_bwd_hop256", "stft_mag_backward_spec_wave2_kernel<2>", STFT + " launch_backward_wave2<2>: capped_grid(groups / 8, 1)", "a workgroup's 8 groups of two frames", 2048, 256,
         4096 + 77, _clips_for(kBwdWave2Waves, 9), "bwd_spec", SLOT_ENDS),
    Case("wave2_bwd_hop512", "stft_mag_backward_spec_wave2_kernel<4>", STFT + " launch_backward_wave2<4>", "a workgroup's 8 groups of two frames", 2048, 512, 512 * 17 - 5,
         _clips_for(kBwdWave2Waves, 9), "bwd_spec", SLOT_ENDS),
    Case("clipw_bwd_4096", "stft_mag_backward_spec_clipw_kernel", STFT + " launch_backward_clip: capped_grid(batch, 1)", "a clip of 16 frames", 2048, 256, 4096, lambda cus: 2 * cus + 1,
         "bwd_spec", "bits"),
    Case("clipw_bwd_4001", "stft_mag_backward_spec_clipw_kernel", STFT + " launch_backward_clip", "a clip of 16 frames, the last two end-padded, odd length", 2048, 256, 4001,
         lambda cus: 2 * cus + 1, "bwd_spec", "bits"),
    Case("ola_grid_y_audio", "stft_overlap_add_kernel behind stft_mag_backward_partial_kernel<5>", STFT + " sot_stft_mag_backward_spec: overlap-add gridDim.y = min(batch, 65535); recomputing slot route", "a clip", 64, 16,
         100, lambda cus: kGridY + 2, "bwd_audio", "bits"),
    Case("ola_grid_y_spec", "stft_overlap_add_kernel behind stft_mag_backward_spec_kernel<5>", STFT + " sot_stft_mag_backward_spec: overlap-add gridDim.y; slot from spectrum", "a clip", 64, 16, 100, lambda cus: kGridY + 2,
         "bwd_spec", "bits"),
    Case("ola_grid_x", "stft_overlap_add_kernel", STFT + " sot_stft_mag_backward_spec: overlap-add gridDim.x = min(samples / 256, 64)", "256 samples of a clip", 512, 128, 2 * kOlaGridX * kThreads + 77,
         lambda cus: 3, "bwd_audio", "bits"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def cus():
    return rl.cus()


def ends_count(B):
    return max(1, min(cus(), 64, B - 1))


def frames_of(case):
    return -(-case.samples // case.hop)


def check_forcing(case, B):
    """the batch forces what the table says, from the CU count alone"""
    frames = frames_of(case)
    groups = (frames + 1) // 2
    if case.id == "wave2_fwd":
        wgs = -(-B * frames // kWave2Waves)
        assert B * frames >= 3072 and wgs >= 2 * cus() + 1 and (B * frames) % kWave2Waves != 0
    elif case.id.startswith("wave2_bwd"):
        wgs = -(-B * groups // kBwdWave2Waves)
        assert frames > 16 and B * groups >= 1024 and wgs >= 2 * cus() + 1 and (B * groups) % kBwdWave2Waves != 0
    elif case.id.startswith("clipw"):
        assert frames <= 16 and case.hop % 2 == 0 and B >= 64 and B >= 2 * cus() + 1
    elif case.id.startswith("ola_grid_y"):
        assert B > kGridY + 1 and case.n_fft != 2048
    elif case.id == "ola_grid_x":
        assert case.samples > 2 * kOlaGridX * kThreads and case.samples % kThreads != 0
    print(f"{case.id}: {cus()} CUs, {B} clips of {frames} frames ({case.unit})")


@functools.lru_cache(maxsize=None)
def stft_batch(name):
    case = BY_ID[name]
    nat, dev = native(), device()
    B = case.clips(cus())
    check_forcing(case, B)
    a, kinds = rk.make_clips(B, case.samples, 31 * case.hop + case.samples, case.n_fft, case.hop, dev)
    win = torch.hann_window(case.n_fft, device=dev)
    g = torch.Generator(device=dev).manual_seed(B)
    inp = dict(a=a, win=win, kinds=kinds, sample=rk.check_sample(B, kinds))
    if case.route != "fwd":
        frames, bins = frames_of(case), case.n_fft // 2 + 1
        inp["gm"] = torch.rand(B, frames, bins, generator=g, device=dev)
        inp["base"] = torch.rand(B, case.samples, generator=g, device=dev)
        inp["up"] = torch.full((1,), 0.37, device=dev)
        inp["spec"] = nat.stft_mag_forward(a, win, case.n_fft, case.hop, want_spec=True)[1] if case.route == "bwd_spec" else None
    torch.cuda.synchronize()
    return inp


ROW_KEYS = ("a", "gm", "base", "spec")


def map_rows(inp, f):
    return {k: (f(v) if k in ROW_KEYS and v is not None else v) for k, v in inp.items()}


def run_stft(nat, case, inp, accumulate=True):
    if case.route == "fwd":
        return nat.stft_mag_forward(inp["a"], inp["win"], case.n_fft, case.hop, want_spec=True)
    return (nat.stft_mag_backward(inp["a"], inp["win"], case.n_fft, case.hop, inp["gm"], grad_scale=inp["up"],
                                  accumulate_into=inp["base"].clone() if accumulate else None, spec=inp["spec"]),)


def stft_reference(a, win, n_fft, hop, gm, up, dtype):
    """torch.stft -> abs in `dtype` and, with gm, autograd's gradient of sum(mag * gm) * up: (mag, spectrum, gradient or None)"""
    from sot_amd import spectra
    x = a.to(dtype).clone().requires_grad_(gm is not None)
    X = torch.stft(spectra.end_padded(x, n_fft, hop), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=win.to(dtype), center=False, normalized=True,
                   return_complex=True).permute(0, 2, 1)
    mag = X.abs()
    if gm is None:
        return mag.detach(), X.detach(), None
    (mag * gm.to(dtype)).sum().backward()
    return mag.detach(), X.detach(), x.grad * float(up)


def err3(got, truth):
    """tests/test_stft_producer.py: _err -- max, median, rms of the error, of the truth's peak"""
    from test_stft_producer import _err
    return _err(got, truth)


@pytest.mark.parametrize("name", [c.id for c in CASES])
def test_stft_loops(name):
    nat, case = native(), BY_ID[name]
    inp = stft_batch(name)
    B = inp["a"].shape[0]
    base = run_stft(nat, case, inp)
    assert all(bool(torch.isfinite(t).all()) for t in base)
    # 1. roll invariance
    for shift in (1, B // 2 + 1):
        again = run_stft(nat, case, map_rows(inp, lambda t: torch.roll(t, shift, 0)))
        rl.assert_rows_equal(case, f"rolled by {shift}", [torch.roll(t, -shift, 0) for t in again], base)
    # 2. the ends alone
    c = ends_count(B)
    peaks = [float(t.abs().max()) for t in base]
    for lo, hi in ((0, c), (B - c, B)):
        alone = run_stft(nat, case, map_rows(inp, lambda t: t[lo:hi].clone()))
        if case.ends == "bits":
            rl.assert_rows_equal(case, f"clips [{lo}, {hi}) alone", alone, [t[lo:hi] for t in base], lo)
        else:
            bound = 1e-6 if case.route == "fwd" else 2e-5
            for k, (x, y, peak) in enumerate(zip(alone, base, peaks)):
                kinds = inp["kinds"][lo:hi]
                worst = 0.0
                for kind in range(len(rk.CLIP_KINDS)):      # each kind against the peak of its own clips in the big call
                    at = torch.nonzero(kinds == kind).flatten()
                    if at.numel():
                        pk = float(y[lo:hi][at].abs().max())
                        d = float((x[at] - y[lo:hi][at]).abs().max())
                        lim = 1e-5 if case.route == "fwd" and rk.CLIP_KINDS[kind] == "tiny" else bound      # the careful |.| path: the existing test's `rel5`
                        assert d == 0.0 if pk == 0.0 else d <= lim * pk, (case.id, lo, k, rk.CLIP_KINDS[kind], d, pk)
                        worst = max(worst, d / pk if pk else 0.0)
                print(f"{case.id}: clips [{lo}, {hi}) alone, output {k}: worst difference {worst:.2e} of the kind's peak (bound {bound:.0e}; {case.ends})")
    # 3. float64 on the check sample
    s = inp["sample"].to(device())
    kinds = inp["kinds"][s].tolist()
    if case.route == "fwd":
        mag64, X64, _ = stft_reference(inp["a"][s].cpu(), inp["win"].cpu(), case.n_fft, case.hop, None, None, torch.float64)
        X64 = X64 * float(case.n_fft) ** 0.5              # the stored spectrum is the transform itself; the magnitudes carry normalized=True's n_fft^-0.5
        got_mag, got_spec = base[0][s].cpu().double(), torch.view_as_complex(base[1][s].cpu().double().contiguous())
        worst = {}
        for i, kind in enumerate(kinds):
            name_k, peak = rk.CLIP_KINDS[kind], float(mag64[i].max())
            if peak == 0.0:
                assert float(got_mag[i].abs().max()) == 0.0 and float(got_spec[i].abs().max()) == 0.0
                continue
            e_mag, e_spec = float((got_mag[i] - mag64[i]).abs().max()) / peak, float((got_spec[i] - X64[i]).abs().max()) / float(X64[i].abs().max())
            was = worst.get(name_k, (0.0, 0.0))
            worst[name_k] = (max(was[0], e_mag), max(was[1], e_spec))
            assert e_mag <= (1e-5 if name_k == "tiny" else 2e-6) and e_spec <= 2e-5, (case.id, int(s[i]), name_k, e_mag, e_spec)
        print(f"{case.id}: {len(kinds)} sample clips against torch.stft in float64, worst (mag, spec) error of the clip's peak per kind: "
              + ", ".join(f"{k} {v[0]:.2e} {v[1]:.2e}" for k, v in worst.items()))
    else:
        plain = run_stft(nat, case, inp, accumulate=False)[0]
        assert torch.equal(base[0], inp["base"] + plain), "accumulate = 1 is one float32 addition onto the base"
        sub = map_rows(inp, lambda t: t[s].cpu())       # both references on the CPU: torch.stft and autograd in float64 and in float32
        _, _, g64 = stft_reference(sub["a"], inp["win"].cpu(), case.n_fft, case.hop, sub["gm"], inp["up"], torch.float64)
        _, _, g32 = stft_reference(sub["a"], inp["win"].cpu(), case.n_fft, case.hop, sub["gm"], inp["up"], torch.float32)
        got = plain[s].cpu()
        worst = {}
        for i, kind in enumerate(kinds):
            name_k = rk.CLIP_KINDS[kind]
            if float(g64[i].abs().max()) == 0.0:
                assert float(got[i].abs().max()) == 0.0, (case.id, int(s[i]), name_k)
                continue
            ours, ref = err3(got[i].numpy(), g64[i].numpy()), err3(g32[i].numpy(), g64[i].numpy())
            was = worst.get(name_k, ((0.0,) * 3, (0.0,) * 3))
            worst[name_k] = (ours, ref) if ours[0] >= was[0][0] else was
            for o, r, what, floor in zip(ours, ref, ("max", "median", "rms"), (1.5e-5, 1e-6, 1e-6)):
                assert o <= 1.5 * r + floor, (case.id, int(s[i]), name_k, what, o, r)
        print(f"{case.id}: {len(kinds)} sample clips against float64 autograd, per kind the clip with the largest HIP error (max over the clip, of its gradient's peak), HIP | torch float32 on that clip: "
              + ", ".join(f"{k} {v[0][0]:.2e} | {v[1][0]:.2e}" for k, v in worst.items()))


# ---- the synthesiser's envelopes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,frames,samples,k,what", [
    (kGridY + 2, 1, 2, 1, OSC + ":633 gridDim.y = min(batch, 65535): the smallest frames, samples and sinusoid count sot_synth_envelopes_forward accepts"),
    (2, 16, 4096, 257, OSC + ":631-633 gridDim.x = min(samples K / 256, 4096 / batch) = 2048 workgroups: 4096 * 257 elements are two rounds and 4096 elements more"),
], ids=["grid_y", "grid_x"])
def test_synth_envelopes_loops(batch, frames, samples, k, what):
    """synth_envelopes_forward_kernel: b += gridDim.y and e += gridDim.x * 256.  Roll invariance, the ends alone, and the bits of the float64-exact model."""
    import synth_model as sm
    nat, dev = native(), device()
    if frames > 1:
        assert samples * k > 2 * (256 * 16 // batch) * kThreads and (samples * k) % kThreads == 0 and (samples * k // kThreads) % (256 * 16 // batch) != 0
    amp_np, freq_np = sm.control_inputs(batch + k, batch, frames, k, False)
    amp, freq = torch.from_numpy(np.ascontiguousarray(amp_np)).to(dev), torch.from_numpy(np.ascontiguousarray(freq_np)).to(dev)
    kind = rk.clip_kind_ids(batch, dev)                      # clips of unlike nature: silent, above Nyquist (amplitude gated to 0), tiny, huge
    amp = torch.where((kind == 3)[:, None, None], torch.zeros_like(amp), amp) * torch.where(kind == 4, 1e-21, 1.0)[:, None, None].float() \
        * torch.where(kind == 5, 1e6, 1.0)[:, None, None].float()
    freq = torch.where((kind == 2)[:, None, None], torch.full_like(freq, 9000.0), freq)
    window = torch.hann_window(2 * samples // frames, device=dev)
    base = nat.synth_envelopes_forward(amp, freq, window, samples, sm.SR, False)
    case = collections.namedtuple("C", "id")(f"envelopes {batch}x{samples}x{k}")
    for shift in (1, batch // 2 + 1):
        again = nat.synth_envelopes_forward(torch.roll(amp, shift, 0), torch.roll(freq, shift, 0), window, samples, sm.SR, False)
        rl.assert_rows_equal(case, f"rolled by {shift}", [torch.roll(t, -shift, 0) for t in again], base)
    c = ends_count(batch)
    for lo, hi in ((0, c), (batch - c, batch)):
        alone = nat.synth_envelopes_forward(amp[lo:hi].clone(), freq[lo:hi].clone(), window, samples, sm.SR, False)
        rl.assert_rows_equal(case, f"clips [{lo}, {hi}) alone", alone, [t[lo:hi] for t in base], lo)
    s = rk.check_sample(batch, kind)
    wa, wf = sm.envelopes(amp[s.to(dev)].cpu().numpy(), freq[s.to(dev)].cpu().numpy(), window.cpu().numpy(), samples, sm.SR, False)
    assert np.array_equal(base[0][s.to(dev)].cpu().numpy(), wa) and np.array_equal(base[1][s.to(dev)].cpu().numpy(), wf), what


# ---- spectral distances ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def magnitudes(count):
    """two flat magnitude arrays whose elements are of unlike nature by a hash of the index: plain, exactly tied, below eps, zero, 1e6"""
    dev = device()
    g = torch.Generator(device=dev).manual_seed(count)
    t, v = torch.rand(count, generator=g, device=dev) * 2, torch.rand(count, generator=g, device=dev) * 2
    kind = (rk.row_hash(torch.arange(count, dtype=torch.int64, device=dev), 0xD157) >> 5) % 16
    v = torch.where(kind == 0, t, v)                                   # |t - v| = 0: sgn(0) = 0
    t = torch.where(kind == 1, torch.full_like(t, 1e-7), t)            # below eps: no gradient through the logarithm
    v = torch.where(kind == 2, torch.zeros_like(v), v)
    t, v = torch.where(kind == 3, t * 1e6, t), torch.where(kind == 3, v * 1e6, v)
    return t.contiguous(), v.contiguous()


def distance64(t, v, mw, lw, l2, rows=None):
    tt, vv = t.double().clone().requires_grad_(True), v.double().clone().requires_grad_(True)
    e = torch.tensor(float(np.float32(1e-5)), dtype=torch.float64, device=t.device)
    sl = lambda x: torch.log(torch.where(x <= e, e, x))      # noqa: E731
    D = (lambda d: d ** 2) if l2 else torch.abs
    if rows is None:
        return mw * D(tt - vv).mean() + lw * D(sl(tt) - sl(vv)).mean(), tt, vv
    return mw * D(tt - vv).reshape(rows, -1).mean(1) + lw * D(sl(tt) - sl(vv)).reshape(rows, -1).mean(1), tt, vv


@pytest.mark.parametrize("mw,lw,l2", [(0.5, 2.0, False), (0.3, 0.7, True)], ids=["l1", "l2"])
def test_spec_distance_forward_loop(mw, lw, l2):
    """spec_distance_partial_kernel: i += gridDim.x * 256 on kDistBlocks = 1024 workgroups (csrc/sot_spec_distance.hip sot_spec_distance_forward): 2 * 1024 * 256 + 1 elements are two full
    rounds and one element of a third.  The sum's order depends on the element index, so a rolled batch is another sum: in place of the
    roll, the call is repeated (deterministic), accumulates onto a base by one float32 addition, and meets float64 within 2e-6."""
    nat = native()
    count = 2 * kDistBlocks * kThreads + 1
    t, v = magnitudes(count)
    got = nat.spec_distance_forward(t, v, mw, lw, 1e-5, l2)
    assert torch.equal(got, nat.spec_distance_forward(t, v, mw, lw, 1e-5, l2))
    base = torch.tensor(0.625, device=device())
    assert torch.equal(nat.spec_distance_forward(t, v, mw, lw, 1e-5, l2, accumulate_into=base.clone()), base + got)
    want = float(distance64(t, v, mw, lw, l2)[0].detach())
    print(f"spec_distance_forward {count}: relative error against float64 {abs(float(got) - want) / abs(want):.2e}")
    assert abs(float(got) - want) <= 2e-6 * abs(want)
    # the last, one-element round counts: without element count - 1 the float64 sum moves by more than the tolerance leaves room for
    t2 = t.clone()
    t2[-1] = 3e7 + v[-1]
    moved = float(nat.spec_distance_forward(t2, v, mw, lw, 1e-5, l2))
    want2 = float(distance64(t2, v, mw, lw, l2)[0].detach())
    assert abs(want2 - want) > 1e-4 * abs(want) and abs(moved - want2) <= 2e-6 * abs(want2)


@pytest.mark.parametrize("per_row", [False, True], ids=["flat", "rows"])
@pytest.mark.parametrize("mw,lw,l2", [(0.5, 2.0, False), (0.3, 0.7, True)], ids=["l1", "l2"])
def test_spec_distance_backward_loops(mw, lw, l2, per_row):
    """spec_distance_backward_kernel / spec_distance_rows_backward_kernel: grid stride on 8192 workgroups (csrc/sot_spec_distance.hip grad_grid: kGradBlocks): 2 * 8192 * 256 + 1
    elements (rows: 5 rows of 838861).  Elementwise, so a roll of the elements rolls the gradients: bit for bit; the ends alone cannot be bit-equal
    (the mean's 1 / count is another), they are covered by float64: 1e-5 of the gradient's peak."""
    nat, dev = native(), device()
    count = 2 * kDistBwdBlocks * kThreads + 1
    rows = 5
    assert count % rows == 0
    t, v = magnitudes(count)
    up = torch.linspace(0.5, 1.5, rows, device=dev) if per_row else torch.full((1,), 1.5, device=dev)

    def call(t_, v_):
        shape = (rows, count // rows) if per_row else (count,)
        return nat.spec_distance_backward(t_.reshape(shape), v_.reshape(shape), mw, lw, up, 2.0, 1e-5, l2, need_target=True, need_value=True, per_row=per_row)
    base = call(t, v)
    # a roll inside the rows keeps every element's row, hence its upstream factor: roll the [rows, count / rows] view along dim 1
    roll = (lambda x, s: torch.roll(x.reshape(rows, -1), s, 1).reshape(-1)) if per_row else (lambda x, s: torch.roll(x, s, 0))
    for shift in (1, count // (2 * rows) + 1):
        again = call(roll(t, shift).contiguous(), roll(v, shift).contiguous())
        for a, b in zip(again, base):
            assert torch.equal(roll(a.reshape(-1), -shift), b.reshape(-1)), (shift, "rolled elements give other gradients")
    val, tt, vv = distance64(t, v, mw, lw, l2, rows if per_row else None)
    (val * up.double() * 2.0).sum().backward()
    for which, got, want in (("target", base[0], tt.grad), ("value", base[1], vv.grad)):
        worst = float((got.reshape(-1).double() - want).abs().max() / want.abs().max())
        print(f"spec_distance_backward per_row={per_row} {which}: worst error {worst:.2e} of the gradient's peak")
        assert worst <= 1e-5


# ---- the fused multi-scale loss and the metrics, one value per clip --------------------------------------------------------------------------
MSS_SIZES = (64, 512)


def mss_windows(sizes):
    return [torch.hann_window(s, device=device()) for s in sizes]


def test_mss_per_clip_gather_loop():
    """mss_finish_kernel (csrc/sot_mss.hip:748): at most 16384 workgroups, each taking two (clip, 256 packed points) blocks per iteration with
    blk += 2 * gridDim.x: a round is 32768 blocks.  3000-sample clips have 6 blocks; 10923 clips are two rounds and two blocks more.  per_clip = 1:
    the loss of a clip is a thread's loop over its tasks."""
    import test_mss_fused as mf
    nat, dev = native(), device()
    samples = 3000
    ranges = ((samples + 1) // 2 + 255) // 256
    B = -(-(2 * 2 * kMssFinishBlocks + 1) // ranges)
    assert B * ranges > 2 * 2 * kMssFinishBlocks and (B * ranges + 1) // 2 > kMssFinishBlocks
    x, _ = rk.make_clips(B, samples, 5, 512, 128, dev)
    noise, kinds = rk.make_clips(B, samples, 6, 512, 128, dev, salt=0x7E57)
    y = (x + 0.3 * noise).contiguous()           # an estimate near its target, its perturbation of another kind
    wins = mss_windows(MSS_SIZES)

    def call(x_, y_):
        return nat.mss_loss_and_grad(x_, y_, MSS_SIZES, wins, 1.0, 1.0, 1e-5, False, True, True, 0.5)
    base = call(x, y)
    assert base[0].shape == (B,) and all(bool(torch.isfinite(t).all()) for t in base)
    case = collections.namedtuple("C", "id")("mss per clip")
    for shift in (1, B // 2 + 1):
        again = call(torch.roll(x, shift, 0), torch.roll(y, shift, 0))
        rl.assert_rows_equal(case, f"rolled by {shift}", [torch.roll(t, -shift, 0) for t in again], base)
    c = ends_count(B)
    for lo, hi in ((0, c), (B - c, B)):
        rl.assert_rows_equal(case, f"clips [{lo}, {hi}) alone", call(x[lo:hi].clone(), y[lo:hi].clone()), [t[lo:hi] for t in base], lo)
    s = rk.check_sample(B, kinds, rk.clip_kind_ids(B))
    xs, ys = x[s.to(dev)].cpu(), y[s.to(dev)].cpu()
    mod = collections.namedtuple("M", "fft_sizes loss_type mag_weight logmag_weight")(MSS_SIZES, "L1", 1.0, 1.0)
    ones = torch.ones(len(s))
    want64, g64 = mf._reference(mod, xs, ys, (1, 2), ones)
    want32, g32 = mf._reference(mod, xs, ys, (1, 2), ones, torch.float32)
    got_l, got_g = base[0][s.to(dev)].cpu().double() / 0.5, base[1][s.to(dev)].cpu().double() / 0.5      # post_scale: a power of two
    # tests/test_mss_fused.py: _check, applied to the sample in two batches -- the clips that hold a 1e6 signal and the rest -- so that the first do not
    # hide the second behind the batch's peak
    huge = rk.CLIP_KINDS.index("huge")
    is_huge = (rk.clip_kind_ids(B)[s] == huge) | (kinds.cpu()[s] == huge)
    for label, at in (("clips with a 1e6 signal", torch.nonzero(is_huge).flatten()), ("the other clips", torch.nonzero(~is_huge).flatten())):
        assert at.numel() >= 4, label
        w64, gl, g, r64, r32 = want64[at], got_l[at], got_g[at], g64[at], g32[at].double()
        err = float((gl - w64).abs().max() / w64.abs().max())
        ref_err, hip_err = float(torch.linalg.norm(r32 - r64) / torch.linalg.norm(r64)), float(torch.linalg.norm(g - r64) / torch.linalg.norm(r64))
        med_hip, med_ref = float((g - r64).abs().median() / r64.abs().max()), float((r32 - r64).abs().median() / r64.abs().max())
        print(f"mss per clip, {label} ({at.numel()} of the sample): loss error {err:.2e} (float32 reference {float((want32[at].double() - w64).abs().max() / w64.abs().max()):.2e}), "
              f"gradient norm error HIP {hip_err:.2e} | float32 reference {ref_err:.2e}, median {med_hip:.2e} | {med_ref:.2e}")
        assert err <= 1e-5, (label, err)
        assert hip_err <= 1.5 * ref_err + 5e-6, (label, hip_err, ref_err)
        assert med_hip <= 1.5 * med_ref + 1e-8, (label, med_hip, med_ref)


def test_metrics_per_clip_finish_loop():
    """metric_finish_kernel (csrc/sot_mss.hip:831-832): per_clip = 1 runs min(batch / 256, 4096) workgroups, one thread per clip with
    o += gridDim.x * 256: a round is 1048576 clips; 2 * 1048576 + 1 clips of 100 samples (n_fft 64: 7 frames, the last three end-padded)."""
    import test_eval_metrics_gpu as em
    from sot_amd import metrics
    nat, dev = native(), device()
    samples, sizes = 100, (64,)
    B = 2 * kMetricFinishBlocks * kFinishThreads + 1
    kw = dict(fft_sizes=[64], mag_weight=1.0, logmag_weight=0.5, log_spectral_distance_weight=0.25, loss_type="L2")
    groups = [em._group(kw)]
    x, _ = rk.make_clips(B, samples, 7, 64, 16, dev)
    noise, kinds = rk.make_clips(B, samples, 8, 64, 16, dev, salt=0x7E57)
    y = (x + 0.3 * noise).contiguous()
    wins = mss_windows(sizes)

    def call(x_, y_):
        return (nat.spec_metrics(x_, y_, sizes, wins, groups, 1e-5, True)[0],)
    base = call(x, y)
    assert base[0].shape == (B,) and bool(torch.isfinite(base[0]).all())
    case = collections.namedtuple("C", "id")("metrics per clip")
    for shift in (1, B // 2 + 1):
        again = call(torch.roll(x, shift, 0), torch.roll(y, shift, 0))
        rl.assert_rows_equal(case, f"rolled by {shift}", [torch.roll(t, -shift, 0) for t in again], base)
    c = ends_count(B)
    for lo, hi in ((0, c), (B - c, B)):
        rl.assert_rows_equal(case, f"clips [{lo}, {hi}) alone", call(x[lo:hi].clone(), y[lo:hi].clone()), [t[lo:hi] for t in base], lo)
    s = rk.check_sample(B, kinds, rk.clip_kind_ids(B))
    xs, ys = x[s.to(dev)].cpu(), y[s.to(dev)].cpu()
    ref32 = metrics.ms_spectral_distance(xs, ys, per_clip=True, **kw)
    em._accuracy("signal loops / per_clip", base[0][s.to(dev)], ref32, xs, ys, kw, per_clip=True)


def test_what_no_batch_can_reach():
    """the arithmetic of the module docstring's NOT REACHABLE list, on this device's CU count"""
    n = cus()
    wavew_round, wavew_largest = 3 * n * kFwdwWaves, 3072 - 1
    assert wavew_round >= wavew_largest, f"{n} CUs: a batch of {wavew_round + 1} ... 3071 frames gives stft_mag_forward_wavew_kernel a second round: add the case"
    persistent_resident, persistent_largest = 6 * n, 512 - 1
    assert persistent_resident >= persistent_largest, f"{n} CUs: stft_mag_forward_persistent_kernel can run a second round: add the case"
