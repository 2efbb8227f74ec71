"""Randomised sweep of the synthesiser kernels (csrc/sot_osc.hip) on the GPU box against the float64 model of tests/synth_model.py, with
its per-element bounds: sinusoid count (log-uniform 1 ... 512), clip length (1 ... 6000, half of the draws within 9 samples of a multiple
of the case's segment length), batch 1 ... 4, entry point (oscillator bank / envelope kernels / one-piece synthesiser with random frames,
hop and harmonic), signal kind (random, constant, chirp through Nyquist, all muted, zero amplitudes) and which gradients are asked for.
    python tools/fuzz_synth.py [seconds=60] [seed=0]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import synth_model as sm
from sot_amd import _native as nat

SR = sm.SR
MAX_ELEMENTS = 1_000_000      # envelope elements per case: keeps the numpy model fast
KINDS = ("random", "constant", "chirp", "muted", "zero_amp")
STATS = {}                    # of the last run(): worst share of phase-tie elements in one input, elements and ties in all


def segment_of(lib, batch, k):
    return 512 * batch * k * 16 // int(lib.sot_oscillator_bank_workspace_bytes(batch, 512, k))


def frequencies(rng, kind, shape):
    """[batch, steps, K] float32 (steps: samples, or frames)."""
    batch, steps, k = shape
    if kind == "constant":
        f = np.broadcast_to(30.0 + 7900.0 * rng.random((batch, 1, k)), shape)
    elif kind == "chirp":
        f = np.linspace(6000.0, 9500.0, steps)[None, :, None] + 500.0 * rng.random((batch, 1, k))
    elif kind == "muted":
        f = 8000.0 + 4000.0 * rng.random(shape)
        f[rng.random(shape) < 0.1] = 8000.0
    else:
        f = 30.0 + 9000.0 * rng.random(shape)
    return np.ascontiguousarray(f, dtype=np.float32)


def draw_case(rng, lib):
    """One case description (everything but the arrays, which draw_arrays makes from its seed)."""
    k = int(min(512, max(1, round(float(np.exp(rng.uniform(0.0, np.log(512.0))))))))
    batch = int(rng.integers(1, 5))
    s = segment_of(lib, batch, k)
    most = max(1, min(6000, MAX_ELEMENTS // (batch * k)))
    if rng.random() < 0.5:
        samples = int(rng.integers(0, most // s + 2)) * s + int(rng.integers(-9, 10))
    else:
        samples = int(rng.integers(1, most + 1))
    samples = min(max(samples, 1), most)
    entry = str(rng.choice(["bank", "envelopes", "synth"]))
    frames = harmonic = None
    if entry != "bank":
        divisors = [d for d in range(1, samples // 2 + 1) if samples % d == 0]
        if not divisors:
            entry = "bank"                                            # one sample: no upsampling exists
        else:
            frames, harmonic = int(rng.choice(divisors)), bool(rng.random() < 0.5)
    need = [(True, True), (True, False), (False, True)][int(rng.integers(0, 3))]
    return dict(seed=int(rng.integers(0, 2 ** 31 - 1)), entry=entry, kind=str(rng.choice(KINDS)), batch=batch, samples=samples, k=k, segment=s,
                frames=frames, harmonic=harmonic, need_freq=need[0], need_amp=need[1])


def draw_arrays(c):
    rng = np.random.default_rng(c["seed"])
    batch, samples, k = c["batch"], c["samples"], c["k"]
    steps = samples if c["entry"] == "bank" else c["frames"]
    freq = frequencies(rng, c["kind"], (batch, steps, k))
    if c["entry"] != "bank" and c["harmonic"]:
        # f0 from the last column: the top partial lies around Nyquist -- except "muted", where f0 itself is at or above it (every partial muted)
        freq = np.ascontiguousarray(freq[:, :, -1:] / np.float32(1.0 if c["kind"] == "muted" else max(k, 2) * 0.75))
    amp = np.zeros((batch, steps, k), np.float32) if c["kind"] == "zero_amp" else rng.random((batch, steps, k)).astype(np.float32)
    grad = rng.standard_normal((batch, samples)).astype(np.float32)
    env_grads = None
    if c["entry"] == "envelopes":
        env_grads = (rng.standard_normal((batch, samples, k)).astype(np.float32), rng.standard_normal((batch, samples, k)).astype(np.float32))
    return freq, amp, grad, env_grads


def model_of(c, arrays):
    """The model's forward for a case: (forward namespace or None, window or None)."""
    freq, amp, _, _ = arrays
    if c["entry"] == "bank":
        return sm.oscillator_bank(freq, amp, SR), None
    hann = torch.hann_window(2 * (c["samples"] // c["frames"])).numpy()
    if c["entry"] == "synth":
        return sm.synth(amp, freq, hann, c["samples"], SR, c["harmonic"]), hann
    return None, hann


def check_case(c, arrays, m, hann, dev):
    """{name: error / bound} of one case on the GPU."""
    freq, amp, grad, env_grads = arrays
    on = lambda a: torch.from_numpy(a).to(dev)
    nf, na = c["need_freq"], c["need_amp"]
    out = {}
    if c["entry"] == "bank":
        f, a, g = on(freq), on(amp), on(grad)
        audio, ws = nat.oscillator_bank_forward(f, a, SR, return_workspace=True)
        out["audio"] = sm.ratio(audio.cpu().numpy() - m.audio, sm.audio_bound(m, c["k"]))
        b = sm.oscillator_bank_backward(freq, amp, SR, grad, fwd=m)
        gf, ga = nat.oscillator_bank_backward(f, a, SR, g, need_freq=nf, need_amp=na, forward_workspace=ws if c["seed"] % 2 else None)
        if na:
            out["grad_amp"] = sm.grad_amp_ratio(ga.cpu().numpy(), b)
            out["grad_amp_muted"] = 0.0 if np.all(ga.cpu().numpy()[m.muted] == 0.0) else float("inf")
        if nf:
            out["grad_freq"] = sm.ratio(gf.cpu().numpy() - b.grad_freq, sm.grad_freq_bound(b))
        return out
    a, f, w = on(amp), on(freq), on(hann)
    samples, harmonic = c["samples"], c["harmonic"]
    if c["entry"] == "envelopes":
        want_a, want_f = sm.envelopes(amp, freq, hann, samples, SR, harmonic)
        got_a, got_f = nat.synth_envelopes_forward(a, f, w, samples, SR, harmonic)
        out["amp_env_bits"] = 0.0 if np.array_equal(got_a.cpu().numpy(), want_a) else float("inf")
        out["freq_env_bits"] = 0.0 if np.array_equal(got_f.cpu().numpy(), want_f) else float("inf")
        b = sm.envelopes_backward(amp, freq, hann, samples, SR, harmonic, env_grads[0] if na else None, env_grads[1] if nf else None)
        ga, gf = nat.synth_envelopes_backward(a, f, w, samples, SR, harmonic, on(env_grads[0]) if na else None, on(env_grads[1]) if nf else None,
                                              need_amp=na, need_freq=nf)
        if na:
            out["grad_amp_frames"] = sm.ratio(ga.cpu().numpy() - b.grad_amp, b.amp_bound)
        if nf:
            out["grad_freq_frames"] = sm.ratio(gf.cpu().numpy() - b.grad_freq, b.freq_bound)
        return out
    g = on(grad)
    audio, ws = nat.synth_forward(a, f, w, samples, SR, harmonic, for_backward=True)
    out["audio"] = sm.ratio(audio.cpu().numpy() - m.audio, sm.audio_bound(m, c["k"]))
    b = sm.synth_backward(amp, freq, hann, samples, SR, harmonic, grad, fwd=m)
    ga, gf = nat.synth_backward(a, f, w, samples, SR, harmonic, g, need_amp=na, need_freq=nf, forward_workspace=ws if c["seed"] % 2 else None)
    if na:
        out["grad_amp_frames"] = sm.ratio(ga.cpu().numpy() - b.grad_amp, b.amp_bound)
    if nf:
        out["grad_freq_frames"] = sm.ratio(gf.cpu().numpy() - b.grad_freq, b.freq_bound)
    return out


def run(budget=60.0, seed0=0, max_cases=None, verbose=True, gpu=True):
    """(cases, failures, worst_ratio): worst_ratio is the largest error / bound over every element of every case; a failure record is
    (what, case, ratios).  gpu=False only draws the cases and counts their phase ties (STATS) -- runs anywhere."""
    lib = nat.load(build_if_missing=False)
    dev = torch.device("cuda:0") if gpu else None
    rng = np.random.default_rng(seed0)
    failures, cases, worst = [], 0, 0.0
    STATS.update(worst_tie_share=0.0, elements=0, ties=0, entries={}, segments=set())
    t_end = time.time() + budget
    while time.time() < t_end and (max_cases is None or cases < max_cases):
        c = draw_case(rng, lib)
        arrays = draw_arrays(c)
        m, hann = model_of(c, arrays)
        cases += 1
        STATS["entries"][c["entry"]] = STATS["entries"].get(c["entry"], 0) + 1
        STATS["segments"].add(c["segment"])
        if m is not None:
            share = float(m.ties.mean())
            STATS.update(worst_tie_share=max(STATS["worst_tie_share"], share), elements=STATS["elements"] + m.ties.size,
                         ties=STATS["ties"] + int(m.ties.sum()))
            if share > sm.TIE_SHARE:
                failures.append(("TIES", c, share))
                verbose and print("TIES", c, share)
        if not gpu:
            continue
        ratios = check_case(c, arrays, m, hann, dev)
        top = max(ratios.values())
        worst = max(worst, top)
        if not top <= 1.0:
            failures.append(("SYNTH", c, ratios))
            verbose and print("SYNTH", c, ratios)
    if verbose:
        print(f"cases {cases} {STATS['entries']}, segment lengths {sorted(STATS['segments'])}, outside their bounds {len(failures)}, "
              f"worst error / bound {worst:.3f}, phase ties {STATS['ties']} of {STATS['elements']} elements (worst share {STATS['worst_tie_share']:.2g})")
    return cases, failures, worst


if __name__ == "__main__":
    run(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 0)
