// sot_stft.hip -- MI355X (gfx950): the producer in front of the SOT loss, the magnitude STFT of the reference's
// `features.TorchSTFT` (features.py:85-113 -> compute_mag / stft, features.py:191-237; end padding utils.pad_for_stft,
// utils.py:252-275): torch.stft(center=False, normalized=True, onesided) of the end-padded signal, |.|, frames-major
// output [batch, frames, n_fft/2 + 1], and its closed-form backward.  SURVEY §8f row 1.
//
// This file is the HOST side: argument checks, the route table, one launcher per route, the C ABI.  The kernels:
//   sot_stft_common.hpp  StftArgs, Geo, the committed tables, the three-rounding complex helpers, clip_row, spec_row, unpack_pair, |.|
//   sot_stft_slot.hpp    slot family, every n_fft: stft_mag_forward_kernel, ..._forward_persistent_kernel,
//                        ..._backward_partial_kernel, ..._backward_spec_kernel, stft_overlap_add_kernel
//   sot_stft_wave2.hpp   in-place one-wavefront family, n_fft 2048: ..._forward_wave2_kernel, ..._backward_spec_wave2_kernel<QS>
//   sot_stft_wfft.hpp    on csrc/sot_wave_fft.hpp, n_fft 2048: ..._forward_wavew_kernel, ..._backward_spec_clipw_kernel
// (The spectral distance of MSSLoss over these magnitudes is an object of its own: csrc/sot_spec_distance.hip.)
//
// Routes (pick_forward_route / pick_backward_route below; T = frames of the whole call, both signals of a pair counted):
//   forward   n_fft 2048, 512 <= T < 3072      wavew                 backward  spectrum, n_fft 2048, <= 16 frames per clip, hop even,
//             n_fft 2048, T >= 3072            wave2                             batch >= 64                              clip (no overlap-add)
//             n_fft 2048                       persistent slot                 spectrum, n_fft 2048, batch x groups >= 1024, hop 256 / 512,
//             else                             slot                              scratch 8-byte aligned, span even        wave2 from spectrum
//                                                                              spectrum                                   slot from spectrum
//                                                                              else                                       recomputing slot
// The routes are different factorisations of one transform and agree to a few ulp, not bit for bit: tests/test_stft_routes_gpu.py
// pins every boundary.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sot_host.hpp"
#include "sot_stft_slot.hpp"
#include "sot_stft_wave2.hpp"
#include "sot_stft_wfft.hpp"

namespace sot_stft {

static int ilog2_exact(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return ((1 << l) == v) ? l : -1;
}

static int fill_args(const float* audio, int64_t batch, int64_t samples, int64_t row_stride, const float* window, int n_fft, int hop,
                     StftArgs* a)
{
    if (batch < 0 || samples < 1 || hop < 1 || row_stride < samples) return SOT_ERR_BAD_SHAPE;
    const int logn = ilog2_exact(n_fft);
    if (logn < 6 || n_fft > kMaxFft) return SOT_ERR_UNSUPPORTED_SIZE;  // 64 ... 4096, powers of two
    if (batch > 0 && (audio == nullptr || window == nullptr)) return SOT_ERR_NULL_POINTER;
    if (reinterpret_cast<uintptr_t>(window) % 8 != 0) return SOT_ERR_BAD_SHAPE;   // the kernels read the window two taps at a time
    a->audio = audio; a->batch = batch; a->samples = samples; a->row_stride = row_stride;
    a->window = window; a->n_fft = n_fft; a->logm = logn - 1; a->hop = hop;
    a->frames = (samples + hop - 1) / hop;  // utils.py:265: -(-signal_len // hop_length)
    if (batch * a->frames > 0x7fffffffLL) return SOT_ERR_UNSUPPORTED_SIZE;
    return SOT_OK;
}

// ---- the route table: which kernel serves a call.  Every predicate stands here, once. ------------------------------------------------
// kFwdWavewMinFrames: below it the slot kernels (a frame is a dependent chain on one wave: small batches want the frame spread over four).
constexpr int64_t kFwdWavewMinFrames = 512;
// kWave2MinFrames: from here the round-4 one-wavefront-per-frame kernel, one 1024-thread workgroup per CU (it keeps the larger batches from
// the round-5 wavew kernel: its results on BASELINE config 5 are what the cutoff mode's knife-edge statistics were taken with).
// Measured (round 4, tools/r4/stft_sizes.py, forward of a pair, n_fft 2048 / hop 256, us per call, slot kernel | this kernel;
// profiles/r4j_stft_wave2.txt): 512 frames 10.6 | 15.0, 1024: 10.6 | 15.3, 2048: 14.4 | 16.1, 4096: 21.6 | 17.3, 8192 (config 5): 37.3 | 28.5,
// 16384: 64.0 | 48.0 -- a frame is a 28 000-clock dependent chain on one wave (~15 us), so the kernel needs at least one frame per
// wave slot of the chip (256 CUs x 16) to pay: from 3072 frames.
constexpr int64_t kWave2MinFrames = 3072;
constexpr int64_t kBwdWave2MinGroups = 1024;   // frame groups of the whole call from which the wave2 backward serves it
constexpr int64_t kBwdClipMinClips = 64;       // clips from which the clip kernel (one workgroup per clip) serves the call
constexpr int64_t kBwdClipMaxFrames = kClipwThreads / 64;   // one wave per frame of a clip

enum class FwdRoute { Slot, PersistentSlot, Wavew, Wave2 };
enum class BwdRoute { SlotRecompute, SlotSpec, Wave2Spec, Clip };

// Slot against persistent slot, measured (tools/ab_stft.py, 256 clips x 4096 samples): n_fft 2048 forward 25.2 -> 21.9 us, forward of a pair
// 42.4 -> 38.1 us; n_fft 512 10.2 -> 10.8 / 16.7 -> 17.8 us -- the small transforms already share a workgroup's tables among 4-16 frame
// slots, so only n_fft 2048 (one frame per workgroup) takes the persistent form.
static FwdRoute pick_forward_route(const StftArgs& a)
{
    const int64_t T = a.batch * a.frames;   // the pair form arrives as ONE batch of both signals
    if (a.logm != 10) return FwdRoute::Slot;
    if (T >= kFwdWavewMinFrames && T < kWave2MinFrames) return FwdRoute::Wavew;
    if (T >= kWave2MinFrames) return FwdRoute::Wave2;
    return FwdRoute::PersistentSlot;
}

// Clip: the WHOLE backward in one kernel (no overlap-add launch).  Wave2Spec: QS = hop / 128 register slots between a group's two frames,
// scratch rows written as 8-byte pairs.
static BwdRoute pick_backward_route(const StftArgs& a)
{
    if (a.spec_in == nullptr) return BwdRoute::SlotRecompute;
    if (a.logm == 10 && a.frames >= 1 && a.frames <= kBwdClipMaxFrames && (a.hop & 1) == 0 && a.batch >= kBwdClipMinClips) return BwdRoute::Clip;
    if (a.logm == 10 && a.batch * a.groups >= kBwdWave2MinGroups && (a.hop == 256 || a.hop == 512) &&
        (reinterpret_cast<uintptr_t>(a.partial) & 7u) == 0 && (a.span & 1) == 0)
        return BwdRoute::Wave2Spec;
    return BwdRoute::SlotSpec;
}

// ---- one launcher per route ---------------------------------------------------------------------------------------------------------
// launches KERNEL<log2(n_fft / 2)> with one frame slot per unit of `work`
#define SOT_STFT_LAUNCH(KERNEL, work, extra_lds_per_slot, st, a)                                                              \
    do {                                                                                                                      \
        switch ((a).logm) {                                                                                                   \
            case 5: launch_slots<KERNEL<5>, 5>(work, extra_lds_per_slot, st, a); break;                                       \
            case 6: launch_slots<KERNEL<6>, 6>(work, extra_lds_per_slot, st, a); break;                                       \
            case 7: launch_slots<KERNEL<7>, 7>(work, extra_lds_per_slot, st, a); break;                                       \
            case 8: launch_slots<KERNEL<8>, 8>(work, extra_lds_per_slot, st, a); break;                                       \
            case 9: launch_slots<KERNEL<9>, 9>(work, extra_lds_per_slot, st, a); break;                                       \
            case 10: launch_slots<KERNEL<10>, 10>(work, extra_lds_per_slot, st, a); break;                                    \
            default: launch_slots<KERNEL<11>, 11>(work, extra_lds_per_slot, st, a); break;                                    \
        }                                                                                                                     \
    } while (0)

template <auto Kernel, int LOGM>
static void launch_slots(int64_t work, size_t extra_lds_per_slot, hipStream_t st, const StftArgs& a)
{
    using G = Geo<LOGM>;
    const size_t lds = G::lds_points * sizeof(float2) + (size_t)G::slots * extra_lds_per_slot;
    if (lds > 64 * 1024) sot::allow_full_lds_once<Kernel>();
    const unsigned grid = (unsigned)((work + G::slots - 1) / G::slots);
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(kThreads), lds, st, a);
}

// the persistent forward kernel (n_fft 2048) on as many workgroups as stay resident (LDS / 2048 threads per CU)
static void launch_forward_persistent(const StftArgs& a, hipStream_t st)
{
    using G = Geo<10>;
    const size_t lds = ((size_t)G::slots * G::zpoints + G::m) * sizeof(float2);
    static sot::GridCache cache;   // (not launch_persistent: the caller reads the launch's status)
    const int resident = sot::cached_resident_grid(cache, stft_mag_forward_persistent_kernel<10>, kThreads, lds);
    hipLaunchKernelGGL(stft_mag_forward_persistent_kernel<10>, dim3(sot::persistent_grid((a.batch * a.frames + G::slots - 1) / G::slots, resident)), dim3(kThreads), lds, st, a);
}

static void launch_forward_wavew(const StftArgs& a, hipStream_t st)
{
    sot::allow_full_lds_once<stft_mag_forward_wavew_kernel>();
    const int grid = sot::capped_grid((a.batch * a.frames + kFwdwWaves - 1) / kFwdwWaves, 3);   // three 256-thread workgroups per CU (LDS)
    hipLaunchKernelGGL(stft_mag_forward_wavew_kernel, dim3(grid), dim3(kFwdwThreads), kFwdwLdsBytes, st, a);
}

static void launch_forward_wave2(const StftArgs& a, hipStream_t st)
{
    sot::allow_full_lds_once<stft_mag_forward_wave2_kernel>();
    const int grid = sot::capped_grid((a.batch * a.frames + kWave2Waves - 1) / kWave2Waves, 1);   // one 1024-thread workgroup per CU
    hipLaunchKernelGGL(stft_mag_forward_wave2_kernel, dim3(grid), dim3(kWave2Threads), kWave2LdsBytes, st, a);
}

static void launch_backward_clip(const StftArgs& a, hipStream_t st)
{
    sot::allow_full_lds_once<stft_mag_backward_spec_clipw_kernel>();
    hipLaunchKernelGGL(stft_mag_backward_spec_clipw_kernel, dim3(sot::capped_grid(a.batch, 1)), dim3(kClipwThreads), kClipwLdsBytes, st, a);
}

template <int QS>
static void launch_backward_wave2(const StftArgs& a, hipStream_t st)
{
    sot::allow_full_lds_once<stft_mag_backward_spec_wave2_kernel<QS>>();
    const int grid = sot::capped_grid((a.batch * a.groups + kBwdWave2Waves - 1) / kBwdWave2Waves, 1);   // one 512-thread workgroup per CU
    hipLaunchKernelGGL(stft_mag_backward_spec_wave2_kernel<QS>, dim3(grid), dim3(kBwdWave2Threads), kBwdWave2LdsBytes, st, a);
}

// the tail of the two forward entry points: pick, launch
static int run_forward(const StftArgs& a, void* stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    switch (pick_forward_route(a)) {
        case FwdRoute::Wavew: launch_forward_wavew(a, st); break;
        case FwdRoute::Wave2: launch_forward_wave2(a, st); break;
        case FwdRoute::PersistentSlot: launch_forward_persistent(a, st); break;
        case FwdRoute::Slot: SOT_STFT_LAUNCH(stft_mag_forward_kernel, a.batch * a.frames, 0, st, a); break;
    }
    return sot::launch_status();
}

}  // namespace sot_stft

extern "C" {

#ifdef STFT_STAMPS
int sot_stft_debug_read_stamps(unsigned long long* host_out, int count)   // diagnostic build only (synchronises)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(sot_stft::g_stft_stamps), sizeof(unsigned long long) * count) == hipSuccess ? 0 : -1;
}
#endif

int64_t sot_stft_frames(int64_t samples, int hop) { return (samples < 1 || hop < 1) ? 0 : (samples + hop - 1) / hop; }

int sot_stft_mag_forward(const float* audio, int64_t batch, int64_t samples, int64_t audio_row_stride, const float* window,
                         int n_fft, int hop, float* mag, void* stream)
{
    return sot_stft_mag_forward_spec(audio, batch, samples, audio_row_stride, window, n_fft, hop, mag, nullptr, stream);
}

int sot_stft_mag_forward_spec(const float* audio, int64_t batch, int64_t samples, int64_t audio_row_stride, const float* window,
                              int n_fft, int hop, float* mag, float* spec, void* stream)
{
    using namespace sot_stft;
    StftArgs a{};
    const int rc = fill_args(audio, batch, samples, audio_row_stride, window, n_fft, hop, &a);
    if (rc != SOT_OK) return rc;
    if (batch == 0) return SOT_OK;
    if (mag == nullptr) return SOT_ERR_NULL_POINTER;
    if (spec != nullptr && reinterpret_cast<uintptr_t>(spec) % 8 != 0) return SOT_ERR_BAD_SHAPE;
    a.mag = mag;
    a.spec = reinterpret_cast<float2*>(spec); a.spec_first = 0;
    return run_forward(a, stream);
}

int sot_stft_mag_forward_pair(const float* audio_a, int64_t row_stride_a, const float* audio_b, int64_t row_stride_b,
                              int64_t batch_each, int64_t samples, const float* window, int n_fft, int hop, float* mag, void* stream)
{
    return sot_stft_mag_forward_pair_spec(audio_a, row_stride_a, audio_b, row_stride_b, batch_each, samples, window, n_fft, hop, mag, nullptr, stream);
}

int sot_stft_mag_forward_pair_spec(const float* audio_a, int64_t row_stride_a, const float* audio_b, int64_t row_stride_b,
                                   int64_t batch_each, int64_t samples, const float* window, int n_fft, int hop, float* mag, float* spec_b,
                                   void* stream)
{
    using namespace sot_stft;
    if (row_stride_b < samples) return SOT_ERR_BAD_SHAPE;
    StftArgs a{};
    const int rc = fill_args(audio_a, 2 * batch_each, samples, row_stride_a, window, n_fft, hop, &a);
    if (rc != SOT_OK) return rc;
    if (batch_each == 0) return SOT_OK;
    if (mag == nullptr || audio_b == nullptr) return SOT_ERR_NULL_POINTER;
    if (spec_b != nullptr && reinterpret_cast<uintptr_t>(spec_b) % 8 != 0) return SOT_ERR_BAD_SHAPE;
    a.audio_b = audio_b; a.split = batch_each; a.row_stride_b = row_stride_b;
    a.mag = mag;
    a.spec = reinterpret_cast<float2*>(spec_b); a.spec_first = batch_each;   // the spectrum of the SECOND signal only (the estimate: the one that is differentiated)
    return run_forward(a, stream);
}

size_t sot_stft_backward_workspace_bytes(int64_t batch, int64_t samples, int n_fft, int hop)
{
    if (batch < 1 || samples < 1 || hop < 1 || n_fft < 1) return 0;
    const int64_t frames = (samples + hop - 1) / hop;
    const int64_t groups = (frames + sot_stft::kFramesPerGroup - 1) / sot_stft::kFramesPerGroup;
    const int64_t span = n_fft + (int64_t)hop * (sot_stft::kFramesPerGroup - 1);
    return sizeof(float) * (size_t)(batch * groups * span);
}

int sot_stft_mag_backward(const float* audio, int64_t batch, int64_t samples, int64_t audio_row_stride, const float* window,
                          int n_fft, int hop, const float* grad_mag, const float* grad_scale, float* grad_audio, int accumulate,
                          void* workspace, size_t workspace_bytes, void* stream)
{
    return sot_stft_mag_backward_spec(audio, nullptr, batch, samples, audio_row_stride, window, n_fft, hop, grad_mag, grad_scale, grad_audio,
                                      accumulate, workspace, workspace_bytes, stream);
}

int sot_stft_mag_backward_spec(const float* audio, const float* spec, int64_t batch, int64_t samples, int64_t audio_row_stride,
                               const float* window, int n_fft, int hop, const float* grad_mag, const float* grad_scale, float* grad_audio,
                               int accumulate, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace sot_stft;
    StftArgs a{};
    if (spec != nullptr && audio == nullptr) { audio = spec; audio_row_stride = samples; }   // never read: the spectra replace the audio
    if (spec != nullptr && reinterpret_cast<uintptr_t>(spec) % 8 != 0) return SOT_ERR_BAD_SHAPE;
    const int rc = fill_args(audio, batch, samples, audio_row_stride, window, n_fft, hop, &a);
    if (rc != SOT_OK) return rc;
    a.spec_in = reinterpret_cast<const float2*>(spec);
    if (batch == 0) return SOT_OK;
    if (grad_mag == nullptr || grad_audio == nullptr || workspace == nullptr) return SOT_ERR_NULL_POINTER;
    if (workspace_bytes < sot_stft_backward_workspace_bytes(batch, samples, n_fft, hop)) return SOT_ERR_WORKSPACE;
    const int64_t span = n_fft + (int64_t)hop * (kFramesPerGroup - 1);
    if (span > 8192) return SOT_ERR_UNSUPPORTED_SIZE;   // the groups' gradients live in LDS
    if (samples > 0x7fffffffLL) return SOT_ERR_UNSUPPORTED_SIZE;   // overlap-add kernel: 32-bit sample indices inside a clip
    a.grad_mag = grad_mag; a.grad_scale = grad_scale; a.grad_audio = grad_audio; a.accumulate = accumulate;
    a.partial = reinterpret_cast<float*>(workspace);
    a.groups = (a.frames + kFramesPerGroup - 1) / kFramesPerGroup;
    a.span = (int)span;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    switch (pick_backward_route(a)) {
        case BwdRoute::Clip: launch_backward_clip(a, st); return sot::launch_status();   // overlap-add inside
        case BwdRoute::Wave2Spec: if (a.hop == 256) launch_backward_wave2<2>(a, st); else launch_backward_wave2<4>(a, st); break;
        case BwdRoute::SlotSpec: SOT_STFT_LAUNCH(stft_mag_backward_spec_kernel, batch * a.groups, sizeof(float) * (size_t)span, st, a); break;
        case BwdRoute::SlotRecompute: SOT_STFT_LAUNCH(stft_mag_backward_partial_kernel, batch * a.groups, sizeof(float) * (size_t)span, st, a); break;
    }
    if (sot::launch_status() != SOT_OK) return SOT_ERR_LAUNCH;
    const int64_t per_clip = (samples + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(stft_overlap_add_kernel, dim3((unsigned)(per_clip < 64 ? per_clip : 64), (unsigned)(batch < 65535 ? batch : 65535)), dim3(kThreads), 0, st, a);
    return sot::launch_status();
}

}  // extern "C"
