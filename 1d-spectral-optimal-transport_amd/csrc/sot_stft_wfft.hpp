// sot_stft_wfft.hpp -- the two kernels of the STFT-magnitude producer that run on the one-wavefront FFT of csrc/sot_wave_fft.hpp
// (round 5; n_fft 2048 only).
//
// That FFT was written for the two-launch MSSLoss: 16 points per lane, radix-4 stages
// in registers, padded additive exchange maps, fused complex products, a transposed network for the inverse -- a frame's forward transform is
// ~415 instructions and ~4 000 clocks on one wave against the 28 000-clock chain of the round-4 wave kernels (sot_stft_wave2.hpp).
//  * stft_mag_backward_spec_clipw_kernel: the backward from the stored spectrum with the overlap-add INSIDE the kernel, for clips of at most
//    16 frames (config 5 and the paper's step: 4096 samples, hop 256), one 1024-thread workgroup per clip: wave f turns frame f's spectrum
//    and upstream gradient into the Hermitian packing G (natural order in its LDS buffer), runs the inverse network and leaves the windowed
//    frame gradient in its buffer; after one barrier the workgroup adds the frames that cover each sample in ascending frame order
//    (deterministic): no scratch buffer, no second kernel (stft_overlap_add_kernel: 7 us at 256 clips).
//  * stft_mag_forward_wavew_kernel: forward (single or pair form, optional spectrum) with one wavefront per frame in 256-thread workgroups,
//    for the batches BELOW the round-4 wave kernel's threshold (512 ... 3071 frames: the paper's 64 clips), where the slot kernel ran.
//
// Their complex arithmetic stands in a namespace of its own, sot_stft_wfft, in which the complex helpers are sot_wfft's FUSED forms (cmul,
// cmul_conj, add_conj, ...): the three-rounding helpers of sot_stft (sot_stft_common.hpp) are not visible there and have to be named in full.
#pragma once
#include "sot_stft_common.hpp"

// Diagnostic build only (-DSTFT_STAMPS; tools/r5/stft_stamps.py): wave 0 of workgroups 0 .. 63 of the wavew forward kernel (slots 0-4) and of the clipw backward kernel (slots 8-14) stamps the shader clock
#ifdef STFT_STAMPS
namespace sot_stft { __device__ unsigned long long g_stft_stamps[64 * 16]; }
#define STFT_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 64) { __builtin_amdgcn_sched_barrier(0); sot_stft::g_stft_stamps[blockIdx.x * 16 + (i)] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define STFT_STAMP(i) do { } while (0)
#endif

namespace sot_stft_wfft {

using namespace sot_wfft;
using sot_stft::magnitude;
using sot_stft::magnitude_plain;

constexpr int kClipwThreads = 1024;   // sixteen waves: one per frame of the clip
constexpr size_t kClipwLdsBytes = ((size_t)16 * kBuf + kTw + kWnMax) * sizeof(float2);
constexpr int kFwdwThreads = 256, kFwdwWaves = 4;   // 51.2 KB of LDS per workgroup (tables 16.4 KB + 8.7 KB per wave): three per CU; a 1088-frame launch reaches every CU
constexpr size_t kFwdwLdsBytes = ((size_t)kFwdwWaves * kBuf + kTw + kWnMax) * sizeof(float2);

// Hermitian packing G of Zin_k = g_k X_k / |X_k| for the lane's bin pairs (k, m - k), k = 64 q + lane (q < 8) and k = m / 2 (lane 0), written to the
// wave's buffer in natural order (csrc/sot_mss.hip: pair_pass, here from the stored spectrum).  PLAIN: 1 / |X| = rsq(re^2 + im^2); the pass also
// returns the largest and the smallest non-zero component magnitude, from which the caller decides whether PLAIN was legitimate.
template <bool PLAIN>
__device__ __forceinline__ void clipw_pack_gradient(const float2* __restrict__ sp, const float* __restrict__ g, float up, v2f* zl,
                                                    const v2f* wn, int lane, float& peak, float& least)
{
    constexpr int m = 1024;
    peak = 0.0f; least = INFINITY;
    // every load of the pass first (34 per lane; bin m / 2 by all lanes: one address): ONE round trip.  Loads inside the pair loop were waited
    // for pair by pair -- nine serial round trips, 10 000 of a wave's 29 000 clocks (tools/r5/stft_stamps.py)
    float2 lpk[9], lpm[9];
    float lgk[9], lgm[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const int k = (q < 8) ? 64 * q + lane : m / 2;
        lpk[q] = sp[k]; lpm[q] = sp[m - k];
        lgk[q] = g[k]; lgm[q] = g[m - k];
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        if (q == 8 && lane != 0) break;
        const int k = (q < 8) ? 64 * q + lane : m / 2;
        const float2 pk = lpk[q], pm = lpm[q];
        const v2f xk = (v2f){pk.x, pk.y}, xm = (v2f){pm.x, pm.y};
        const float gk = lgk[q] * up, gm = lgm[q] * up;
        float ck, cm;
        if (PLAIN) {
            const float ak = fmaxf(fabsf(pk.x), fabsf(pk.y)), am = fmaxf(fabsf(pm.x), fabsf(pm.y));
            peak = fmaxf(peak, fmaxf(ak, am));
            least = fminf(least, fminf(ak > 0.0f ? ak : INFINITY, am > 0.0f ? am : INFINITY));
            const float sk2 = fmaf(xk.x, xk.x, xk.y * xk.y), sm2 = fmaf(xm.x, xm.x, xm.y * xm.y);
            ck = sk2 > 0.0f ? gk * __builtin_amdgcn_rsqf(sk2) : 0.0f;      // torch: sgn(0) = 0
            cm = sm2 > 0.0f ? gm * __builtin_amdgcn_rsqf(sm2) : 0.0f;
        } else {
            const float mk = hypotf(xk.x, xk.y), mm = hypotf(xm.x, xm.y);
            ck = mk > 0.0f ? gk / mk : 0.0f;
            cm = mm > 0.0f ? gm / mm : 0.0f;
        }
        if (q == 0 && k == 0) { ck *= 2.0f; cm *= 2.0f; }                  // H_0 and H_m are the (real) Zin themselves, not halves
        const v2f hk = ck * xk;                                             // 2 H_k
        const v2f hc = (q < 8) ? cm * cconj(xm) : cconj(hk);               // 2 conj H_(m-k)
        const v2f sk = 0.5f * (hk + hc), dd = hk - hc;
        // the THREE-ROUNDING product, alone in this file: it is what this kernel has always computed (the name used to resolve to
        // sot_stft's), and the gradients of the clip route are pinned bit for bit
        const v2f P = sot_stft::cmul_conj(dd, wn[k]);                      // i conj(W) (H_k - conj H_(m-k))
        zl[k] = sk + P;
        if (q < 8 && k != 0) zl[m - k] = conj_sub(sk, P);
    }
}

// the frame's bins from the packed transform in the wave's buffer (natural order, Z_0 again at slot m): |.| / sqrt(n) (and the complex spectrum
// on request); PLAIN: magnitude_plain(), else the careful form
template <bool PLAIN>
__device__ __forceinline__ void wavew_unpack_store(const v2f* zl, const v2f* wn, int lane, float scale, float* dst, float2* sp)
{
    constexpr int m = 1024;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        if (q == 8 && lane != 0) break;
        const int k = (q < 8) ? 64 * q + lane : m / 2;
        const v2f zk = zl[k], zm = zl[m - k];                  // (k = 0: slot m holds the copy of Z_0)
        const v2f e = add_conj(zk, zm), o = sub_conj(zk, zm);
        const v2f wz = cmul(o, wn[k]), eh = 0.5f * e;
        const v2f xk = eh + wz, xc = eh - wz;                   // X_k, conj X_(m-k)
        dst[k] = (PLAIN ? magnitude_plain(xk) : magnitude(xk)) * scale;
        dst[m - k] = (PLAIN ? magnitude_plain(xc) : magnitude(xc)) * scale;
        if (sp != nullptr) { sp[k] = make_float2(xk.x, xk.y); sp[m - k] = make_float2(xc.x, -xc.y); }
    }
}

}  // namespace sot_stft_wfft

// The kernels keep their names in sot_stft.  Their own text is addressing, loads, the transform calls and stores: no complex helper is
// named in it (one would resolve to sot_stft's three-rounding form); whatever needs one stands above, in sot_stft_wfft.  (The bodies as
// functions of that namespace, called from here, moved both kernels' code.)
namespace sot_stft {

using sot_stft_wfft::kClipwThreads;
using sot_stft_wfft::kClipwLdsBytes;
using sot_stft_wfft::kFwdwThreads;
using sot_stft_wfft::kFwdwWaves;
using sot_stft_wfft::kFwdwLdsBytes;

__global__ __launch_bounds__(kClipwThreads) void stft_mag_backward_spec_clipw_kernel(const StftArgs a)
{
    using namespace sot_wfft;
    constexpr int n = 2048, nb = 1025, m = 1024;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    v2f* const tw = reinterpret_cast<v2f*>(smem_f);
    v2f* const wn = tw + kTw;
    v2f* const bufs = wn + kWnMax;                   // 16 frame buffers of kBuf points
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    v2f* const zl = bufs + wave * kBuf;
    STFT_STAMP(8);
    build_tables<kClipwThreads>(kWn, tw, wn);
    __syncthreads();
    STFT_STAMP(9);
    const float scale = 1.0f / sqrtf((float)n);
    const float up = a.grad_scale ? *a.grad_scale : 1.0f;
    const int frames = (int)a.frames, hp = a.hop >> 1;        // hop in packed points (hop is even: host)
    const int samples = (int)a.samples;
    const float2* const win2 = reinterpret_cast<const float2*>(a.window);
    for (int64_t b = blockIdx.x; b < a.batch; b += gridDim.x) {
        if (wave < frames) {
            int lane = threadIdx.x & 63;
            asm volatile("" : "+v"(lane));   // lane-derived LDS addresses are recomputed per clip instead of living in registers across clips
            const float2* const sp = a.spec_in + (b * a.frames + wave) * nb;
            const float* const g = a.grad_mag + (b * a.frames + wave) * nb;
            float peak, least;
            sot_stft_wfft::clipw_pack_gradient<true>(sp, g, up, zl, wn, lane, peak, least);
            // re^2 + im^2 of every non-zero bin must be a normal number that cannot overflow: else the careful form.  (A NaN bin does NOT fail
            // this test -- the maxima drop NaN operands -- and needs no care: it propagates through either form.)
            const float wpeak = wave_max_f32(peak), wleast = -wave_max_f32(-least);
            if (__builtin_amdgcn_readfirstlane((int)(wpeak < 1e15f && wleast > 1e-18f)) == 0) {
                wave_sync();
                sot_stft_wfft::clipw_pack_gradient<false>(sp, g, up, zl, wn, lane, peak, least);
            }
            wave_sync();
            STFT_STAMP(10);
            v2f r[16], wt[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) r[q] = zl[lane + 64 * brev4(q)];
#pragma unroll
            for (int q = 0; q < 16; ++q) { const float2 wv = win2[64 * q + lane]; wt[q] = (v2f){wv.x, wv.y}; }   // arrive during the transform
            wave_sync();
            inverse_transform<10>(r, zl, tw, lane);
            STFT_STAMP(11);
#pragma unroll
            for (int q = 0; q < 16; ++q) zl[64 * q + lane] = (wt[q] * r[q]) * scale;      // the windowed frame gradient, packed point 64 q + lane
        }
        __syncthreads();
        STFT_STAMP(12);
        float* const dst = a.grad_audio + b * a.samples;
        for (int p = threadIdx.x; 2 * p < samples; p += kClipwThreads) {   // packed point p of the clip = samples 2 p, 2 p + 1
            const int f_hi = min(p / hp, frames - 1);
            int f_lo = (p - (m - 1) + hp - 1) / hp;
            if (p - (m - 1) <= 0) f_lo = 0;
            v2f sum = (v2f){0.0f, 0.0f};
            for (int f = f_lo; f <= f_hi; ++f) sum += bufs[f * kBuf + (p - f * hp)];
            if (2 * p + 1 < samples) {
                float2* d2 = reinterpret_cast<float2*>(dst + 2 * p);
                if ((reinterpret_cast<uintptr_t>(d2) & 7u) == 0) {
                    float2 o = make_float2(sum.x, sum.y);
                    if (a.accumulate) { const float2 old = *d2; o.x += old.x; o.y += old.y; }
                    *d2 = o;
                } else {
                    dst[2 * p] = a.accumulate ? dst[2 * p] + sum.x : sum.x;
                    dst[2 * p + 1] = a.accumulate ? dst[2 * p + 1] + sum.y : sum.y;
                }
            } else {
                dst[2 * p] = a.accumulate ? dst[2 * p] + sum.x : sum.x;
            }
        }
        STFT_STAMP(13);
        __syncthreads();   // the frame buffers are read before the next clip overwrites them
        STFT_STAMP(14);
    }
}

__global__ __launch_bounds__(kFwdwThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void stft_mag_forward_wavew_kernel(const StftArgs a)
{
    using namespace sot_wfft;
    constexpr int n = 2048, nb = 1025;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    v2f* const tw = reinterpret_cast<v2f*>(smem_f);
    v2f* const wn = tw + kTw;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    v2f* const zl = wn + kWnMax + wave * kBuf;
    const float2* const win2 = reinterpret_cast<const float2*>(a.window);
    const unsigned total = (unsigned)(a.batch * a.frames), frames = (unsigned)a.frames;
    const unsigned stride = gridDim.x * kFwdwWaves;
    STFT_STAMP(0);
    // (the first frame's 32 loads issued ahead of the table build change nothing: the build then waits behind them -- tables + loads are
    //  ~6 300 clocks of a wave's 13 000 either way, tools/r5/stft_stamps.py)
    build_tables<kFwdwThreads>(kWn, tw, wn);
    __syncthreads();
    STFT_STAMP(1);
    const float scale = 1.0f / sqrtf((float)n);
    for (unsigned fr = blockIdx.x * kFwdwWaves + wave; fr < total; fr += stride) {
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));
        const unsigned b = fr / frames, f = fr - b * frames;
        // (clip row and 16-point fetch: inline copies -- as helpers they move this kernel's code, see sot_stft_common.hpp)
        const float* src = (a.audio_b != nullptr && (int64_t)b >= a.split) ? a.audio_b + ((int64_t)b - a.split) * a.row_stride_b
                                                                          : a.audio + (int64_t)b * a.row_stride;
        const int64_t t0 = (int64_t)f * a.hop;
        const float* const s0 = src + t0;
        v2f r[16];
        const bool pairs = t0 + n <= a.samples && (reinterpret_cast<uintptr_t>(s0) & 7u) == 0;   // wave-uniform
        if (pairs) {
            const float2* const s2 = reinterpret_cast<const float2*>(s0);
#pragma unroll
            for (int q = 0; q < 16; ++q) { const float2 v = s2[64 * q + lane]; r[q] = (v2f){v.x, v.y}; }
        } else {
            const int left = (int)min((int64_t)n, a.samples - t0);      // zeros past the clip's end (utils.py:252-275)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = 64 * q + lane;
                r[q] = (v2f){(2 * i < left) ? s0[2 * i] : 0.0f, (2 * i + 1 < left) ? s0[2 * i + 1] : 0.0f};
            }
        }
        float amax = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float2 wv = win2[64 * q + lane];
            r[q] = r[q] * (v2f){wv.x, wv.y};
            amax = fmaxf(amax, fmaxf(fabsf(r[q].x), fabsf(r[q].y)));
        }
        const bool plain = __builtin_amdgcn_readfirstlane((int)frame_is_plain(wave_max_f32(amax))) != 0;   // one range test per FRAME
        STFT_STAMP(2);
        forward_transform<10>(r, zl, tw, lane);
        STFT_STAMP(3);
        write_natural<10>(r, zl, lane);
        wave_sync();
        float* const dst = a.mag + (int64_t)fr * nb;
        float2* const sp = spec_row(a, b, fr, frames, nb);
        if (plain) sot_stft_wfft::wavew_unpack_store<true>(zl, wn, lane, scale, dst, sp);
        else sot_stft_wfft::wavew_unpack_store<false>(zl, wn, lane, scale, dst, sp);
        STFT_STAMP(4);
        wave_sync();   // the unpack reads are issued before the next frame's exchange writes
    }
}

}  // namespace sot_stft
