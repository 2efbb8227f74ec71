// sot_stft_wave2.hpp -- the IN-PLACE ONE-WAVEFRONT family of the STFT-magnitude producer (round 4; n_fft 2048 only): one wavefront per
// frame (forward) or per group of two frames (backward from the stored spectrum), three-rounding complex products like the slot family.
//
// The 1024-point complex transform of the packed frame runs as five radix-4 decimation-in-frequency
// stages on 16 points per lane.  With the index written in base 4, i = (d4 d3 d2 d1 d0), a lane keeps two digits in its 16 registers and
// the other three are its lane number: stages 1-2 (digits d4, d3) on r = 4 d4 + d3, lane = 16 d2 + 4 d1 + d0 (element 64 r + lane: the
// load is coalesced), one exchange through the wave's LDS buffer, stages 3-4 (d2, d1), a second exchange, stage 5 (d0); the results are
// written to LDS in natural frequency order (k = q4 + 4 q3 + 16 q2 + 64 q1 + 256 q0) for the pairwise unpacking of the real transform.
// Index algebra checked against numpy's FFT (6e-14) before it was written down here.
#pragma once
#include "sot_stft_common.hpp"

namespace sot_stft {

constexpr int kWaveBuf = 64 * 17;   // v2f slots of one wave's exchange buffer: [lane][16 registers + 1 pad]; >= zi(1024) = 1056

// ---------------------------------------------------------------------------------------------
// Round 4: the one-wavefront-per-frame transform, built around occupancy (stft_mag_forward_wave2_kernel, n_fft 2048).
// What the round-2 kernel paid for: 194 VGPRs (two waves per SIMD) and three quarters of a CU's LDS per four frames.  Here
//  * ONE 1024-thread workgroup per CU: sixteen waves = sixteen frames in flight per CU share one twiddle table (W_1024^j, 8 KB) and one
//    copy of the window (8 KB); 159.8 KB of LDS; the 128-VGPR budget of a 1024-thread workgroup is met by doing every radix-4 stage IN
//    PLACE on the sixteen points a lane holds (no second 16-point array);
//  * the frame's |.| values take magnitude_plain() after ONE range test per frame on the windowed samples (frame_is_plain) instead of a
//    range test, a wave vote and libm's sqrtf per value;
//  * samples and taps are fetched as 8-byte pairs (the clip's row and hop keep frames 8-byte aligned in every reference configuration; a
//    scalar path covers the rest).
// No workgroup barrier inside the frame loop: a wave's exchanges through its private LDS buffer need only wave-level ordering.
// ---------------------------------------------------------------------------------------------
template <bool INVERSE>
__device__ __forceinline__ v2f ctw(v2f a, v2f w) { return INVERSE ? cmul_conj(a, w) : cmul(a, w); }   // a * twiddle (inverse: conjugate twiddle)

template <bool INVERSE>
__device__ __forceinline__ void bf4_ip(v2f& a0, v2f& a1, v2f& a2, v2f& a3)
{
    const v2f s02 = a0 + a2, d02 = a0 - a2, s13 = a1 + a3, d13 = a1 - a3;
    a0 = s02 + s13; a2 = s02 - s13;
    a1 = INVERSE ? add_pi(d02, d13) : add_mi(d02, d13);   // d02 + (-+i) d13
    a3 = INVERSE ? add_mi(d02, d13) : add_pi(d02, d13);   // d02 - (-+i) d13
}

// r[q] = z[64 q + lane] on entry; on return the transform sits in zl[zi(k)], k = 0 .. 1023 (after the caller's slot_sync).  The index
// algebra is the one above (five radix-4 decimation-in-frequency stages, two exchanges), every stage in place.
template <bool INVERSE>
__device__ __forceinline__ void fft1024_wave_ip(v2f (&r)[16], v2f* zl, const v2f* tw, int lane)
{
    // stage 1 (digit d4; registers 4 p + d3 -> 4 q + d3): twiddle W_1024^{(64 d3 + lane) q}
#pragma unroll
    for (int d3 = 0; d3 < 4; ++d3) {
        const int j = 64 * d3 + lane;
        const v2f w1 = tw[j & 1023], w2 = tw[(2 * j) & 1023], w3 = tw[(3 * j) & 1023];   // requested ahead of the butterfly
        bf4_ip<INVERSE>(r[d3], r[4 + d3], r[8 + d3], r[12 + d3]);
        r[4 + d3] = ctw<INVERSE>(r[4 + d3], w1); r[8 + d3] = ctw<INVERSE>(r[8 + d3], w2); r[12 + d3] = ctw<INVERSE>(r[12 + d3], w3);
    }
    // stage 2 (digit d3; registers 4 q4 + p -> 4 q4 + q): twiddle W_256^{lane q} = W_1024^{4 lane q}
    {
        const v2f w1 = tw[(4 * lane) & 1023], w2 = tw[(8 * lane) & 1023], w3 = tw[(12 * lane) & 1023];   // the same three for every q4
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            bf4_ip<INVERSE>(r[4 * q4], r[4 * q4 + 1], r[4 * q4 + 2], r[4 * q4 + 3]);
            r[4 * q4 + 1] = ctw<INVERSE>(r[4 * q4 + 1], w1); r[4 * q4 + 2] = ctw<INVERSE>(r[4 * q4 + 2], w2); r[4 * q4 + 3] = ctw<INVERSE>(r[4 * q4 + 3], w3);
        }
    }
    // exchange 1: register (q4, q3) of lane (d2, d1, d0) -> register (d2, d1) of lane (q4, q3, d0): logical element (column 4 q + d0, row rr)
    // written by lane (rr, d0), row q of column L read by lane L.  Storage [column ^ g(row)][17]: the reader's lanes still sweep 64 different
    // columns per instruction (conflict-free as before), the writer's 16-lane groups no longer pile four lanes on one bank pair
    // (SQ_LDS_BANK_CONFLICT was 49 % of the kernel's LDS cycles, all of it these stores): g(row) = 4 (row & 3) here (two-way left),
    // g(row) = row >> 2 in exchange 2 (conflict-free).
    const int d0 = lane & 3;
    {
        const int rr = lane >> 2;   // 4 d2 + d1
#pragma unroll
        for (int q = 0; q < 16; ++q) zl[((4 * q + d0) ^ (4 * (rr & 3))) * 17 + rr] = r[q];
        slot_sync<true>();
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = zl[(lane ^ (4 * (q & 3))) * 17 + q];
        slot_sync<true>();
    }
    // stage 3 (digit d2; registers 4 p + d1 -> 4 q + d1): twiddle W_64^{(4 d1 + d0) q} = W_1024^{16 (4 d1 + d0) q}
#pragma unroll
    for (int d1 = 0; d1 < 4; ++d1) {
        const int j = 16 * (4 * d1 + d0);
        const v2f w1 = tw[j & 1023], w2 = tw[(2 * j) & 1023], w3 = tw[(3 * j) & 1023];
        bf4_ip<INVERSE>(r[d1], r[4 + d1], r[8 + d1], r[12 + d1]);
        r[4 + d1] = ctw<INVERSE>(r[4 + d1], w1); r[8 + d1] = ctw<INVERSE>(r[8 + d1], w2); r[12 + d1] = ctw<INVERSE>(r[12 + d1], w3);
    }
    // stage 4 (digit d1; registers 4 q2 + p -> 4 q2 + q): twiddle W_16^{d0 q} = W_1024^{64 d0 q}
    {
        const v2f w1 = tw[(64 * d0) & 1023], w2 = tw[(128 * d0) & 1023], w3 = tw[(192 * d0) & 1023];   // the same three for every q2
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) {
            bf4_ip<INVERSE>(r[4 * q2], r[4 * q2 + 1], r[4 * q2 + 2], r[4 * q2 + 3]);
            r[4 * q2 + 1] = ctw<INVERSE>(r[4 * q2 + 1], w1); r[4 * q2 + 2] = ctw<INVERSE>(r[4 * q2 + 2], w2); r[4 * q2 + 3] = ctw<INVERSE>(r[4 * q2 + 3], w3);
        }
    }
    // exchange 2: register (q2, q1) of lane (q4, q3, d0) -> register (d0, q1) of lane (q4, q3, q2)
    {
        const int hi = lane >> 2;   // 4 q4 + q3
#pragma unroll
        for (int q = 0; q < 16; ++q) zl[((4 * hi + (q >> 2)) ^ d0) * 17 + 4 * d0 + (q & 3)] = r[q];   // row 4 d0 + (q & 3): g = d0
        slot_sync<true>();
#pragma unroll
        for (int q = 0; q < 16; ++q) r[q] = zl[(lane ^ (q >> 2)) * 17 + q];
        slot_sync<true>();
    }
    // stage 5 (digit d0; registers 4 p + q1 -> 4 q0 + q1), no twiddle; result (q4 q3 q2 q1 q0) is frequency k = q4 + 4 q3 + 16 q2 + 64 q1 + 256 q0
    const int kb = (lane >> 4) + 4 * ((lane >> 2) & 3) + 16 * (lane & 3);
#pragma unroll
    for (int q1 = 0; q1 < 4; ++q1) {
        bf4_ip<INVERSE>(r[q1], r[4 + q1], r[8 + q1], r[12 + q1]);
#pragma unroll
        for (int q0 = 0; q0 < 4; ++q0) zl[zi(kb + 64 * q1 + 256 * q0)] = r[4 * q0 + q1];
    }
}

constexpr int kWave2Threads = 1024;
constexpr int kWave2Waves = kWave2Threads / 64;
constexpr size_t kWave2LdsBytes = (1024 + 520 + 1024 + (size_t)kWave2Waves * kWaveBuf) * sizeof(float2);

// tables of the one-wave kernels: W_1024^j, W_2048^k (k <= 512), the window as tap pairs; all threads of the workgroup, then a barrier
template <int THREADS>
__device__ __forceinline__ void wave2_load_tables(const StftArgs& a, v2f* tw, v2f* wn, v2f* wl)
{
    const float2* win = reinterpret_cast<const float2*>(a.window);
    for (int j = threadIdx.x; j < 1024; j += THREADS) {   // W_1024^{256 a + b} = W_2048^{2 b} (-i)^a  (exact quarter turns of the committed table)
        const float2 t = kWn[4 * (j & 255)];
        v2f w = (v2f){t.x, t.y};
        const int qa = j >> 8;
        if (qa == 1) w = mul_mi(w); else if (qa == 2) w = -w; else if (qa == 3) w = mul_i(w);
        tw[j] = w;
        const float2 tap = win[j];
        wl[j] = (v2f){tap.x, tap.y};
    }
    for (int k = threadIdx.x; k <= 512; k += THREADS) { const float2 t = kWn[2 * k]; wn[k] = (v2f){t.x, t.y}; }
    __syncthreads();
}

// the frame's bins from the transform in LDS: |.| / sqrt(n) (and the complex spectrum on request); PLAIN: magnitude_plain(), else the careful form
template <bool PLAIN>
__device__ __forceinline__ void wave2_unpack_store(const v2f* zl, const v2f* wn, int lane, float scale, float* dst, float2* sp)
{
    constexpr int LOGM = 10, m = 1024;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int k = lane + 64 * j;
        if (j < 8 || k <= m / 2) {
            v2f xk, xm;
            unpack_pair<LOGM>(zl, wn, k, xk, xm);
            dst[k] = (PLAIN ? magnitude_plain(xk) : magnitude(xk)) * scale;
            dst[m - k] = (PLAIN ? magnitude_plain(xm) : magnitude(xm)) * scale;
            if (sp != nullptr) store_spec(sp, k, m - k, xk, xm);
        }
    }
}

__global__ __launch_bounds__(kWave2Threads) void stft_mag_forward_wave2_kernel(const StftArgs a)
{
    constexpr int n = 2048, nb = 1025;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    v2f* const tw = reinterpret_cast<v2f*>(smem_f);          // W_1024^j, j < 1024
    v2f* const wn = tw + 1024;                                // W_2048^k, k <= 512 (+ pad)
    v2f* const wl = wn + 520;                                 // window taps (2 i, 2 i + 1), i < 1024
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;   // the wave number in a scalar register:
    v2f* const zl = wl + 1024 + wave * kWaveBuf;                                                        // frame, clip and row pointers stay scalar
    const float2* win = reinterpret_cast<const float2*>(a.window);
    const unsigned total = (unsigned)(a.batch * a.frames), frames = (unsigned)a.frames;
    const unsigned stride = gridDim.x * kWave2Waves;
    v2f r[16];
    // (16-point fetch and spectrum row: inline copies, see sot_stft_common.hpp)
    auto fetch = [&](unsigned fr) {   // raw samples (2 i, 2 i + 1), i = 64 q + lane, of frame fr; zeros past the clip's end (utils.py:252-275)
        const unsigned b = fr / frames, f = fr - b * frames;
        const float* src = clip_row(a, b);
        const int64_t t0 = (int64_t)f * a.hop;
        const float* const s0 = src + t0;
        const bool pairs = t0 + n <= a.samples && (reinterpret_cast<uintptr_t>(s0) & 7u) == 0;   // wave-uniform
        if (pairs) {
            const float2* const s2 = reinterpret_cast<const float2*>(s0);
#pragma unroll
            for (int q = 0; q < 16; ++q) { const float2 v = s2[64 * q + lane]; r[q] = (v2f){v.x, v.y}; }
        } else {
            const int left = (int)min((int64_t)n, a.samples - t0);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = 64 * q + lane;
                r[q] = (v2f){(2 * i < left) ? s0[2 * i] : 0.0f, (2 * i + 1 < left) ? s0[2 * i + 1] : 0.0f};
            }
        }
    };
    unsigned fr = blockIdx.x * kWave2Waves + wave;
    if (fr < total) fetch(fr);   // the first frame's samples are in flight while the tables are built
    // wave2_load_tables<kWave2Threads>() in this kernel's own text: the call moves its code (it sits on the 128-register budget)
    for (int j = threadIdx.x; j < 1024; j += kWave2Threads) {   // W_1024^{256 a + b} = W_2048^{2 b} (-i)^a  (exact quarter turns of the committed table)
        const float2 t = kWn[4 * (j & 255)];
        v2f w = (v2f){t.x, t.y};
        const int qa = j >> 8;
        if (qa == 1) w = mul_mi(w); else if (qa == 2) w = -w; else if (qa == 3) w = mul_i(w);
        tw[j] = w;
        const float2 tap = win[j];
        wl[j] = (v2f){tap.x, tap.y};
    }
    for (int k = threadIdx.x; k <= 512; k += kWave2Threads) { const float2 t = kWn[2 * k]; wn[k] = (v2f){t.x, t.y}; }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)n);
    for (; fr < total; fr += stride) {
        // the lane number as an opaque value per frame: hipcc otherwise hoists every lane-derived LDS address out of this (two-trip) loop
        // and pays for the ~40 live registers with spills (23 dwords at the 128-register budget of a 1024-thread workgroup)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        float amax = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            r[q] = r[q] * wl[64 * q + ln];
            amax = fmaxf(amax, fmaxf(fabsf(r[q].x), fabsf(r[q].y)));
        }
        // one range test per FRAME (NaN samples fail it and take the careful path); a scalar, so the two forms below are two branches
        const bool plain = __builtin_amdgcn_readfirstlane((int)frame_is_plain(wave_max_f32(amax))) != 0;
        fft1024_wave_ip<false>(r, zl, tw, ln);
        if (fr + stride < total) fetch(fr + stride);   // the next frame's samples arrive while this one is unpacked
        slot_sync<true>();
        const unsigned b = fr / frames;
        float* dst = a.mag + (int64_t)fr * nb;
        float2* sp = (a.spec != nullptr && (int64_t)b >= a.spec_first) ? a.spec + ((int64_t)fr - a.spec_first * frames) * nb : nullptr;
        if (plain) wave2_unpack_store<true>(zl, wn, ln, scale, dst, sp);
        else wave2_unpack_store<false>(zl, wn, ln, scale, dst, sp);
        slot_sync<true>();   // the unpack reads are issued before the next frame's exchange writes
    }
}

// ---------------------------------------------------------------------------------------------
// Round 4: the backward from the stored spectrum with ONE WAVEFRONT per frame group (n_fft 2048, hop a multiple of 128; the counterpart
// of stft_mag_forward_wave2_kernel).  A wave takes the kFramesPerGroup = 2 consecutive frames of its group one after the other: spectrum
// and upstream gradient of the lane's nine bin pairs (k, m - k) -> Zin -> Hermitian packing G (as backward_partial_body, with
// 1 / |X| = rsq(re^2 + im^2) after one range test per frame instead of a careful |.| and an IEEE division per value) -> G to the wave's LDS
// buffer in natural order -> the 16 points 64 q + lane into registers -> fft1024_wave_ip<true> -> windowed, scaled, and overlap-added IN
// REGISTERS: the second frame starts QS = hop / 128 register slots behind the first (its packed point i sits at point i + hop / 2 of the
// group's span), same lane.  The group's span leaves as 16 + QS coalesced 8-byte stores into the scratch buffer stft_overlap_add_kernel
// reads (same layout as the slot kernel's).  512-thread workgroups: 8 frame groups in flight per CU (tables 20 KB + 8 x 8.7 KB of LDS).
// ---------------------------------------------------------------------------------------------
constexpr int kBwdWave2Threads = 512;
constexpr int kBwdWave2Waves = kBwdWave2Threads / 64;
constexpr size_t kBwdWave2LdsBytes = (1024 + 520 + 1024 + (size_t)kBwdWave2Waves * kWaveBuf) * sizeof(float2);

// The Hermitian packing G of one frame's Zin_k = g_k X_k / |X_k| into the wave's LDS buffer (natural order), pair by pair -- nothing is held
// across pairs.  PLAIN: 1 / |X| = rsq(re^2 + im^2); the pass also returns the frame's largest and smallest non-zero component magnitude,
// from which the caller decides whether PLAIN was legitimate (and repeats the pass in the careful form if not: rare).
template <bool PLAIN>
__device__ __forceinline__ void wave2_pack_gradient(const float2* __restrict__ sp, const float* __restrict__ g, float up, v2f* zl, const v2f* wn,
                                                    int lane, float& peak, float& least)
{
    constexpr int m = 1024;
    peak = 0.0f; least = INFINITY;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int k = lane + 64 * j;
        if (j < 8 || k <= m / 2) {
            const float2 pk = sp[k], pm = sp[m - k];
            const v2f xk = (v2f){pk.x, pk.y}, xm = (v2f){pm.x, pm.y};
            const float gk_up = g[k], gm_up = g[m - k];
            float ck, cm;
            if (PLAIN) {
                const float ak = fmaxf(fabsf(pk.x), fabsf(pk.y)), am = fmaxf(fabsf(pm.x), fabsf(pm.y));
                peak = fmaxf(peak, fmaxf(ak, am));
                least = fminf(least, fminf(ak > 0.0f ? ak : INFINITY, am > 0.0f ? am : INFINITY));
                const float sk2 = fmaf(xk.x, xk.x, xk.y * xk.y), sm2 = fmaf(xm.x, xm.x, xm.y * xm.y);
                ck = sk2 > 0.0f ? (gk_up * up) * __builtin_amdgcn_rsqf(sk2) : 0.0f;      // torch: sgn(0) = 0
                cm = sm2 > 0.0f ? (gm_up * up) * __builtin_amdgcn_rsqf(sm2) : 0.0f;
            } else {
                const float mk = magnitude(xk), mm = magnitude(xm);
                ck = mk > 0.0f ? (gk_up * up) / mk : 0.0f;
                cm = mm > 0.0f ? (gm_up * up) / mm : 0.0f;
            }
            v2f hk = (0.5f * ck) * xk, hm = (0.5f * cm) * xm;
            if (k == 0) { hk = (v2f){ck * xk.x, 0.0f}; hm = (v2f){cm * xm.x, 0.0f}; }   // H_0, H_m are real
            const v2f sk = hk + cconj(hm);      // H_k + conj(H_{m-k})
            const v2f dk = hk - cconj(hm);      // H_k - conj(H_{m-k})
            const v2f wk = wn[k];
            zl[k] = sk + mul_i(cmul(cconj(wk), dk));                                   // G_k = s + i conj(W) d
            if (k > 0 && k < m - k) zl[m - k] = cconj(sk) + mul_i(cmul(wk, cconj(dk)));   // G_{m-k} = conj(s) + i W conj(d)
        }
    }
}

// One frame of the backward from the stored spectrum on one wavefront: out[q] = tap * (inverse transform of the Hermitian packing of
// Zin_k = g_k X_k / |X_k|) * scale at the packed points 64 q + lane, i.e. the frame's windowed audio gradient (samples 2 i, 2 i + 1).
// sp / g: the frame's spectrum and upstream gradient rows.  Ends with a wave-level ordering point (zl may be reused).
__device__ __forceinline__ void wave2_frame_gradient(const float2* __restrict__ sp, const float* __restrict__ g, float up, float scale, v2f* zl,
                                                     const v2f* tw, const v2f* wn, const v2f* wl, int lane_in, v2f (&out)[16])
{
    int lane = lane_in;
    asm volatile("" : "+v"(lane));   // lane-derived LDS addresses are recomputed per frame instead of living in registers across frames
    float peak, least;
    wave2_pack_gradient<true>(sp, g, up, zl, wn, lane, peak, least);
    // re^2 + im^2 of every non-zero bin must be a normal number that cannot overflow (NaNs fail the test): else the careful form
    const float wpeak = wave_max_f32(peak), wleast = -wave_max_f32(-least);
    if (__builtin_amdgcn_readfirstlane((int)(wpeak < 1e15f && wleast > 1e-18f)) == 0) {
        slot_sync<true>();
        wave2_pack_gradient<false>(sp, g, up, zl, wn, lane, peak, least);
    }
    slot_sync<true>();
    v2f r[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) r[q] = zl[64 * q + lane];
    slot_sync<true>();   // every lane holds its points before the transform's exchanges reuse the buffer
    fft1024_wave_ip<true>(r, zl, tw, lane);
    slot_sync<true>();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const v2f v = zl[zi(64 * q + lane)], tap = wl[64 * q + lane];
        out[q] = (v2f){tap.x * v.x * scale, tap.y * v.y * scale};
    }
    slot_sync<true>();   // the reads are issued before the buffer is written again
}

template <int QS>
__global__ __launch_bounds__(kBwdWave2Threads) void stft_mag_backward_spec_wave2_kernel(const StftArgs a)
{
    static_assert(kFramesPerGroup == 2, "two frames per wave: 16 + QS register slots");
    constexpr int n = 2048, nb = 1025;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    v2f* const tw = reinterpret_cast<v2f*>(smem_f);          // W_1024^j, j < 1024
    v2f* const wn = tw + 1024;                                // W_2048^k, k <= 512 (+ pad)
    v2f* const wl = wn + 520;                                 // window taps (2 i, 2 i + 1), i < 1024
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    v2f* const zl = wl + 1024 + wave * kWaveBuf;
    wave2_load_tables<kBwdWave2Threads>(a, tw, wn, wl);
    const float scale = 1.0f / sqrtf((float)n);
    const float up = a.grad_scale ? *a.grad_scale : 1.0f;
    const unsigned total = (unsigned)(a.batch * a.groups), groups = (unsigned)a.groups;
    for (unsigned w = blockIdx.x * kBwdWave2Waves + wave; w < total; w += gridDim.x * kBwdWave2Waves) {
        const unsigned b = w / groups, grp = w - b * groups;
        v2f acc[16 + QS];
#pragma unroll
        for (int q = 0; q < 16 + QS; ++q) acc[q] = (v2f){0.0f, 0.0f};
#pragma unroll
        for (int fi = 0; fi < 2; ++fi) {
            const int64_t f = (int64_t)grp * 2 + fi;
            if (f < a.frames) {   // wave-uniform
                v2f out[16];
                wave2_frame_gradient(a.spec_in + ((int64_t)b * a.frames + f) * nb, a.grad_mag + ((int64_t)b * a.frames + f) * nb, up, scale, zl, tw, wn,
                                     wl, lane, out);
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q + QS * fi] += out[q];
            }
        }
        float2* dst = reinterpret_cast<float2*>(a.partial + (int64_t)w * a.span);
#pragma unroll
        for (int q = 0; q < 16 + QS; ++q) dst[64 * q + lane] = make_float2(acc[q].x, acc[q].y);
    }
}

}  // namespace sot_stft
