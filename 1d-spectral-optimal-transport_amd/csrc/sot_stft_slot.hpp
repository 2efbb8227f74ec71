// sot_stft_slot.hpp -- the SLOT family of the STFT-magnitude producer: every transform size (n_fft 64 ... 4096), instantiated per size.
//
// Forward: one frame slot (n_fft/8 threads) per frame.  The windowed REAL frame
// is packed into n_fft/2 complex points and goes through an in-LDS complex FFT of half the frame length (bit-reversed
// load, two radix-2 stages per barrier-separated pass, twiddles copied into LDS from constant tables); the n_fft/2 + 1
// bins are unpacked pairwise and reduced to |.| / sqrt(n_fft).
// Backward (closed form of abs o stft's autograd): per group of two consecutive frames, frame by frame, recompute the
// frame's spectrum X, form
// Z_k = g_k X_k / |X_k| (0 where |X_k| = 0, torch's sgn(0)), inverse-transform it as a Hermitian spectrum (again a
// half-length complex transform), multiply by window / sqrt(n_fft) and overlap-add it into the group's gradient, which
// is kept in LDS and written once to a scratch buffer; a second kernel adds, per sample, the groups that cover it in a
// fixed order: no atomics, deterministic.
// HBM traffic: forward reads n_fft samples per frame (L2-resident overlap) and writes n_fft/2+1 magnitudes; backward
// reads the audio and the magnitude gradients once, writes and re-reads the groups' partial gradients (4.5 x the audio
// for 2 frames per group at 8 frames per sample: 19 MB for 4096 frames of 2048, L2/MALL-resident) and writes the audio
// gradient once.  (4 frames per group: 2.75 x, but half the workgroups; the same time at n_fft 2048, 20 % slower over
// the six scales of MSSLoss.)
#pragma once
#include "sot_stft_common.hpp"

namespace sot_stft {

// waves per SIMD the persistent forward kernel is compiled for: 6 = 76 VGPRs, no spills; 8 = 64 VGPRs with 10 spilled, measured
// slower (26.4 vs 21.9 us)
constexpr int kPersistentWaves = 6;

// twiddles from the constant tables (L2-resident) into LDS: tw[2 (h - 1) + pos] = exp(-2 pi i pos / 2h),
// tw[2 (h - 1) + h + pos] = exp(-2 pi i pos / 4h) for every pass half size h <= m/4;  wn[k] = exp(-2 pi i k / n)
template <int LOGM>
__device__ __forceinline__ void load_tables(v2f* tw, v2f* wn)
{
    using G = Geo<LOGM>;
    for (int i = threadIdx.x; i < G::m - 2; i += kThreads) { const float2 t = kPassTw[i]; tw[i] = (v2f){t.x, t.y}; }
    for (int k = threadIdx.x; k <= G::m / 2; k += kThreads) { const float2 t = kWn[k << (11 - LOGM)]; wn[k] = (v2f){t.x, t.y}; }
}

// In-place decimation-in-time FFT of m = 2^LOGM points held in LDS (element i at z[zi(i)]) in BIT-REVERSED order on
// entry, natural order on exit, executed by the tpf threads lid = 0 .. tpf-1 of one frame slot (the barriers are
// workgroup-wide, every slot runs the same passes).  Two radix-2 stages are executed per pass (a radix-4 butterfly on the
// elements i0, i0+h, i0+2h, i0+3h: the same operations, in the same order per element, as two separate stages -- half
// the LDS round trips and barriers); an odd LOGM starts with one plain radix-2 stage.  INVERSE: conjugate twiddles
// (no 1/m).  Ends with a barrier.
template <int LOGM, bool INVERSE>
__device__ __forceinline__ void fft_inplace(v2f* z, const v2f* tw, int lid)
{
    using G = Geo<LOGM>;
    if (LOGM & 1) {  // stage 1: half = 1, twiddle 1
        slot_sync<G::wave_sync>();
        for (int j = lid; j < G::m / 2; j += G::tpf) {
            const int p0 = zi(2 * j), p1 = zi(2 * j + 1);
            const v2f a = z[p0], b = z[p1];
            z[p0] = a + b;
            z[p1] = a - b;
        }
    }
#pragma unroll
    for (int s = (LOGM & 1) ? 2 : 1; s <= LOGM; s += 2) {
        const int h = 1 << (s - 1);       // half size of stage s; stage s+1 has half size 2h
        slot_sync<G::wave_sync>();
        for (int j = lid; j < G::m / 4; j += G::tpf) {
            const int pos = j & (h - 1);
            const int i0 = ((j >> (s - 1)) << (s + 1)) + pos;
            const int p0 = zi(i0), p1 = zi(i0 + h), p2 = zi(i0 + 2 * h), p3 = zi(i0 + 3 * h);
            v2f w1 = tw[2 * (h - 1) + pos], w2 = tw[2 * (h - 1) + h + pos];
            if (INVERSE) { w1 = cconj(w1); w2 = cconj(w2); }
            const v2f a = z[p0], b = cmul(z[p1], w1), c = z[p2], d = cmul(z[p3], w1);
            const v2f a1 = a + b, b1 = a - b, c1 = c + d, d1 = c - d;
            const v2f c2 = cmul(c1, w2);
            // exp(-2 pi i (pos + h) / (4h)) = w2 * (-i)  (forward),  w2 * (+i)  (inverse)
            const v2f d2 = cmul(d1, INVERSE ? mul_i(w2) : mul_mi(w2));
            z[p0] = a1 + c2;
            z[p2] = a1 - c2;
            z[p1] = b1 + d2;
            z[p3] = b1 - d2;
        }
    }
    slot_sync<G::wave_sync>();
}

// windowed, end-padded, packed frame -> LDS in bit-reversed order (zeros for an idle slot)
template <int LOGM>
__device__ __forceinline__ void load_frame(const StftArgs& a, const float* src, int64_t t0, v2f* z, bool active, int lid)
{
    using G = Geo<LOGM>;
    const float2* win = reinterpret_cast<const float2*>(a.window);   // 8-byte aligned (checked by the host)
    const bool inside = active && t0 + G::n <= a.samples;            // the whole frame lies inside the clip
    const float* const s0 = src + t0;                                // frame start: 32-bit offsets from here on
    const int left = (int)min((int64_t)G::n, a.samples - t0);        // samples of the frame that exist
#pragma unroll
    for (int i = lid; i < G::m; i += G::tpf) {
        const float2 w = win[i];
        float v0, v1;
        if (inside) {
            v0 = s0[2 * i] * w.x; v1 = s0[2 * i + 1] * w.y;
        } else {                                                      // end padding: zeros (utils.py:252-275)
            v0 = (active && 2 * i < left) ? s0[2 * i] * w.x : 0.0f;
            v1 = (active && 2 * i + 1 < left) ? s0[2 * i + 1] * w.y : 0.0f;
        }
        z[zi(bitrev(i, LOGM))] = (v2f){v0, v1};
    }
}

template <int LOGM>
__global__ __launch_bounds__(kThreads) void stft_mag_forward_kernel(const StftArgs a)
{
    using G = Geo<LOGM>;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int slot = threadIdx.x / G::tpf, lid = threadIdx.x - slot * G::tpf;
    v2f* const zall = reinterpret_cast<v2f*>(smem_f);
    v2f* const z = zall + slot * G::zpoints;
    v2f* const tw = zall + G::slots * G::zpoints;
    v2f* const wn = tw + G::m;
    const float scale = 1.0f / sqrtf((float)G::n);  // normalized=True: frame_length^-0.5
    const unsigned total = (unsigned)(a.batch * a.frames), frames = (unsigned)a.frames;   // < 2^31 (host)
    load_tables<LOGM>(tw, wn);
    if constexpr (G::wave_sync) __syncthreads();   // the tables are shared by the slots, which then run wave-synchronised
    const unsigned fr = blockIdx.x * G::slots + slot;
    const bool active = fr < total;
    const unsigned b = active ? fr / frames : 0u, f = active ? fr - b * frames : 0u;
    // clip row: inline copy (clip_row() moves this kernel's code, see sot_stft_common.hpp)
    const float* src = (a.audio_b != nullptr && (int64_t)b >= a.split) ? a.audio_b + ((int64_t)b - a.split) * a.row_stride_b
                                                                      : a.audio + (int64_t)b * a.row_stride;
    load_frame<LOGM>(a, src, (int64_t)f * a.hop, z, active, lid);
    fft_inplace<LOGM, false>(z, tw, lid);
    if (active) {
        float* dst = a.mag + (int64_t)fr * G::nb;
        float2* sp = spec_row(a, b, fr, frames, G::nb);
#pragma unroll
        for (int k = lid; k <= G::m / 2; k += G::tpf) {
            v2f xk, xm;
            unpack_pair<LOGM>(z, wn, k, xk, xm);
            dst[k] = magnitude(xk) * scale;
            dst[G::m - k] = magnitude(xm) * scale;
            if (sp != nullptr) store_spec(sp, k, G::m - k, xk, xm);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same transform with PERSISTENT workgroups: a workgroup loads the twiddle tables and its threads' window
// taps once, then walks over frame groups g = blockIdx.x, blockIdx.x + gridDim.x, ...; the audio of the NEXT frame is fetched into
// registers before the passes of the current one start, so its latency (and the tables') is paid once per workgroup instead of once
// per frame.  Results are identical to stft_mag_forward_kernel's (the same operations on the same values).
// (LDS: z [slots][zi(m)] | pass twiddles [m]; the unpacking twiddles W_n^k of a thread's bins sit in registers: 16.6 KB at n_fft 2048,
// eight workgroups per CU, which the 64-VGPR budget of amdgpu_waves_per_eu(8) matches.)
template <int LOGM>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kPersistentWaves, 8))) void stft_mag_forward_persistent_kernel(const StftArgs a)
{
    using G = Geo<LOGM>;
    constexpr int PER = G::m / G::tpf;                       // packed points per thread and frame
    constexpr int PERK = (G::m / 2 + G::tpf) / G::tpf;       // bin pairs (k, m - k), k <= m/2, per thread and frame
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int slot = threadIdx.x / G::tpf, lid = threadIdx.x - slot * G::tpf;
    v2f* const zall = reinterpret_cast<v2f*>(smem_f);
    v2f* const z = zall + slot * G::zpoints;
    v2f* const tw = zall + G::slots * G::zpoints;
    v2f wnr[PERK];
#pragma unroll
    for (int j = 0; j < PERK; ++j) {
        const int k = min(lid + j * G::tpf, G::m / 2);
        const float2 t = kWn[k << (11 - LOGM)];
        wnr[j] = (v2f){t.x, t.y};
    }
    const float scale = 1.0f / sqrtf((float)G::n);
    const unsigned total = (unsigned)(a.batch * a.frames), frames = (unsigned)a.frames;
    const unsigned ngroups = (total + G::slots - 1) / G::slots;
    const float2* win = reinterpret_cast<const float2*>(a.window);
    float2 w[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) w[j] = win[lid + j * G::tpf];

    float2 cur[PER];
    // (slot fetch and spectrum row: inline copies -- as helpers they move this kernel's code, see sot_stft_common.hpp)
    auto fetch = [&](unsigned g) {   // raw samples 2i, 2i+1 of frame g*slots+slot for i = lid + j tpf; zeros outside the clip / for an idle slot
        const unsigned fr = g * G::slots + slot;
        const bool active = fr < total;
        const unsigned b = active ? fr / frames : 0u, f = active ? fr - b * frames : 0u;
        const float* src = clip_row(a, b);
        const int64_t t0 = (int64_t)f * a.hop;
        const float* const s0 = src + t0;
        const int left = active ? (int)min((int64_t)G::n, a.samples - t0) : 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = lid + j * G::tpf;
            cur[j].x = (2 * i < left) ? s0[2 * i] : 0.0f;
            cur[j].y = (2 * i + 1 < left) ? s0[2 * i + 1] : 0.0f;
        }
    };
    unsigned g = blockIdx.x;
    if (g < ngroups) fetch(g);
    for (int i = threadIdx.x; i < G::m - 2; i += kThreads) { const float2 t = kPassTw[i]; tw[i] = (v2f){t.x, t.y}; }   // load_tables() without W_n
    if constexpr (G::wave_sync) __syncthreads();
    for (; g < ngroups; g += gridDim.x) {
#pragma unroll
        for (int j = 0; j < PER; ++j)   // the products of load_frame(): sample * tap (zero * tap = 0 for the padding)
            z[zi(bitrev(lid + j * G::tpf, LOGM))] = (v2f){cur[j].x * w[j].x, cur[j].y * w[j].y};
        const unsigned fr = g * G::slots + slot;
        if (g + gridDim.x < ngroups) fetch(g + gridDim.x);   // in flight during the passes below
        fft_inplace<LOGM, false>(z, tw, lid);
        if (fr < total) {
            float* dst = a.mag + (int64_t)fr * G::nb;
            float2* sp = (a.spec != nullptr && (int64_t)(fr / frames) >= a.spec_first) ? a.spec + ((int64_t)fr - a.spec_first * frames) * G::nb : nullptr;
#pragma unroll
            for (int j = 0; j < PERK; ++j) {
                const int k = lid + j * G::tpf;
                if (k <= G::m / 2) {
                    v2f xk, xm;
                    unpack_pair_w<LOGM>(z, wnr[j], k, xk, xm);
                    dst[k] = magnitude(xk) * scale;
                    dst[G::m - k] = magnitude(xm) * scale;
                    if (sp != nullptr) store_spec(sp, k, G::m - k, xk, xm);
                }
            }
        }
        slot_sync<G::wave_sync>();   // the spectrum has been read before the next frame overwrites it
    }
}

// Backward.  With Zin_k = g_k X_k / |X_k| (k = 0 .. m) the gradient of the windowed frame is
//   y_i = Re(sum_{k=0}^{m} Zin_k e^{+2 pi i k i / n}) / sqrt(n),
// i.e. the (unnormalised) inverse real transform of the Hermitian spectrum H_k = Zin_k / 2 (0 < k < m), H_0 = Re Zin_0,
// H_m = Re Zin_m, again through a half-length complex transform:  G_k = (H_k + conj(H_{m-k})) + i conj(W) (H_k - conj(H_{m-k})),
// g = IFFT_m(G) (no 1/m), y_{2i} = Re g_i, y_{2i+1} = Im g_i.
// Pass 1 (this kernel): one frame slot per group of kFramesPerGroup consecutive frames; their windowed gradients are
// overlap-added in LDS and stored as the group's partial result.  Pass 2 (stft_overlap_add_kernel) adds, per sample, the
// partial results of the groups that cover it in ascending group order: deterministic, no atomics.
// SPEC: the frames' complex spectra come from the forward pass (StftArgs::spec_in: what the forward kernels store on request, bit for
// bit the X this kernel would recompute): no audio is read and the forward transform of every frame is skipped -- the kernel is
// the magnitude / phase arithmetic, ONE (inverse) transform per frame and the overlap-add.
template <int LOGM, bool SPEC>
__device__ __forceinline__ void backward_partial_body(const StftArgs& a)
{
    using G = Geo<LOGM>;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    constexpr int m = G::m;
    const int slot = threadIdx.x / G::tpf, lid = threadIdx.x - slot * G::tpf;
    constexpr int kPairIters = (m / 2 + 1 + G::tpf - 1) / G::tpf;   // m/2 + 1 pairs (k, m-k) over the slot's threads (3 at m/4 threads)
    v2f* const zall = reinterpret_cast<v2f*>(smem_f);
    v2f* const z = zall + slot * G::zpoints;
    v2f* const tw = zall + G::slots * G::zpoints;
    v2f* const wn = tw + m;
    float* const acc = reinterpret_cast<float*>(zall + G::lds_points) + slot * a.span;  // this group's overlap-added gradient [span]
    const float2* win = reinterpret_cast<const float2*>(a.window);
    const float scale = 1.0f / sqrtf((float)G::n);
    const float up = a.grad_scale ? *a.grad_scale : 1.0f;
    const unsigned total = (unsigned)(a.batch * a.groups), groups = (unsigned)a.groups;
    constexpr int PER = m / G::tpf;
    float2 wt[PER];   // this thread's window taps: used twice per frame (analysis and synthesis side)
#pragma unroll
    for (int j = 0; j < PER; ++j) wt[j] = win[lid + j * G::tpf];
    load_tables<LOGM>(tw, wn);
    if constexpr (G::wave_sync) __syncthreads();
    const unsigned w = blockIdx.x * G::slots + slot;
    const bool active = w < total;
    const unsigned b = active ? w / groups : 0u, grp = active ? w - b * groups : 0u;
    const float* src = a.audio + (int64_t)b * a.row_stride;
    const int64_t f_begin = (int64_t)grp * kFramesPerGroup;
    float2 cur[PER];   // raw samples of the frame about to be transformed (fetched while the frame before it is processed)
    auto fetch_audio = [&](int64_t f) {   // the persistent kernel's slot fetch: inline copy (as a helper it moves this kernel's code, see sot_stft_common.hpp)
        const int64_t t0 = f * a.hop;
        const float* const s0 = src + t0;
        const int left = (active && f < a.frames) ? (int)min((int64_t)G::n, a.samples - t0) : 0;   // zeros past the clip (utils.py:252-275)
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = lid + j * G::tpf;
            cur[j].x = (2 * i < left) ? s0[2 * i] : 0.0f;
            cur[j].y = (2 * i + 1 < left) ? s0[2 * i + 1] : 0.0f;
        }
    };
    if constexpr (!SPEC) fetch_audio(f_begin);
    for (int t = lid; t < a.span; t += G::tpf) acc[t] = 0.0f;
    for (int fi = 0; fi < kFramesPerGroup; ++fi) {
        const int64_t f = f_begin + fi;
        const bool has = active && f < a.frames;   // idle slots / missing frames run the same passes on zeros
        slot_sync<G::wave_sync>();
        if constexpr (!SPEC) {
#pragma unroll
            for (int j = 0; j < PER; ++j)
                z[zi(bitrev(lid + j * G::tpf, LOGM))] = (v2f){cur[j].x * wt[j].x, cur[j].y * wt[j].y};
            if (fi + 1 < kFramesPerGroup) fetch_audio(f + 1);
        }
        // this frame's upstream gradients: requested before the transform, consumed after it
        const float* g = a.grad_mag + ((int64_t)b * a.frames + (has ? f : 0)) * G::nb;
        float gup_k[kPairIters], gup_m[kPairIters];
#pragma unroll
        for (int r = 0; r < kPairIters; ++r) {
            const int k = lid + r * G::tpf;
            const bool use = has && k <= m / 2;
            gup_k[r] = use ? g[k] : 0.0f;
            gup_m[r] = use ? g[m - k] : 0.0f;
        }
        // the frame's spectrum: recomputed here, or the one the forward pass stored
        const float2* sp = SPEC ? a.spec_in + ((int64_t)b * a.frames + (has ? f : 0)) * G::nb : nullptr;
        v2f sxk[SPEC ? kPairIters : 1], sxm[SPEC ? kPairIters : 1];
        if constexpr (SPEC) {
#pragma unroll
            for (int r = 0; r < kPairIters; ++r) {
                const int k = lid + r * G::tpf;
                const bool use = has && k <= m / 2;
                const float2 pk = use ? sp[k] : make_float2(0.0f, 0.0f), pm = use ? sp[m - k] : make_float2(0.0f, 0.0f);
                sxk[r] = (v2f){pk.x, pk.y}; sxm[r] = (v2f){pm.x, pm.y};
            }
        } else {
            fft_inplace<LOGM, false>(z, tw, lid);
        }
        // pairs (k, m-k): spectrum -> Zin -> H -> G, kept in registers until every thread has read z
        v2f gk[kPairIters], gm[kPairIters];
#pragma unroll
        for (int r = 0; r < kPairIters; ++r) {
            const int k = lid + r * G::tpf;
            gk[r] = (v2f){0.0f, 0.0f}; gm[r] = (v2f){0.0f, 0.0f};
            if (has && k <= m / 2) {
                v2f xk, xm;
                if constexpr (SPEC) { xk = sxk[r]; xm = sxm[r]; }
                else unpack_pair<LOGM>(z, wn, k, xk, xm);
                const float mk = magnitude(xk), mm = magnitude(xm);
                const float ck = mk > 0.0f ? (gup_k[r] * up) / mk : 0.0f;      // torch: sgn(0) = 0
                const float cm = mm > 0.0f ? (gup_m[r] * up) / mm : 0.0f;
                v2f hk = (0.5f * ck) * xk, hm = (0.5f * cm) * xm;
                if (k == 0) { hk = (v2f){ck * xk.x, 0.0f}; hm = (v2f){cm * xm.x, 0.0f}; }   // H_0, H_m are real
                const v2f sk = hk + cconj(hm);      // H_k + conj(H_{m-k})
                const v2f dk = hk - cconj(hm);      // H_k - conj(H_{m-k})
                const v2f wk = wn[k];
                gk[r] = sk + mul_i(cmul(cconj(wk), dk));                 // s + i conj(W) d
                // G_{m-k} = (H_{m-k} + conj(H_k)) + i (-W) (H_{m-k} - conj(H_k)) = conj(s) + i W conj(d)
                gm[r] = cconj(sk) + mul_i(cmul(wk, cconj(dk)));
            }
        }
        if constexpr (!SPEC) slot_sync<G::wave_sync>();   // (SPEC: nobody has read z since the barrier at the top of the frame)
#pragma unroll
        for (int r = 0; r < kPairIters; ++r) {
            const int k = lid + r * G::tpf;
            if (k <= m / 2) {
                z[zi(bitrev(k, LOGM))] = gk[r];
                if (k > 0 && k < m - k) z[zi(bitrev(m - k, LOGM))] = gm[r];
            }
        }
        fft_inplace<LOGM, true>(z, tw, lid);
        if (has) {
            const int off = fi * a.hop;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int i = lid + j * G::tpf;
                const v2f v = z[zi(i)];
                acc[off + 2 * i] += wt[j].x * v.x * scale;
                acc[off + 2 * i + 1] += wt[j].y * v.y * scale;
            }
        }
    }
    slot_sync<G::wave_sync>();
    if (active) {
        float* dst = a.partial + (int64_t)w * a.span;
        for (int t = lid; t < a.span; t += G::tpf) dst[t] = acc[t];
    }
}

template <int LOGM>
__global__ __launch_bounds__(kThreads) void stft_mag_backward_partial_kernel(const StftArgs a) { backward_partial_body<LOGM, false>(a); }

template <int LOGM>
__global__ __launch_bounds__(kThreads) void stft_mag_backward_spec_kernel(const StftArgs a) { backward_partial_body<LOGM, true>(a); }

// pass 2 of every backward route but the clip kernel's: per sample, the partial results of the groups that cover it, in ascending group order
__global__ __launch_bounds__(kThreads) void stft_overlap_add_kernel(const StftArgs a)
{
    // clips over blockIdx.y; 32-bit arithmetic inside a clip (samples < 2^31 is checked by the host)
    const int samples = (int)a.samples, span = a.span, groups = (int)a.groups;
    const int gstep = kFramesPerGroup * a.hop;                  // samples between the starts of consecutive groups
    for (int64_t b = blockIdx.y; b < a.batch; b += gridDim.y) {
        const float* part = a.partial + b * (int64_t)groups * span;
        float* out = a.grad_audio + b * a.samples;
        for (int t = blockIdx.x * kThreads + threadIdx.x; t < samples; t += gridDim.x * kThreads) {
            int g_lo = (t - span + gstep) / gstep;              // first group whose span [g * gstep, g * gstep + span) holds t
            if (t - span + 1 <= 0) g_lo = 0;
            const int g_hi = min(t / gstep, groups - 1);
            float sum = 0.0f;
            for (int g = g_lo; g <= g_hi; ++g) sum += part[(int64_t)g * span + (t - g * gstep)];
            out[t] = a.accumulate ? out[t] + sum : sum;
        }
    }
}

}  // namespace sot_stft
