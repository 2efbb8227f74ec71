// Time-invariant FIR filtering of [batch, samples] audio: the HIP form of the reference's ddsp.fft_convolve for a 2-D impulse
// response with padding="same" (ddsp.py:504-633 + crop_and_compensate_delay :695-734), which synths.Sinusoidal applies as the
// harmonic roll-off (synths.py:121-126: a 128-tap linear-phase filter from frequency_filter, ddsp.py:350-379).  The reference
// multiplies two 8192-point spectra; 128 taps are cheaper as a direct sum, and a direct fp32 sum is also the more accurate of
// the two.  With x zero outside [0, T):
//   forward        y[b,t]  = sum_{k<L} h[b,k] x[b, t + start - k]
//   d/d audio      gx[b,u] = sum_{k<L} h[b,k] g[b, u - start + k]    -- the same FIR with reversed taps and start' = L - 1 - start
//   d/d taps       gh[b,k] = sum_{t<T} g[b,t] x[b, t + start - k]
// (include/sot_hip.h: sot_fir_same_forward / sot_fir_same_backward; start = (L - 1) / 2 - 1 is the reference's default crop.)
//
// fir_same_kernel: one workgroup per (clip, tile of kTile consecutive outputs).  The tile and its halo are staged into LDS once
// (zero outside [0, T)), the taps next to them (already in the order the sum walks them, zero-padded to a multiple of four).
// A thread owns four consecutive outputs; per group of four taps it reads ONE new 16-byte piece of the signal and one 16-byte
// piece of the taps (the same address in every lane: an LDS broadcast) for 16 FMAs, the older piece of the 8-sample window stays
// in registers.  Every output is one fp32 fmaf chain in ascending tap order starting from 0, so its bits depend on its own row
// only -- not on the batch size, the tile it falls into or the thread that computes it.
//
// Tap gradient: fir_tap_grad_partial_kernel forms, per (clip, chunk of kChunk samples), the products in fp64 (exact for fp32
// factors) and adds them in t order into the caller's workspace [batch, chunks, L]; fir_tap_grad_finish_kernel adds the chunks in
// index order and rounds once to fp32.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sot_host.hpp"

namespace sot_fir {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kTile = SOT_FIR_TILE;            // outputs per workgroup
constexpr int kMaxTaps = 512;
constexpr int kMinTaps = 3;
constexpr int64_t kMaxSamples = 1 << 20;
constexpr int kChunk = 512;                     // samples per workgroup of the tap-gradient partial kernel
static_assert(kTile == kThreads * kPerThread, "a thread owns kPerThread consecutive outputs of the tile");
static_assert(kMaxTaps % 4 == 0 && kMaxTaps <= 2 * kThreads, "tap groups of four; the tap gradient gives a thread two taps at most");

struct FirArgs {
    const float* x;          // [batch, T] rows, x_stride floats apart
    const float* h;          // [batch, L] rows, h_stride floats apart (0: one shared filter)
    float* y;                // [batch, T] contiguous
    int64_t x_stride, h_stride;
    int T, L, start, reversed, tiles;
};

// x[q] of a row with zeros outside [0, T)
__device__ __forceinline__ float sample_or_zero(const float* __restrict__ row, int64_t q, int T)
{
    return (q >= 0 && q < T) ? row[q] : 0.0f;
}

// Stage row[g0 .. g0 + count) into dst[0 .. count) (zero outside [0, T)): 16-byte loads for the aligned pieces that lie inside
// the row, dword loads at the row's ends and for rows whose pieces straddle them.
__device__ __forceinline__ void stage_row(float* dst, const float* __restrict__ row, int64_t g0, int count, int T)
{
    const int64_t addr = (int64_t)(reinterpret_cast<uintptr_t>(row) >> 2) + g0;   // in floats; the tensors are 4-byte aligned
    const int lead = (int)(((addr % 4) + 4) % 4);                                   // floats past a 16-byte boundary at g0
    const int pieces = (count + lead + 3) / 4;
    for (int v = threadIdx.x; v < pieces; v += kThreads) {
        const int i0 = 4 * v - lead;                                                // dst index of the piece's first float
        const int64_t q = g0 + i0;
        float4 p;
        if (q >= 0 && q + 3 < T) {
            p = *reinterpret_cast<const float4*>(row + q);
        } else {
            p.x = sample_or_zero(row, q, T);
            p.y = sample_or_zero(row, q + 1, T);
            p.z = sample_or_zero(row, q + 2, T);
            p.w = sample_or_zero(row, q + 3, T);
        }
        if (i0 >= 0 && i0 + 3 < count) {
            dst[i0] = p.x; dst[i0 + 1] = p.y; dst[i0 + 2] = p.z; dst[i0 + 3] = p.w;
        } else {
            if (i0 >= 0 && i0 < count) dst[i0] = p.x;
            if (i0 + 1 >= 0 && i0 + 1 < count) dst[i0 + 1] = p.y;
            if (i0 + 2 >= 0 && i0 + 2 < count) dst[i0 + 2] = p.z;
            if (i0 + 3 >= 0 && i0 + 3 < count) dst[i0 + 3] = p.w;
        }
    }
}

__global__ __launch_bounds__(kThreads) void fir_same_kernel(FirArgs a)
{
    // xs[i] = x[tile0 + start - (Lp - 1) + i], Lp = L rounded up to four: output lo of the tile and tap k meet at xs[lo + Lp - 1 - k]
    __shared__ __attribute__((aligned(16))) float xs[kTile + kMaxTaps];
    __shared__ __attribute__((aligned(16))) float hs[kMaxTaps];
    const int b = blockIdx.x / a.tiles;
    const int tile0 = (blockIdx.x - b * a.tiles) * kTile;
    const int L = a.L, T = a.T;
    const int Lp = (L + 3) & ~3;
    const float* __restrict__ xrow = a.x + (int64_t)b * a.x_stride;
    const float* __restrict__ hrow = a.h + (int64_t)b * a.h_stride;

    for (int k = threadIdx.x; k < Lp; k += kThreads)
        hs[k] = k < L ? hrow[a.reversed ? L - 1 - k : k] : 0.0f;
    stage_row(xs, xrow, (int64_t)tile0 + a.start - (Lp - 1), kTile + Lp, T);
    __syncthreads();

    const int lo = kPerThread * threadIdx.x;
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
    // taps kg .. kg + 3 of outputs lo .. lo + 3 read xs[lo + Lp - 4 - kg + (0 .. 6)]: `hi` holds +4 .. +7, `low` +0 .. +3
    float4 hi = *reinterpret_cast<const float4*>(&xs[lo + Lp]);
    const int full = L & ~3;
    int kg = 0;
    for (; kg < full; kg += 4) {
        const float4 low = *reinterpret_cast<const float4*>(&xs[lo + Lp - 4 - kg]);
        const float4 t = *reinterpret_cast<const float4*>(&hs[kg]);
        // tap kg: outputs j = 0..3 take window entries 3 + j
        acc0 = fmaf(t.x, low.w, acc0); acc1 = fmaf(t.x, hi.x, acc1); acc2 = fmaf(t.x, hi.y, acc2); acc3 = fmaf(t.x, hi.z, acc3);
        acc0 = fmaf(t.y, low.z, acc0); acc1 = fmaf(t.y, low.w, acc1); acc2 = fmaf(t.y, hi.x, acc2); acc3 = fmaf(t.y, hi.y, acc3);
        acc0 = fmaf(t.z, low.y, acc0); acc1 = fmaf(t.z, low.z, acc1); acc2 = fmaf(t.z, low.w, acc2); acc3 = fmaf(t.z, hi.x, acc3);
        acc0 = fmaf(t.w, low.x, acc0); acc1 = fmaf(t.w, low.y, acc1); acc2 = fmaf(t.w, low.z, acc2); acc3 = fmaf(t.w, low.w, acc3);
        hi = low;
    }
    if (kg < L) {   // one to three taps left (wave-uniform): the padded taps are never multiplied
        const float4 low = *reinterpret_cast<const float4*>(&xs[lo + Lp - 4 - kg]);
        const float4 t = *reinterpret_cast<const float4*>(&hs[kg]);
        acc0 = fmaf(t.x, low.w, acc0); acc1 = fmaf(t.x, hi.x, acc1); acc2 = fmaf(t.x, hi.y, acc2); acc3 = fmaf(t.x, hi.z, acc3);
        if (kg + 1 < L) {
            acc0 = fmaf(t.y, low.z, acc0); acc1 = fmaf(t.y, low.w, acc1); acc2 = fmaf(t.y, hi.x, acc2); acc3 = fmaf(t.y, hi.y, acc3);
        }
        if (kg + 2 < L) {
            acc0 = fmaf(t.z, low.y, acc0); acc1 = fmaf(t.z, low.z, acc1); acc2 = fmaf(t.z, low.w, acc2); acc3 = fmaf(t.z, hi.x, acc3);
        }
    }

    const int t0 = tile0 + lo;
    if (t0 >= T) return;
    float* yrow = a.y + (int64_t)b * T;
    if (t0 + 3 < T && ((reinterpret_cast<uintptr_t>(yrow + t0) & 15) == 0)) {
        *reinterpret_cast<float4*>(yrow + t0) = make_float4(acc0, acc1, acc2, acc3);
    } else {
        yrow[t0] = acc0;
        if (t0 + 1 < T) yrow[t0 + 1] = acc1;
        if (t0 + 2 < T) yrow[t0 + 2] = acc2;
        if (t0 + 3 < T) yrow[t0 + 3] = acc3;
    }
}

struct TapGradArgs {
    const float* g;          // [batch, T] contiguous upstream gradient
    const float* x;          // [batch, T] rows, x_stride floats apart
    double* partial;         // [batch, chunks, L]
    float* gh;               // [batch, L]
    int64_t x_stride;
    int T, L, start, chunks;
};

__global__ __launch_bounds__(kThreads) void fir_tap_grad_partial_kernel(TapGradArgs a)
{
    // gs[i] = g[c0 + i]; xs[i] = x[c0 + start - (L - 1) + i]: sample c0 + i and tap k meet at xs[i + L - 1 - k]
    __shared__ __attribute__((aligned(16))) float gs[kChunk];
    __shared__ __attribute__((aligned(16))) float xs[kChunk + kMaxTaps];
    const int b = blockIdx.x / a.chunks;
    const int chunk = blockIdx.x - b * a.chunks;
    const int c0 = chunk * kChunk;
    const int L = a.L, T = a.T;
    const int len = T - c0 < kChunk ? T - c0 : kChunk;
    stage_row(gs, a.g + (int64_t)b * T, c0, kChunk, T);
    stage_row(xs, a.x + (int64_t)b * a.x_stride, (int64_t)c0 + a.start - (L - 1), kChunk + L - 1, T);
    __syncthreads();
    double* out = a.partial + ((int64_t)b * a.chunks + chunk) * L;
    for (int k = threadIdx.x; k < L; k += kThreads) {
        const float* xk = xs + (L - 1 - k);
        double acc = 0.0;
        for (int i = 0; i < len; ++i)
            acc += (double)gs[i] * (double)xk[i];    // the product of two floats is exact in fp64
        out[k] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void fir_tap_grad_finish_kernel(TapGradArgs a, int64_t count /* batch * L */)
{
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= count) return;
    const int64_t b = e / a.L;
    const int k = (int)(e - b * a.L);
    const double* p = a.partial + b * a.chunks * a.L + k;
    double acc = 0.0;
    for (int c = 0; c < a.chunks; ++c)
        acc += p[(int64_t)c * a.L];
    a.gh[e] = (float)acc;
}

inline int chunks_of(int64_t samples) { return (int)((samples + kChunk - 1) / kChunk); }

// the kernels' domain (include/sot_hip.h); 0 = inside
inline int check_domain(int64_t batch, int64_t samples, int taps, int start)
{
    if (batch < 0 || samples < 1 || taps < 1) return SOT_ERR_BAD_SHAPE;
    if (taps < kMinTaps || taps > kMaxTaps || samples > kMaxSamples || start < 0 || start > taps - 2) return SOT_ERR_UNSUPPORTED_SIZE;
    return SOT_OK;
}

inline int launch_fir(const float* x, int64_t x_stride, const float* h, int64_t h_stride, int64_t batch, int64_t samples, int taps,
                      int start, int reversed, float* y, hipStream_t st)
{
    FirArgs a{};
    a.x = x; a.h = h; a.y = y; a.x_stride = x_stride; a.h_stride = h_stride;
    a.T = (int)samples; a.L = taps; a.start = start; a.reversed = reversed;
    a.tiles = (int)((samples + kTile - 1) / kTile);
    hipLaunchKernelGGL(fir_same_kernel, dim3((unsigned)(batch * a.tiles)), dim3(kThreads), 0, st, a);
    return sot::launch_status();
}

}  // namespace sot_fir

extern "C" {

size_t sot_fir_workspace_bytes(int64_t batch, int64_t samples, int taps)
{
    using namespace sot_fir;
    if (batch < 1 || check_domain(batch, samples, taps, 0) != SOT_OK) return 0;
    return sizeof(double) * (size_t)batch * (size_t)chunks_of(samples) * (size_t)taps;
}

int sot_fir_same_forward(const float* audio, int64_t audio_row_stride, const float* taps, int64_t taps_row_stride, int64_t batch,
                         int64_t samples, int n_taps, int start, float* out, void* stream)
{
    using namespace sot_fir;
    if (const int rc = check_domain(batch, samples, n_taps, start)) return rc;
    if (audio_row_stride < samples || (taps_row_stride != 0 && taps_row_stride < n_taps)) return SOT_ERR_BAD_SHAPE;
    if (batch == 0) return SOT_OK;
    if (audio == nullptr || taps == nullptr || out == nullptr) return SOT_ERR_NULL_POINTER;
    if (batch * ((samples + kTile - 1) / kTile) > 0x7fffffffLL) return SOT_ERR_UNSUPPORTED_SIZE;
    (void)hipGetLastError();
    return launch_fir(audio, audio_row_stride, taps, taps_row_stride, batch, samples, n_taps, start, 0, out,
                      reinterpret_cast<hipStream_t>(stream));
}

int sot_fir_same_backward(const float* grad_out, const float* audio, int64_t audio_row_stride, const float* taps,
                          int64_t taps_row_stride, int64_t batch, int64_t samples, int n_taps, int start, float* grad_audio,
                          float* grad_taps, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace sot_fir;
    if (const int rc = check_domain(batch, samples, n_taps, start)) return rc;
    if (taps_row_stride != 0 && taps_row_stride < n_taps) return SOT_ERR_BAD_SHAPE;
    if (grad_taps != nullptr && audio_row_stride < samples) return SOT_ERR_BAD_SHAPE;
    if (batch == 0 || (grad_audio == nullptr && grad_taps == nullptr)) return SOT_OK;
    if (grad_out == nullptr || (grad_audio != nullptr && taps == nullptr) || (grad_taps != nullptr && audio == nullptr))
        return SOT_ERR_NULL_POINTER;
    if (batch * ((samples + kTile - 1) / kTile) > 0x7fffffffLL || batch * (int64_t)chunks_of(samples) > 0x7fffffffLL)
        return SOT_ERR_UNSUPPORTED_SIZE;
    if (grad_taps != nullptr) {
        if (workspace == nullptr) return SOT_ERR_NULL_POINTER;
        if (workspace_bytes < sot_fir_workspace_bytes(batch, samples, n_taps) || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
            return SOT_ERR_WORKSPACE;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (grad_audio != nullptr) {
        const int rc = launch_fir(grad_out, samples, taps, taps_row_stride, batch, samples, n_taps, n_taps - 1 - start, 1, grad_audio, st);
        if (rc != SOT_OK) return rc;
    }
    if (grad_taps != nullptr) {
        TapGradArgs a{};
        a.g = grad_out; a.x = audio; a.partial = static_cast<double*>(workspace); a.gh = grad_taps; a.x_stride = audio_row_stride;
        a.T = (int)samples; a.L = n_taps; a.start = start; a.chunks = chunks_of(samples);
        hipLaunchKernelGGL(fir_tap_grad_partial_kernel, dim3((unsigned)(batch * a.chunks)), dim3(kThreads), 0, st, a);
        const int64_t count = batch * n_taps;
        hipLaunchKernelGGL(fir_tap_grad_finish_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a, count);
        return sot::launch_status();
    }
    return SOT_OK;
}

}  // extern "C"
