// sot_stft_common.hpp -- what every kernel family of the STFT-magnitude producer shares (map: csrc/sot_stft.hip): the argument block, the
// frame geometry, the committed twiddle tables, the three-rounding complex helpers, the forward kernels' row addressing, the pairwise unpacking of the real transform and |.|
// in its careful and its plain form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "sot_wave_fft.hpp"

namespace sot_stft {

constexpr int kThreads = 256;
constexpr int kFramesPerGroup = 2;  // backward: one frame slot per group of consecutive frames of a clip
constexpr int kMaxFft = 4096;

#include "sot_stft_tables.inc"      // kPassTw, kWn (csrc/gen/make_stft_tables.py)

// synchronisation of one frame slot (see Geo::wave_sync): the LDS executes a wavefront's instructions in issue order
template <bool WAVE>
__device__ __forceinline__ void slot_sync()
{
    if constexpr (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

using sot_wfft::v2f;   // one complex point; arithmetic maps to v_pk_*_f32

__device__ __forceinline__ void store_spec(float2* sp, int k, int mk, v2f xk, v2f xm)
{
    sp[k] = make_float2(xk.x, xk.y);
    sp[mk] = make_float2(xm.x, xm.y);
}

// Complex product on the packed-fp32 unit.  Round 4: the swizzled product a.yy * (-b.y, b.x) is ONE v_pk_mul_f32 whose operand halves
// are picked by op_sel and negated by neg_lo (hipcc builds the swizzled operand with v_xor + v_mov first: five instructions per product
// instead of three).  Same three roundings as the vector expression, so every result is bit-identical to rounds 2-3.  (A fused form --
// v_pk_mul + v_pk_fma, two instructions -- was measured too: its last-bit differences move rows of the SOT stage across the cutoff's
// knife edge, which the float64 yardstick test of the audio-in chain does not tolerate: 1.2e-5 -> 1.5e-4 of the gradient's peak.)
// These are the helpers of the slot and the in-place one-wavefront kernels; the kernels of sot_stft_wfft.hpp take sot_wfft's fused forms.
__device__ __forceinline__ v2f cmul(v2f a, v2f b)
{
    v2f t;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(t) : "v"(a), "v"(b));   // (-a.y b.y, a.y b.x)
    return a.xx * b + t;
}
// a * conj(b) = a.xx * (b.x, -b.y) + a.yy * (b.y, b.x)
__device__ __forceinline__ v2f cmul_conj(v2f a, v2f b)
{
    v2f t1, t2;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(t1) : "v"(a), "v"(b));   // (a.x b.x, -a.x b.y)
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(t2) : "v"(a), "v"(b));               // (a.y b.y, a.y b.x)
    return t1 + t2;
}
// a + (-i) b = (a.x + b.y, a.y - b.x)   and   a + (+i) b = (a.x - b.y, a.y + b.x): one packed add with swapped / negated halves
__device__ __forceinline__ v2f add_mi(v2f a, v2f b)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ v2f add_pi(v2f a, v2f b)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ v2f cconj(v2f a) { return (v2f){a.x, -a.y}; }
__device__ __forceinline__ v2f mul_i(v2f a) { return (v2f){-a.y, a.x}; }    // a * (+i)
__device__ __forceinline__ v2f mul_mi(v2f a) { return (v2f){a.y, -a.x}; }   // a * (-i)

// LDS index of element i of a transform buffer: one point of padding after every 32.  The bit-reversed load (lane
// stride m/2, m/4, ...) and the stride-4 accesses of the first pass would otherwise pile 32 lanes onto two banks
// (SQ_LDS_BANK_CONFLICT 72 % -> 37 % of the LDS cycles of the forward kernel).  Other paddings were no faster (n_fft 2048: one point per
// 32 22.4 / 53.0 us forward / backward, per 16 23.3 / 54.2, per 8 23.6 / 54.8, none 29.3 / 65.7).
__host__ __device__ constexpr int zi(int i)
{
    return i + (i >> 5);
}

// Frame geometry for n_fft = 2^(LOGM+1).  The frames are REAL, so each one is transformed by a complex FFT of HALF its
// length m = n_fft/2 on the packed signal z[i] = v[2i] + i v[2i+1]:   with Ze = (Z_k + conj(Z_{m-k})) / 2,
// Zo = -i/2 (Z_k - conj(Z_{m-k})), W = exp(-2 pi i k / n):   X_k = Ze + W Zo,   X_{m-k} = conj(Ze - W Zo)   (k <= m/2).
// One frame SLOT is m/4 threads (one radix-4 butterfly each per pass; at least 16); small transforms share a workgroup:
// n_fft = 64 / 128 -> 16 frames per workgroup, 256 -> 8, 512 -> 4, 1024 -> 2, 2048 and 4096 -> 1 (4096: two butterflies per thread).
// LDS: z [slots][zi(m)] | per-pass FFT twiddles [m] | W_n^k [m/2 + 2]  (| backward: overlap-add buffers [slots][span]).
template <int LOGM>
struct Geo {
    static constexpr int logm = LOGM, m = 1 << LOGM, n = 2 * m, nb = m + 1;
    // threads per frame slot: one radix-4 butterfly per thread and pass (m/4), at least 16.  Slots of at most one wavefront
    // (n_fft <= 512) synchronise with a compiler-level ordering point instead of the workgroup barrier (slot_sync): n_fft 512
    // forward 10.7 -> 10.3 us, backward 30.2 -> 28.7 us for 8192 frames.  (Shrinking the slots of n_fft 1024 / 2048 to one
    // wavefront -- 2 / 4 butterflies per thread and pass -- was measured slower: n_fft 2048 forward 24.6 -> 29.4 us, backward 53 -> 104 us.)
    static constexpr int tpf = (m / 4 > 16) ? (m / 4 > kThreads ? kThreads : m / 4) : 16;   // n_fft 4096: two butterflies per thread and pass
    static constexpr bool wave_sync = tpf <= 64;
    static constexpr int slots = kThreads / tpf;
    static constexpr int zpoints = zi(m - 1) + 2;
    static constexpr int table_points = m + m / 2 + 2;
    static constexpr size_t lds_points = (size_t)slots * zpoints + table_points;
};

__device__ __forceinline__ int bitrev(int v, int logn) { return (int)(__brev((unsigned)v) >> (32 - logn)); }

struct StftArgs {
    const float* audio; int64_t batch, samples, row_stride;
    const float* audio_b; int64_t split, row_stride_b;   // forward of two signals in one launch: clips >= split come from audio_b
    const float* window; int n_fft, logm, hop; int64_t frames;   // logm = log2(n_fft / 2)
    float* mag;                 // forward output [batch, frames, n_fft/2+1]
    float2* spec;               // forward, optional: the complex spectrum X of the clips >= spec_first, [batch - spec_first, frames, n_fft/2+1]
    int64_t spec_first;         //   (what abs()'s autograd would save: the backward then needs no second forward transform)
    const float2* spec_in;      // backward, optional: that spectrum for all `batch` clips (then `audio` is not read)
    const float* grad_mag;      // backward input, same shape
    const float* grad_scale;    // backward: optional device scalar multiplying grad_mag (an upstream gradient), or null
    int accumulate;             // backward: grad_audio += result (the sum over the scales of MSSLoss)
    float* grad_audio;          // backward output [batch, samples] (contiguous)
    float* partial;             // backward scratch [batch, groups, span]: each frame group's overlap-added gradient
    int64_t groups; int span;   // span = n_fft + hop * (kFramesPerGroup - 1)
};

// the forward kernels' addressing: clip b's audio row (pair form: the clips >= split come from audio_b) ...
__device__ __forceinline__ const float* clip_row(const StftArgs& a, unsigned b)
{
    return (a.audio_b != nullptr && (int64_t)b >= a.split) ? a.audio_b + ((int64_t)b - a.split) * a.row_stride_b : a.audio + (int64_t)b * a.row_stride;
}
// ... and where frame fr of clip b (fr = b * frames + f) stores its complex spectrum of nb bins: null when none was asked for this clip
__device__ __forceinline__ float2* spec_row(const StftArgs& a, unsigned b, unsigned fr, unsigned frames, int nb)
{
    return (a.spec != nullptr && (int64_t)b >= a.spec_first) ? a.spec + ((int64_t)fr - a.spec_first * frames) * nb : nullptr;
}

// Which kernels take these two, and which keep the expression in their own text, is decided kernel by kernel by the device assembly: a
// helper is used only where it leaves a kernel's instruction text as it was (several of these kernels meet their register budget narrowly).
//   clip_row   used by stft_mag_forward_persistent_kernel and stft_mag_forward_wave2_kernel; it moves the code of every
//              stft_mag_forward_kernel<LOGM> and of stft_mag_forward_wavew_kernel, which keep an inline copy
//   spec_row   used by every stft_mag_forward_kernel<LOGM> and stft_mag_forward_wavew_kernel; it moves the persistent and the wave2
//              forward kernel, which keep an inline copy
// Tried the same way and NOT adopted, the copies marked where they stand:
//   the 16-points-per-lane raw fetch   leaves the wave2 forward kernel unchanged but moves the wavew kernel (with the clip row inside
//              or passed in): one user is no shared helper
//   the zero-padded slot fetch         as a whole it moves the persistent kernel and stft_mag_backward_partial_kernel<6, 7, 8, 11>; its
//              loop alone leaves the persistent kernel and moves all seven recomputing backward kernels
//   wave2_load_tables in the wave2 forward kernel   moves it (sot_stft_wave2.hpp)
//   unpack_pair as a call of unpack_pair_w          moves stft_mag_forward_kernel<6, 7, 11>, the wave2 forward kernel and
//              stft_mag_backward_partial_kernel<8, 9, 10, 11> (below)

// |x| as torch's abs(complex) gives it (hypot): sqrt(re^2 + im^2) wherever the squares stay normal (a correctly rounded
// sqrt of a sum that is good to 1 ulp); the scaled hypotf when any lane of the wave holds a tiny or huge value
__device__ __forceinline__ float magnitude(v2f x)
{
    const float s = fmaf(x.x, x.x, x.y * x.y);
    const bool plain = (s > 1e-30f && s < 1e30f) || (x.x == 0.0f && x.y == 0.0f);
    if (__builtin_expect(__ballot(!plain) != 0ull, 0)) return hypotf(x.x, x.y);
    return sqrtf(s);   // (v_sqrt_f32 alone: the same time, and past the 2e-6 pin against float64)
}

// |x| for a frame whose input amplitude has been checked once (frame_is_plain below): re^2 + im^2 can neither overflow nor lose the bins
// that matter to underflow, so the per-value range test, the wave vote and the libm sqrtf (range scaling + special cases: ~20 VALU
// instructions) shrink to v_sqrt_f32, v_rsq_f32 and one Newton step on the residual (8 instructions; the result is within half an ulp of
// sqrt(s) up to the rounding of s itself, like torch's hypot-based abs(complex)); s == 0 gives 0.
__device__ __forceinline__ float magnitude_plain(v2f x)
{
    const float s = fmaf(x.x, x.x, x.y * x.y);
    const float r = __builtin_amdgcn_sqrtf(s);
    const float h = 0.5f * __builtin_amdgcn_rsqf(s);
    const float e = fmaf(-r, r, s);
    const float v = fmaf(e, h, r);
    return s == 0.0f ? 0.0f : v;
}
// amax = largest |sample * tap| of the frame.  |X_k| <= n amax, so the squares cannot overflow below 1e15; the spectrum's peak is >= amax
// (Parseval), so with amax > 1e-9 every bin within 1e-10 of the peak keeps a normal square.  An all-zero frame is plain too (every bin 0).
__device__ __forceinline__ bool frame_is_plain(float amax) { return (amax > 1e-9f && amax < 1e15f) || amax == 0.0f; }

// spectrum bins k and m-k of the real frame from the packed transform in LDS (see Geo; the slot kernels and the in-place one-wavefront
// kernels), the bin's twiddle W_n^k passed by value ...
template <int LOGM>
__device__ __forceinline__ void unpack_pair_w(const v2f* z, v2f w, int k, v2f& xk, v2f& xm)
{
    constexpr int m = 1 << LOGM;
    const v2f zk = z[zi(k)], zm = z[zi((m - k) & (m - 1))];
    const v2f ze = 0.5f * (zk + cconj(zm));
    const v2f zo = 0.5f * mul_mi(zk - cconj(zm));          // -i/2 (Z_k - conj(Z_{m-k}))
    const v2f wz = cmul(w, zo);
    xk = ze + wz;
    xm = cconj(ze - wz);
}
// ... or read from the table in LDS (its own copy of the body: as a call of unpack_pair_w it moves eight kernels, listed above)
template <int LOGM>
__device__ __forceinline__ void unpack_pair(const v2f* z, const v2f* wn, int k, v2f& xk, v2f& xm)
{
    constexpr int m = 1 << LOGM;
    const v2f zk = z[zi(k)], zm = z[zi((m - k) & (m - 1))];
    const v2f ze = 0.5f * (zk + cconj(zm));
    const v2f zo = 0.5f * mul_mi(zk - cconj(zm));
    const v2f wz = cmul(wn[k], zo);
    xk = ze + wz;
    xm = cconj(ze - wz);
}

__device__ __forceinline__ float wave_max_f32(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

}  // namespace sot_stft
