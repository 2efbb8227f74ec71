// sot_hip.hip -- MI355X (gfx950) C ABI of the 1-D spectral optimal-transport loss: the small kernels (position plan, batch mean,
// sorts), launch setup, the routing of a call to its row kernel (run_forward / run_backward, for float32 and bfloat16 rows alike), the
// bodies of the row-weight calls that the float32 and the _bf16 entry points share (forward_call ...) and the extern "C" entry points.
// The row kernels are in sot_rows.hpp (generic) and sot_full_fwd.hpp / sot_full_bwd.hpp (compile-time geometries); build.py lists the objects.
#include "sot_launch.hpp"

namespace sot {

// ---------------------------------------------------------------------------------------------
// Shared-position preparation (losses.py:287-288 for row-invariant positions): one workgroup per
// array checks sortedness and, if needed, sorts (position, index) pairs in LDS.
// ---------------------------------------------------------------------------------------------
// UNIT: the array is divided by its maximum first (trainer.py:196-197: `x_pos = x_pos / x_pos.max()` -- torch.max's NaN rule, IEEE
// division: the same floats as the two torch kernels), so that a training step that rebuilds its grid pays one launch, not four.
template <bool UNIT>
__global__ __launch_bounds__(1024) void sot_prepare_positions_kernel(
    const float* __restrict__ xpos, const float* __restrict__ ypos, int n, int m,
    float* __restrict__ sx, float* __restrict__ sy, int* __restrict__ px, int* __restrict__ py,
    int* __restrict__ ident)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int which = blockIdx.x;
    const float* pos = which ? ypos : xpos;
    const int len = which ? m : n;
    float* spos = which ? sy : sx;
    int* perm = which ? py : px;
    const int npad = sort16_npad(len), cap = (sort16_capacity(npad) + 3) & ~3;
    float* key = smem;
    int* idx = reinterpret_cast<int*>(smem + cap);
    int* const unsorted_flag = reinterpret_cast<int*>(smem + 2 * cap);  // all LDS is dynamic (16-B aligned carve)
    const int t = threadIdx.x, T = blockDim.x;
    if (t == 0) *unsorted_flag = 0;
    float top = 1.0f;
    if (UNIT) {   // max over the array: NaN wins (torch.max), otherwise order-free
        float* const part = reinterpret_cast<float*>(unsorted_flag + 1);   // 16 floats behind the flag
        float mx = -INFINITY;
        bool nan = false;
        for (int i = t; i < len; i += T) {
            const float v = pos[i];
            nan |= (v != v);
            mx = fmaxf(mx, v);
        }
        if (nan) mx = NAN;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float o = __shfl_xor(mx, off);
            mx = (mx != mx || o != o) ? NAN : fmaxf(mx, o);
        }
        if ((t & 63) == 0) part[t >> 6] = mx;
        __syncthreads();
        top = part[0];
        for (int w = 1; w < (T >> 6); ++w) {
            const float o = part[w];
            top = (top != top || o != o) ? NAN : fmaxf(top, o);
        }
    }
    for (int i = t; i < npad; i += T) {
        key[i] = (i < len) ? (UNIT ? pos[i] / top : pos[i]) : INFINITY;
        idx[i] = (i < len) ? i : INT_MAX;
    }
    __syncthreads();
    int bad = 0;
    for (int i = t; i + 1 < len; i += T) bad |= (key[i] > key[i + 1]);
    if (bad) *unsorted_flag = 1;
    __syncthreads();
    const bool need_sort = *unsorted_flag != 0;
    if (need_sort) {   // npad <= 16384 = 16 x 1024 threads: one block of 16 per thread
        const SortJob job{key, idx, len, npad}, none{nullptr, nullptr, 0, 0};
        merge_sort16_kv2<1>(job, none, t, T, [] { __syncthreads(); });
    }
    for (int i = t; i < len; i += T) { spos[i] = key[i]; perm[i] = need_sort ? idx[i] : i; }
    if (t == 0) ident[which] = need_sort ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------
// Batch mean (losses.py:203-211): optional hinge, fixed-order fp64 accumulation, one workgroup.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void sot_reduce_mean_kernel(const float* __restrict__ row_loss, int64_t B, double denom,
                                                               int apply_hinge, float hinge, float* __restrict__ mean_out,
                                                               double* __restrict__ sum_out)
{
    __shared__ double wsum[16];
    const int t = threadIdx.x;
    double acc = 0.0;
    // Fixed summation order (independent of timing): thread t accumulates rows [8t + 8192k, 8t + 8192k + 8) for k = 0, 1, ...
    // in ascending order; the loads of one chunk are independent 16-B loads, so the loop is not a chain of L2 round trips.
    const bool vec_ok = (reinterpret_cast<uintptr_t>(row_loss) & 15) == 0;
    for (int64_t base = (int64_t)t * 8; base < B; base += (int64_t)blockDim.x * 8) {
        float v[8];
        if (vec_ok && base + 8 <= B) {
            const float4 a = *reinterpret_cast<const float4*>(row_loss + base);
            const float4 b = *reinterpret_cast<const float4*>(row_loss + base + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (base + k < B) ? row_loss[base + k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float w = v[k];
            if (apply_hinge) w = (base + k < B) ? fmaxf(w - hinge, 0.0f) : 0.0f;
            acc += (double)w;
        }
    }
    acc = wave_sum(acc);
    if ((t & 63) == 0) wsum[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += wsum[w];
        if (sum_out) *sum_out = tot;
        if (mean_out) *mean_out = (float)(tot / denom);
    }
}

// data[i] *= *scalar (the upstream gradient of a loss whose gradient sot_w1d_loss_and_grad computed ahead of the backward
// pass); nothing is touched when the scalar is exactly 1 (a plain loss.backward()).
__global__ __launch_bounds__(256) void sot_scale_inplace_kernel(float* __restrict__ data, int64_t count, const float* __restrict__ scalar)
{
    const float s = *scalar;
    if (s == 1.0f) return;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t nvec = ((reinterpret_cast<uintptr_t>(data) & 15) == 0) ? count / 4 : 0;
    float4* d4 = reinterpret_cast<float4*>(data);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        float4 v = d4[i];
        v.x *= s; v.y *= s; v.z *= s; v.w *= s;
        d4[i] = v;
    }
    for (int64_t i = nvec * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) data[i] *= s;
}

// ---------------------------------------------------------------------------------------------
// Standalone segmented sort (torch.sort(keys, 1) of losses.py:287-288): one workgroup per row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void sot_segmented_sort_kernel(const float* __restrict__ keys, int64_t B, int n, int64_t stride,
                                                                 float* __restrict__ out_keys, int64_t* __restrict__ out_idx)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int npad = sort16_npad(n), cap = (sort16_capacity(npad) + 3) & ~3;
    float* key = smem;
    int* idx = reinterpret_cast<int*>(smem + cap);
    const int t = threadIdx.x, T = blockDim.x;
    const SortJob job{key, idx, n, npad}, none{nullptr, nullptr, 0, 0};
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const float* src = keys + row * stride;
        for (int i = t; i < npad; i += T) key[i] = (i < n) ? src[i] : INFINITY;
        __syncthreads();
        merge_sort16_kv2<1>(job, none, t, T, [] { __syncthreads(); });   // the launcher sizes the block so that npad <= 16 T
        for (int i = t; i < n; i += T) {
            if (out_keys) out_keys[row * (int64_t)n + i] = key[i];
            if (out_idx) out_idx[row * (int64_t)n + i] = (int64_t)min(idx[i], n - 1);   // NaN keys: a pad's index never leaves the kernel
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// The same sort, ONE WAVEFRONT per row (round 6; rows of <= 2048 keys): sot_wave_sort.hpp -- a payload-free network on one 32-bit
// word per key in registers, no workgroup barrier; a row the fast path declines (clustered / non-finite keys) is sorted by the same
// wavefront with the merge sort.  Four independent rows per 256-thread workgroup; the next row's keys are fetched while the
// current one is stored.  FAST: n == 64 KPL, rows and outputs 16-byte aligned -- no validity tests, 16-byte loads and stores.
// ---------------------------------------------------------------------------------------------
// LDS dwords of a row's key array (natural keys; the merge-sort fallback's skewed image) and of its index / scratch array (either sort's)
template <int KPL>
__host__ __device__ constexpr int wave_sort_key_cap() { return align4(sort16_capacity(sort16_npad(64 * KPL))); }
template <int KPL>
__host__ __device__ constexpr int wave_sort_idx_cap() { return align4(imax(sort16_capacity(sort16_npad(64 * KPL)), wave_sort_scratch(KPL))); }
// waves per workgroup (the segmented sort runs the network: 17.4 KB per wave, two workgroups per CU; its 16 B per key of traffic bound it)
template <int KPL>
__host__ __device__ constexpr int wave_sort_wg_waves() { return 4; }

template <int KPL, bool FAST>
__global__ __launch_bounds__(64 * wave_sort_wg_waves<KPL>(), 2) void sot_segmented_sort_wave_kernel(const float* __restrict__ keys, int64_t B, int n, int64_t stride,
                                                                         float* __restrict__ out_keys, int64_t* __restrict__ out_idx)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NPAD = 64 * KPL, KCAP = wave_sort_key_cap<KPL>(), ICAP = wave_sort_idx_cap<KPL>(), WGW = wave_sort_wg_waves<KPL>();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* key = smem + wv * (KCAP + ICAP);
    uint32_t* idx = reinterpret_cast<uint32_t*>(key + KCAP);
    const int64_t step = (int64_t)gridDim.x * WGW;
    int64_t row = (int64_t)blockIdx.x * WGW + wv;
    float x[KPL];
    auto fetch = [&](int64_t rw) {
        const float* src = keys + rw * stride;
        if constexpr (FAST) {
#pragma unroll
            for (int r = 0; r < KPL; r += 4) {
                const float4 v = *reinterpret_cast<const float4*>(src + wsort_elem<true>(r, lane));
                x[r] = v.x; x[r + 1] = v.y; x[r + 2] = v.z; x[r + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int r = 0; r < KPL; ++r) { const int e = r * 64 + lane; const float v = src[min(e, n - 1)]; x[r] = (e < n) ? v : INFINITY; }
        }
    };
    if (row < B) fetch(row);
    for (; row < B; row += step) {
        if constexpr (FAST) {
#pragma unroll
            for (int r = 0; r < KPL; r += 4) *reinterpret_cast<float4*>(key + wsort_elem<true>(r, lane)) = make_float4(x[r], x[r + 1], x[r + 2], x[r + 3]);
        } else {
#pragma unroll
            for (int r = 0; r < KPL; ++r) key[r * 64 + lane] = x[r];
        }
        row_sync<1>();
        float sk[KPL]; uint32_t si[KPL];
        const bool fast = wave_sort_kv<KPL, false, FAST, FAST>(x, key, idx, n, lane, sk, si);
        if (!fast) {   // clustered / non-finite keys: the merge sort, by this wavefront alone (nothing of the fast path is live across it)
            constexpr int MAXB = (NPAD / 16 + 63) / 64;
            const SortJob job{key, reinterpret_cast<int*>(idx), n, sort16_npad(n)}, none{nullptr, nullptr, 0, 0};
            row_sync<1>();
            merge_sort16_kv2<MAXB>(job, none, lane, 64, [] { row_sync<1>(); });
            row_sync<1>();
#pragma unroll
            for (int r = 0; r < KPL; ++r) { sk[r] = key[wsort_elem<FAST>(r, lane)]; si[r] = idx[wsort_elem<FAST>(r, lane)]; }
        }
        if (row + step < B) fetch(row + step);   // the next row's keys travel while this one is stored
        if constexpr (FAST) {
            float* ok_row = out_keys ? out_keys + row * (int64_t)n : nullptr;
            int64_t* oi_row = out_idx ? out_idx + row * (int64_t)n : nullptr;
#pragma unroll
            for (int r = 0; r < KPL; r += 4) {
                const int e = wsort_elem<true>(r, lane);
                if (ok_row) *reinterpret_cast<float4*>(ok_row + e) = make_float4(sk[r], sk[r + 1], sk[r + 2], sk[r + 3]);
                if (oi_row) {   // (NaN keys: a pad's index never leaves the kernel)
                    typedef long long ll2 __attribute__((ext_vector_type(2)));
                    ll2 a, b;
                    a.x = min((int)si[r], n - 1); a.y = min((int)si[r + 1], n - 1); b.x = min((int)si[r + 2], n - 1); b.y = min((int)si[r + 3], n - 1);
                    *reinterpret_cast<ll2*>(oi_row + e) = a;
                    *reinterpret_cast<ll2*>(oi_row + e + 2) = b;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < KPL; ++r) {
                const int e = r * 64 + lane;
                if (e < n) {
                    if (out_keys) out_keys[row * (int64_t)n + e] = sk[r];
                    if (out_idx) out_idx[row * (int64_t)n + e] = (int64_t)min((int)si[r], n - 1);
                }
            }
        }
        row_sync<1>();
    }
}

template <int KPL>
int launch_segmented_sort_wave(const float* keys, int64_t B, int n, int64_t stride, float* out_keys, int64_t* out_idx, hipStream_t s)
{
    constexpr int WGW = wave_sort_wg_waves<KPL>();
    constexpr size_t lds = (size_t)(wave_sort_key_cap<KPL>() + wave_sort_idx_cap<KPL>()) * 4 * WGW;   // waves x (key | idx)
    constexpr bool CAN_VEC = KPL % 4 == 0;
    const bool fast = CAN_VEC && n == 64 * KPL && stride % 4 == 0 && ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(out_keys) |
                                                                     reinterpret_cast<uintptr_t>(out_idx)) & 15) == 0;
    int per_cu = (int)(kLdsLimit / lds);
    if (per_cu > 16 / WGW) per_cu = 16 / WGW;
    if (per_cu < 1) per_cu = 1;
    const int grid = capped_grid((B + WGW - 1) / WGW, per_cu);
    auto go = [&](auto vec) {
        constexpr auto kern = sot_segmented_sort_wave_kernel<KPL, decltype(vec)::value>;
        allow_full_lds_once<kern>();
        (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WGW), lds, s, keys, B, n, stride, out_keys, out_idx);
    };
    if (fast) go(std::bool_constant<CAN_VEC>{});
    else go(std::false_type{});
    return launch_status();
}

// ---------------------------------------------------------------------------------------------
// Per-row positions, sorted AHEAD of the row kernels (round 6): one wavefront per row sorts the row's two position arrays with the wave
// sort (sot_wave_sort.hpp) and leaves their permutations in the [B, n + m] uint16 image the row kernels gather through (row_perm_in).
// Inside the row kernels the same network cost their other phases the registers (loop invariants spilled on paths that never sort:
// sorted rows 71 -> 90 us, backward 276 -> 348 us at 4096 x 2048, measured inlined and as a call); a kernel of its own has its own
// allocation, every wavefront of it sorts, and it needs 8.5 KB of LDS per wavefront (the transposition image; the run repair reads the
// full keys from global memory).
// An array that arrives sorted gets the identity; an array the wave sort declines (clustered / non-finite positions) is sorted by the same wavefront with
// the stable merge sort of round 4 (17.4 KB of LDS per wave are provisioned for it: the kernel's 8 waves per CU leave the room): the image is always complete.
// ---------------------------------------------------------------------------------------------

// The stable merge sort of ONE array by ONE wavefront (what a declined wave sort falls back to): a call, not inlined -- its 64 result registers stay
// out of the pre-sort kernel's hot path.  key: natural keys in LDS with +inf behind the len real ones up to sort16_npad(len); idx: scratch in, indices out.
template <int MAXB>
static __device__ __attribute__((noinline)) void wave_merge_sort_array(float* key, int* idx, int len, int lane)
{
    const SortJob job{key, idx, len, sort16_npad(len)}, none{nullptr, nullptr, 0, 0};
    row_sync<1>();
    merge_sort16_kv2<MAXB>(job, none, lane, kWave, [] { row_sync<1>(); });
    row_sync<1>();
}
constexpr int kRowposSortMaxWg = 4;
constexpr int kRowposSortWaves = 2;   // wavefronts per SIMD the pre-sort kernel is compiled for (LDS: 16.9 KB per wave of the 32-keys-per-lane form = 8 waves per CU)

// VEC: n, m multiples of 4, position rows 16-byte aligned, permutation rows 8-byte aligned (16-byte loads, 8-byte stores); FULL: n == m == 64 KPL
template <int KPL, bool FULL, bool VEC>
__global__ __launch_bounds__(256, kRowposSortWaves) void sot_rowpos_sort_kernel(const float* __restrict__ xpos, const float* __restrict__ ypos, int64_t B, int n, int m,
                                                                 int64_t xps, int64_t yps, uint16_t* __restrict__ perm)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // per wave: [idx / scratch | key]: the wave sort needs the first only (8.25 KB at 32 keys per lane); the merge-sort fallback both (17.4 KB) -- at the 8 waves
    // per CU the kernel's registers allow anyway, the CU holds that
    constexpr int ICAP = wave_sort_idx_cap<KPL>(), KCAP = wave_sort_key_cap<KPL>();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* const idx = reinterpret_cast<uint32_t*>(smem) + wv * (ICAP + KCAP);
    float* const keyl = reinterpret_cast<float*>(idx + ICAP);
    // one task = ONE array (task 2 r: the x positions of row r, 2 r + 1: its y positions): 2 B tasks spread evenly over whatever number of waves is
    // resident; an array's outcome is its own business -- sorted on arrival: the identity, sorted here (wave sort, or the merge sort when that declines): its permutation
    for (int64_t task = (int64_t)blockIdx.x * 4 + wv; task < 2 * B; task += (int64_t)gridDim.x * 4) {
        const int64_t row = task >> 1;
        const int which = (int)(task & 1);
        {
            const float* src = which ? ypos + row * yps : xpos + row * xps;
            const int len = which ? m : n;
            uint16_t* const dst = perm + row * ((int64_t)n + m) + (which ? n : 0);
            float x[KPL];
            if constexpr (VEC) {
#pragma unroll
                for (int r = 0; r < KPL; r += 4) {
                    const int e = wsort_elem<true>(r, lane);
                    const float4 v = *reinterpret_cast<const float4*>(src + (FULL ? e : min(e, len - 4)));
                    const bool real = FULL || e < len;   // whole groups of four: len % 4 == 0
                    x[r] = real ? v.x : INFINITY; x[r + 1] = real ? v.y : INFINITY; x[r + 2] = real ? v.z : INFINITY; x[r + 3] = real ? v.w : INFINITY;
                }
            } else {
#pragma unroll
                for (int r = 0; r < KPL; ++r) { const int e = r * 64 + lane; const float v = src[min(e, len - 1)]; x[r] = (e < len) ? v : INFINITY; }
            }
            // sortedness (as the row kernels test it: an element greater than its right neighbour; +inf behind the last one)
            bool unsorted = false;
            if constexpr (VEC) {   // (pads are +inf: never greater than their right neighbour)
#pragma unroll
                for (int g4 = 0; g4 < KPL; g4 += 4) {
                    // the element after this lane's four: the next lane's first; for lane 63 the first of the next block of 256 (lane 0)
                    float nxt = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x[g4]), 0x130 /* wave_shl:1 */, 0xF, 0xF, false));
                    const float wrap = (g4 + 4 < KPL) ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x[g4 + 4 < KPL ? g4 + 4 : 0]))) : INFINITY;
                    nxt = (lane == 63) ? wrap : nxt;
                    unsorted |= (x[g4] > x[g4 + 1]) | (x[g4 + 1] > x[g4 + 2]) | (x[g4 + 2] > x[g4 + 3]) | (x[g4 + 3] > nxt);
                }
            } else {
#pragma unroll
                for (int r = 0; r < KPL; ++r) {
                    float nxt = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x[r]), 0x130 /* wave_shl:1 */, 0xF, 0xF, false));
                    const float wrap = (r + 1 < KPL) ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x[r + 1 < KPL ? r + 1 : 0]))) : INFINITY;
                    nxt = (lane == 63) ? wrap : nxt;
                    unsorted |= (r * 64 + lane + 1 < len) && (x[r] > nxt);
                }
            }
            float sk[KPL]; uint32_t si[KPL];
            if (__builtin_amdgcn_ballot_w64(unsorted) == 0ull) {      // sorted on arrival: the identity
#pragma unroll
                for (int r = 0; r < KPL; ++r) si[r] = (uint32_t)wsort_elem<VEC>(r, lane);
            } else {
                const bool done = wave_sort_core<KPL, false, FULL, VEC, false>(x, [src](uint32_t i) { return src[i]; }, nullptr, idx, len, lane, sk, si);
                row_sync<1>();   // the scratch image is free again
                if (!done) {     // declined (clustered / non-finite positions; wave-uniform): the stable merge sort of round 4, by this wavefront alone
                    constexpr int NP = 64 * KPL;
#pragma unroll
                    for (int r = 0; r < KPL; ++r) keyl[wsort_elem<VEC>(r, lane)] = x[r];          // natural order; +inf behind the row (x[] holds the pads)
                    for (int e = NP + lane; e < sort16_npad(len); e += 64) keyl[e] = INFINITY;    // (never: sort16_npad(len) <= 64 KPL)
                    wave_merge_sort_array<(NP / 16 + 63) / 64>(keyl, reinterpret_cast<int*>(idx), len, lane);
#pragma unroll
                    for (int r = 0; r < KPL; ++r) si[r] = (uint32_t)min(reinterpret_cast<int*>(idx)[wsort_elem<VEC>(r, lane)], len - 1);   // (a pad's INT_MAX / NaN rows: never outside the row)
                    row_sync<1>();
                }
            }
            if constexpr (VEC) {
#pragma unroll
                for (int r = 0; r < KPL; r += 4) {
                    uint2 pk;
                    pk.x = si[r] | (si[r + 1] << 16); pk.y = si[r + 2] | (si[r + 3] << 16);
                    const int e = wsort_elem<true>(r, lane);
                    if (FULL || e < len) *reinterpret_cast<uint2*>(dst + e) = pk;   // (positions < len never hold a pad: no clamp)
                }
            } else {
#pragma unroll
                for (int r = 0; r < KPL; ++r) { const int e = r * 64 + lane; if (e < len) dst[e] = (uint16_t)min((int)si[r], len - 1); }
            }
        }
    }
}

// dest: [B, n + m] uint16.  n, m in [2, 2048].
int launch_rowpos_sort(const float* xpos, const float* ypos, int64_t B, int n, int m, int64_t xps, int64_t yps, uint16_t* dest, hipStream_t s)
{
    const int N = n > m ? n : m;
    const bool aligned = ((reinterpret_cast<uintptr_t>(xpos) | reinterpret_cast<uintptr_t>(ypos)) & 15) == 0 && (xps & 3) == 0 && (yps & 3) == 0 &&
                         (reinterpret_cast<uintptr_t>(dest) & 7) == 0 && (n & 3) == 0 && (m & 3) == 0;
    (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
    auto go = [&](auto kpl_tag, auto full, auto vec) {
        constexpr int KP = decltype(kpl_tag)::value;
        constexpr auto kern = sot_rowpos_sort_kernel<KP, decltype(full)::value, decltype(vec)::value>;
        constexpr size_t lds = (size_t)(wave_sort_idx_cap<KP>() + wave_sort_key_cap<KP>()) * 4 * 4;   // 4 waves x (idx / scratch | key)
        allow_full_lds_once<kern>();
        int per_cu = (int)(kLdsLimit / lds);
        if (per_cu > kRowposSortMaxWg) per_cu = kRowposSortMaxWg;   // four-wave workgroups: one wave of each per SIMD, at most 16 waves per CU
        hipLaunchKernelGGL(kern, dim3(capped_grid((2 * B + 3) / 4, per_cu)), dim3(256), lds, s, xpos, ypos, B, n, m, xps, yps, dest);   // one wave per array
    };
    auto pick = [&](auto kpl_tag) {
        constexpr int KP = decltype(kpl_tag)::value;
        if (aligned && n == 64 * KP && m == 64 * KP) go(kpl_tag, std::true_type{}, std::true_type{});
        else if (aligned) go(kpl_tag, std::false_type{}, std::true_type{});
        else go(kpl_tag, std::false_type{}, std::false_type{});
    };
    if (N <= 512) pick(std::integral_constant<int, 8>{});
    else if (N <= 1024) pick(std::integral_constant<int, 16>{});
    else pick(std::integral_constant<int, 32>{});
    return launch_status();
}

int launch_prepare(const float* xpos, const float* ypos, int n, int m, float* sx, float* sy, int* px, int* py, int* ident,
                          hipStream_t s, bool unit)
{
    const int npad = sort16_npad(n > m ? n : m);
    if (npad > 16 * 1024) return SOT_ERR_UNSUPPORTED_SIZE;
    const size_t prep_lds = (size_t)align4(sort16_capacity(npad)) * 8 + 16 + 64;   // + the flag's slot + 16 partial maxima
    if (prep_lds > kLdsLimit) return SOT_ERR_UNSUPPORTED_SIZE;
    (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
    auto go = [&](auto unit_tag) {
        constexpr auto kern = sot_prepare_positions_kernel<decltype(unit_tag)::value>;
        allow_full_lds_once<kern>();
        hipLaunchKernelGGL(kern, dim3(2), dim3(1024), prep_lds, s, xpos, ypos, n, m, sx, sy, px, py, ident);
    };
    if (unit) go(std::true_type{});
    else go(std::false_type{});
    return launch_status();
}

// validation, config choice, optional position preparation, persistent-grid sizing
int setup_launch(const sot_problem* pr, bool with_grad, void* workspace, size_t workspace_bytes, void* stream, Launch* out)
{
    int rc = validate(pr);
    if (rc != SOT_OK) return rc;
    Launch& l = *out;
    l.s = reinterpret_cast<hipStream_t>(stream);
    l.rowpos = pr->xpos_row_stride != 0;
    const bool need_prep = !l.rowpos && (pr->flags & SOT_FLAG_REQUIRE_SORT);
    const int n = pr->n, m = pr->m;
    int rpw = 1;
    if (!pick_cfg(n, m, l.rowpos, with_grad, &l.cfg, &l.lds, &l.block, &rpw)) return SOT_ERR_UNSUPPORTED_SIZE;

    FwdArgs a{};
    a.x = pr->x; a.y = pr->y; a.xpos = pr->xpos; a.ypos = pr->ypos;
    a.B = pr->B; a.n = n; a.m = m;
    a.xs = pr->x_row_stride; a.ys = pr->y_row_stride; a.xps = pr->xpos_row_stride; a.yps = pr->ypos_row_stride;
    a.p = pr->p; a.flags = pr->flags;
    if (l.rowpos && (pr->flags & SOT_FLAG_REQUIRE_SORT)) { a.perm_out = pr->row_perm_out; a.perm_in = pr->row_perm_in; }
    // per-row positions nobody has sorted yet: the wave-sort kernel runs first (round 6) and the row kernel gathers through its
    // permutations -- into the caller's row_perm_out, else into the workspace when it is large enough (sot_workspace_bytes), else the
    // row kernel sorts in LDS as before
    // (the domain is rowpos_presort_runs, csrc/sot_launch.hpp: the predicate sot_workspace_bytes reports room by)
    if (rowpos_presort_runs(pr)) {
        uint16_t* dest = pr->row_perm_out;
        if (dest == nullptr && workspace != nullptr && workspace_bytes >= rowpos_perm_bytes(pr->B, n, m)) dest = reinterpret_cast<uint16_t*>(workspace);
        if (dest != nullptr) {
            rc = launch_rowpos_sort(pr->xpos, pr->ypos, pr->B, n, m, pr->xpos_row_stride, pr->ypos_row_stride, dest, l.s);
            if (rc != SOT_OK) return rc;
            a.perm_in = dest; a.perm_out = nullptr;   // the image is complete: the row kernel only reads it
        }
    }

    if (need_prep && pr->perm_is_identity != nullptr) {  // caller-provided plan: positions are already sorted
        a.xperm = pr->xperm; a.yperm = pr->yperm; a.ident = pr->perm_is_identity;
    } else if (need_prep && pr->B > 0) {
        const WsLayout w = ws_layout(n, m);
        if (workspace == nullptr) return SOT_ERR_NULL_POINTER;
        if (workspace_bytes < w.total) return SOT_ERR_WORKSPACE;
        char* ws = reinterpret_cast<char*>(workspace);
        float* sx = reinterpret_cast<float*>(ws + w.sx);
        float* sy = reinterpret_cast<float*>(ws + w.sy);
        int* px = reinterpret_cast<int*>(ws + w.px);
        int* py = reinterpret_cast<int*>(ws + w.py);
        int* ident = reinterpret_cast<int*>(ws + w.ident);
        rc = launch_prepare(pr->xpos, pr->ypos, n, m, sx, sy, px, py, ident, l.s);
        if (rc != SOT_OK) return rc;
        a.xpos = sx; a.ypos = sy; a.xperm = px; a.yperm = py; a.ident = ident;
    }
    l.a = a;

    l.want = (pr->B + rpw - 1) / rpw;
    l.pm = (pr->p == 1.0f) ? 1 : ((pr->p == 2.0f) ? 2 : 0);
    // 16-B-per-lane loads need 16-B aligned rows of whole float4s
    l.vec = ((n & 3) == 0) && ((m & 3) == 0) && ((pr->x_row_stride & 3) == 0) && ((pr->y_row_stride & 3) == 0) &&
            ((reinterpret_cast<uintptr_t>(pr->x) & 15) == 0) && ((reinterpret_cast<uintptr_t>(pr->y) & 15) == 0);
    return SOT_OK;
}

// wt == Elem::bf16 (both routers): pr->x / pr->y are 16-bit rows and bf16_native(pr) holds (the caller's business: bf16_rows_call), which
// makes `full` true below; nothing ahead of the dispatch follows x or y, and the route predicates are computed once for both element types.
int run_forward(const sot_problem* pr, float* row_loss, float* uq, float* vq, float* Q, float* U, float* V,
                       bool quant, void* workspace, size_t workspace_bytes, void* stream, const MeanTail* mean_tail, Elem wt)
{
    const bool h = wt == Elem::bf16;
    Launch l;
    int rc = setup_launch(pr, false, workspace, workspace_bytes, stream, &l);
    if (rc != SOT_OK) return rc;
    if (pr->B == 0) return SOT_OK;
    l.a.row_loss = row_loss;
    if (mean_tail != nullptr && row_loss != nullptr) l.a.mt = *mean_tail;  // the batch mean comes out of this launch's last workgroup
    l.a.oUq = uq; l.a.oVq = vq; l.a.oQ = Q; l.a.oU = U; l.a.oV = V;
    // row lengths with a compile-time kernel (forward_full_supports: powers of two 512 ... 8192 and n_fft/2 + 1) take it
    const bool full = !l.rowpos && !quant && pr->n == pr->m && forward_full_supports(pr->n, l.vec) &&
                !(pr->flags & (SOT_FLAG_PRENORMALIZED | SOT_FLAG_NO_SPECIALIZE));
    // every other row length up to 8192 on shared positions: the same kernels with the length at run time (full_rt_capacity)
    const bool full_rt = !full && !l.rowpos && !quant && pr->n == pr->m && full_rt_capacity(pr->n) != 0 &&
                   !(pr->flags & (SOT_FLAG_PRENORMALIZED | SOT_FLAG_NO_SPECIALIZE));
    // per-row positions with their permutations at hand (handed in, or just written by the pre-sort kernel), 2048- / 1024- / 512-point rows: the
    // compile-time-length kernel with a position copy of its own per row (sot_full_fwd.hpp: RP)
    const bool full_rp = l.rowpos && l.a.perm_in != nullptr && !quant && (pr->n == 2048 || pr->n == 1024 || pr->n == 512) && pr->m == pr->n && l.vec && (pr->flags & SOT_FLAG_REQUIRE_SORT) &&
                   (reinterpret_cast<uintptr_t>(l.a.perm_in) & 15) == 0 && !(pr->flags & (SOT_FLAG_PRENORMALIZED | SOT_FLAG_NO_SPECIALIZE));
    if (h && !full) return SOT_ERR_BAD_SHAPE;   // (never: 16-bit rows have no other kernel)
    if (full_rp) return launch_status(dispatch_forward_full_rowpos(l.pm, l.a, l.s));
    // p = 1 on one grid shared by both measures, no cutoff: the merge-free kernel (sot_full_fwd.hpp: sot_area_full_kernel)
    const bool area = (full || full_rt) && l.pm == 1 && (pr->flags & SOT_FLAG_SAME_GRID) && !(pr->flags & (SOT_FLAG_LIMIT_Q | SOT_FLAG_NO_AREA));
    const hipError_t e = h          ? (area ? dispatch_area_full_pow2<uint16_t>(l.a, l.s) : dispatch_forward_full_pow2<uint16_t>(l.pm, l.a, l.s))
                         : area     ? (full ? dispatch_area_full(l.a, l.s) : dispatch_area_full_rt(l.a, l.s))
                         : full     ? dispatch_forward_full(l.pm, l.a, l.s)
                         : full_rt  ? dispatch_forward_full_rt(l.pm, l.a, l.s)
                         : l.rowpos ? dispatch_forward<true>(l.cfg, quant, l.pm, l.vec, l.a, l.lds, l.want, l.block, l.s)
                                    : dispatch_forward<false>(l.cfg, quant, l.pm, l.vec, l.a, l.lds, l.want, l.block, l.s);
    return launch_status(e);
}

// row_loss_out (loss-and-gradient form): the kernels that can also emit the row losses do so and *fused is set; the caller
// runs the forward kernel otherwise.  grad_row == nullptr: an upstream gradient of 1 for every row.
int run_backward(const sot_problem* pr, const float* grad_row, int64_t grad_row_stride, float grad_scale, float* gx,
                        float* gy, void* workspace, size_t workspace_bytes, void* stream, float* row_loss_out, bool* fused,
                        const MeanTail* mean_tail, Elem wt, const float* rescale)
{
    const bool h = wt == Elem::bf16;
    Launch l;
    int rc = setup_launch(pr, true, workspace, workspace_bytes, stream, &l);
    if (rc != SOT_OK) return rc;
    if (fused) *fused = false;
    if (pr->B == 0 || (gx == nullptr && gy == nullptr)) return SOT_OK;
    BwdArgs b{};
    b.f = l.a; b.grad_row = grad_row; b.grad_row_stride = grad_row_stride; b.grad_scale = grad_scale; b.gx = gx; b.gy = gy; b.rescale = rescale;
    // row lengths with a compile-time kernel take it (as in run_forward)
    const bool aligned16 = l.vec && (gx == nullptr || (reinterpret_cast<uintptr_t>(gx) & 15) == 0) &&
                           (gy == nullptr || (reinterpret_cast<uintptr_t>(gy) & 15) == 0);
    const bool full = !l.rowpos && pr->n == pr->m && backward_full_supports(pr->n, aligned16) &&
                !(pr->flags & (SOT_FLAG_PRENORMALIZED | SOT_FLAG_NO_SPECIALIZE));
    const bool full_rt = !full && !l.rowpos && pr->n == pr->m && full_rt_capacity(pr->n) != 0 && full_rt_capacity(pr->n) <= 4096 &&
                   !(pr->flags & (SOT_FLAG_PRENORMALIZED | SOT_FLAG_NO_SPECIALIZE));
    // per-row positions with their permutations at hand, 2048- / 512-point rows: the compile-time-length kernel with a position copy of its own per row
    const bool full_rp = l.rowpos && b.f.perm_in != nullptr && (pr->n == 2048 || pr->n == 512) && pr->m == pr->n && l.vec && (pr->flags & SOT_FLAG_REQUIRE_SORT) &&
                   (reinterpret_cast<uintptr_t>(b.f.perm_in) & 15) == 0 && !(pr->flags & (SOT_FLAG_PRENORMALIZED | SOT_FLAG_NO_SPECIALIZE));
    if ((full || full_rt || full_rp) && gx == nullptr && row_loss_out != nullptr) {   // the y-only full-row kernel accumulates the loss on its walk
        b.f.row_loss = row_loss_out;
        if (mean_tail != nullptr) b.f.mt = *mean_tail;
        if (fused) *fused = true;
    }
    // p = 1 on one grid, gradient w.r.t. y alone, no cutoff: the merge-free training form (sot_full_bwd.hpp: sot_area_train_kernel)
    // -- OPT-IN (SOT_FLAG_TIE_FREE_GRADIENT): at exactly tied levels it returns the derivative in the CDF values, not the reference's
    // float32 tie-order artefact
    const bool area = full && gx == nullptr && l.pm == 1 && area_train_supports(pr->n) && (pr->flags & SOT_FLAG_SAME_GRID) && (pr->flags & SOT_FLAG_TIE_FREE_GRADIENT) &&
                      !(pr->flags & (SOT_FLAG_LIMIT_Q | SOT_FLAG_NO_AREA));
    if (h && (!full || area)) return SOT_ERR_BAD_SHAPE;   // (never: 16-bit rows have no other kernel)
    const hipError_t e = h          ? dispatch_backward_full_pow2<uint16_t>(l.pm, b, l.s)
                         : area     ? dispatch_area_train(b, l.s)
                         : full_rp  ? dispatch_backward_full_rowpos(l.pm, b, l.s)
                         : full     ? dispatch_backward_full(l.pm, b, l.s)
                         : full_rt  ? dispatch_backward_full_rt(l.pm, b, l.s)
                         : l.rowpos ? dispatch_backward<true>(l.cfg, l.pm, l.vec, b, l.lds, l.want, l.block, l.s)
                                    : dispatch_backward<false>(l.cfg, l.pm, l.vec, b, l.lds, l.want, l.block, l.s);
    return launch_status(e);
}

}  // namespace sot

// =============================================================================================
// C ABI (include/sot_hip.h)
// =============================================================================================
namespace sot {
constexpr int kProfileSlots = 64;
static hipEvent_t g_prof_start[kProfileSlots], g_prof_stop[kProfileSlots];
static bool g_prof_made[kProfileSlots];
static std::mutex g_prof_mu;
static thread_local int t_prof_armed = -1;   // slot the calling thread armed for its next full-row launch

bool profile_take(hipEvent_t* start, hipEvent_t* stop)
{
    const int slot = t_prof_armed;
    if (slot < 0) return false;
    t_prof_armed = -1;
    *start = g_prof_start[slot]; *stop = g_prof_stop[slot];
    return true;
}

// The four row-weight calls, each ONE body for both element types: the argument checks of the entry point, then `body` -- on the caller's
// problem for float32, through bf16_rows_call (sot_bf16.hip) for bfloat16, which hands it the 16-bit rows where the native kernels take
// them and float32 images of them otherwise.
template <class Body>
static inline int rows_call(Elem wt, const sot_problem* prob, bool backward, void* gx, void* gy, const float* rescale, void* workspace,
                            size_t workspace_bytes, void* stream, const Body& body)
{
    if (wt == Elem::f32) return body(wt, prob, static_cast<float*>(gx), static_cast<float*>(gy), nullptr, workspace, workspace_bytes);
    return bf16_rows_call(prob, backward, static_cast<uint16_t*>(gx), static_cast<uint16_t*>(gy), rescale, workspace, workspace_bytes, stream, std::cref(body));
}

int forward_call(Elem wt, const sot_problem* prob, float* row_loss, void* workspace, size_t workspace_bytes, void* stream)
{
    if (prob != nullptr && prob->B > 0 && row_loss == nullptr) return SOT_ERR_NULL_POINTER;
    return rows_call(wt, prob, false, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream,
                     [&](Elem t, const sot_problem* pr, float*, float*, const float*, void* ws, size_t wsb) {
                         return run_forward(pr, row_loss, nullptr, nullptr, nullptr, nullptr, nullptr, false, ws, wsb, stream, nullptr, t);
                     });
}

int loss_call(Elem wt, const sot_problem* prob, float* row_loss, double denom, int apply_hinge, float hinge_threshold, float* mean_out, double* sum_out,
              uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream)
{
    if (prob != nullptr && prob->B > 0 && row_loss == nullptr) return SOT_ERR_NULL_POINTER;
    if (mean_out == nullptr && sum_out == nullptr) return SOT_ERR_NULL_POINTER;
    if (prob != nullptr && prob->B == 0) return SOT_ERR_BAD_SHAPE;  // the mean of zero rows is undefined
    const MeanTail mt = make_tail(completion_counters, denom, apply_hinge, hinge_threshold, mean_out, sum_out);
    return rows_call(wt, prob, false, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream,
                     [&](Elem t, const sot_problem* pr, float*, float*, const float*, void* ws, size_t wsb) {
                         const int rc = run_forward(pr, row_loss, nullptr, nullptr, nullptr, nullptr, nullptr, false, ws, wsb, stream,
                                                    completion_counters ? &mt : nullptr, t);
                         if (rc != SOT_OK || completion_counters != nullptr) return rc;
                         return sot_w1d_reduce_mean(row_loss, pr->B, denom, apply_hinge, hinge_threshold, mean_out, sum_out, stream);
                     });
}

int backward_call(Elem wt, const sot_problem* prob, const float* grad_row, int64_t grad_row_stride, float grad_scale, void* grad_x, void* grad_y,
                  const float* rescale, void* workspace, size_t workspace_bytes, void* stream)
{
    if (grad_row_stride != 0 && grad_row_stride != 1) return SOT_ERR_BAD_SHAPE;
    return rows_call(wt, prob, true, grad_x, grad_y, rescale, workspace, workspace_bytes, stream,
                     [&](Elem t, const sot_problem* pr, float* gx, float* gy, const float* rs, void* ws, size_t wsb) {
                         return run_backward(pr, grad_row, grad_row_stride, grad_scale, gx, gy, ws, wsb, stream, nullptr, nullptr, nullptr, t, rs);
                     });
}

int loss_and_grad_call(Elem wt, const sot_problem* prob, float* row_loss, double denom, float* mean_out, double* sum_out, float grad_scale, void* grad_y,
                       uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream)
{
    if (prob == nullptr) return SOT_ERR_NULL_POINTER;
    if (prob->B == 0) return SOT_ERR_BAD_SHAPE;  // the mean of zero rows is undefined
    if (row_loss == nullptr || grad_y == nullptr || (mean_out == nullptr && sum_out == nullptr)) return SOT_ERR_NULL_POINTER;
    const MeanTail mt = make_tail(completion_counters, denom, 0, 0.0f, mean_out, sum_out);
    const MeanTail* tail = completion_counters ? &mt : nullptr;
    return rows_call(wt, prob, true, nullptr, grad_y, nullptr, workspace, workspace_bytes, stream,
                     [&](Elem t, const sot_problem* pr, float*, float* gy, const float*, void* ws, size_t wsb) {
                         bool fused = false;   // the y-only full-row kernel writes the row losses on its walk; behind every other backward the forward kernel runs
                         int rc = run_backward(pr, nullptr, 0, grad_scale, nullptr, gy, ws, wsb, stream, row_loss, &fused, tail, t);
                         if (rc == SOT_OK && !fused) rc = run_forward(pr, row_loss, nullptr, nullptr, nullptr, nullptr, nullptr, false, ws, wsb, stream, tail, t);
                         if (rc != SOT_OK || tail != nullptr) return rc;  // (with a tail the kernel that wrote the row losses reduced them)
                         return sot_w1d_reduce_mean(row_loss, pr->B, denom, 0, 0.0f, mean_out, sum_out, stream);
                     });
}
}  // namespace sot

extern "C" {

int sot_profile_next_launch(int slot)
{
    if (slot < 0 || slot >= sot::kProfileSlots) return SOT_ERR_BAD_SHAPE;
    {
        std::lock_guard<std::mutex> lock(sot::g_prof_mu);
        if (!sot::g_prof_made[slot]) {
            if (hipEventCreate(&sot::g_prof_start[slot]) != hipSuccess || hipEventCreate(&sot::g_prof_stop[slot]) != hipSuccess) {
                (void)hipGetLastError();
                return SOT_ERR_LAUNCH;
            }
            sot::g_prof_made[slot] = true;
        }
    }
    sot::t_prof_armed = slot;
    return SOT_OK;
}

int sot_profile_elapsed_ms(int slot, float* ms)
{
    if (slot < 0 || slot >= sot::kProfileSlots || ms == nullptr || !sot::g_prof_made[slot]) return SOT_ERR_BAD_SHAPE;
    if (hipEventSynchronize(sot::g_prof_stop[slot]) != hipSuccess || hipEventElapsedTime(ms, sot::g_prof_start[slot], sot::g_prof_stop[slot]) != hipSuccess) {
        (void)hipGetLastError();
        return SOT_ERR_LAUNCH;
    }
    return SOT_OK;
}

int sot_abi_version(void) { return SOT_ABI_VERSION; }

const char* sot_status_string(int status)
{
    switch (status) {
        case SOT_OK: return "ok";
        case SOT_ERR_INVALID_P: return "The OT loss is only valid for p>=1";
        case SOT_ERR_BAD_SHAPE: return "bad shape or stride";
        case SOT_ERR_UNSUPPORTED_SIZE: return "row working set exceeds one CU's LDS (n + m too large)";
        case SOT_ERR_NULL_POINTER: return "null pointer";
        case SOT_ERR_WORKSPACE: return "workspace too small (see sot_workspace_bytes)";
        case SOT_ERR_LAUNCH: return "kernel launch failed";
        default: return "unknown status";
    }
}

size_t sot_workspace_bytes(const sot_problem* prob)
{
    if (prob == nullptr || prob->n < 1 || prob->m < 1) return 0;
    if (prob->xpos_row_stride != 0)   // per-row positions: room for the pre-sort's permutations (optional: without it the row kernel sorts in LDS)
        return sot::rowpos_presort_runs(prob) && prob->row_perm_out == nullptr   // 0 where the pre-sort cannot run (setup_launch's own predicate)
                   ? sot::rowpos_perm_bytes(prob->B, prob->n, prob->m) : 0;
    return sot::ws_layout(prob->n, prob->m).total;
}

static int prepare_positions(const float* xpos, const float* ypos, int32_t n, int32_t m, float* xpos_sorted, float* ypos_sorted,
                             int32_t* xperm, int32_t* yperm, int32_t* perm_is_identity, void* stream, bool unit)
{
    if (n < 1 || m < 1) return SOT_ERR_BAD_SHAPE;
    if (!xpos || !ypos || !xpos_sorted || !ypos_sorted || !xperm || !yperm || !perm_is_identity) return SOT_ERR_NULL_POINTER;
    return sot::launch_prepare(xpos, ypos, n, m, xpos_sorted, ypos_sorted, xperm, yperm, perm_is_identity,
                               reinterpret_cast<hipStream_t>(stream), unit);
}

int sot_prepare_positions(const float* xpos, const float* ypos, int32_t n, int32_t m, float* xpos_sorted, float* ypos_sorted,
                          int32_t* xperm, int32_t* yperm, int32_t* perm_is_identity, void* stream)
{
    return prepare_positions(xpos, ypos, n, m, xpos_sorted, ypos_sorted, xperm, yperm, perm_is_identity, stream, false);
}

int sot_prepare_unit_positions(const float* xpos, const float* ypos, int32_t n, int32_t m, float* xpos_sorted, float* ypos_sorted,
                               int32_t* xperm, int32_t* yperm, int32_t* perm_is_identity, void* stream)
{
    return prepare_positions(xpos, ypos, n, m, xpos_sorted, ypos_sorted, xperm, yperm, perm_is_identity, stream, true);
}

int sot_w1d_forward(const sot_problem* prob, float* row_loss, void* workspace, size_t workspace_bytes, void* stream)
{
    return sot::forward_call(sot::Elem::f32, prob, row_loss, workspace, workspace_bytes, stream);
}

int sot_w1d_quantiles(const sot_problem* prob, float* uq, float* vq, float* Q, float* U, float* V, void* workspace,
                      size_t workspace_bytes, void* stream)
{
    return sot::run_forward(prob, nullptr, uq, vq, Q, U, V, true, workspace, workspace_bytes, stream);
}

int sot_w1d_reduce_mean(const float* row_loss, int64_t B, double denom, int apply_hinge, float hinge_threshold, float* mean_out,
                        double* sum_out, void* stream)
{
    if (B < 0) return SOT_ERR_BAD_SHAPE;
    if (B > 0 && row_loss == nullptr) return SOT_ERR_NULL_POINTER;
    if (mean_out == nullptr && sum_out == nullptr) return SOT_ERR_NULL_POINTER;
    (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
    hipLaunchKernelGGL(sot::sot_reduce_mean_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), row_loss, B,
                       denom, apply_hinge, hinge_threshold, mean_out, sum_out);
    return sot::launch_status();
}

int sot_w1d_backward(const sot_problem* prob, const float* grad_row, int64_t grad_row_stride, float grad_scale, float* grad_x,
                     float* grad_y, void* workspace, size_t workspace_bytes, void* stream)
{
    return sot::backward_call(sot::Elem::f32, prob, grad_row, grad_row_stride, grad_scale, grad_x, grad_y, nullptr, workspace, workspace_bytes, stream);
}

int sot_w1d_loss_and_grad(const sot_problem* prob, float* row_loss, double denom, float* mean_out, double* sum_out, float grad_scale,
                          float* grad_y, uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream)
{
    return sot::loss_and_grad_call(sot::Elem::f32, prob, row_loss, denom, mean_out, sum_out, grad_scale, grad_y, completion_counters, workspace,
                                   workspace_bytes, stream);
}

int sot_scale_inplace(float* data, int64_t count, const float* scalar, void* stream)
{
    if (count < 0) return SOT_ERR_BAD_SHAPE;
    if (count == 0) return SOT_OK;
    if (data == nullptr || scalar == nullptr) return SOT_ERR_NULL_POINTER;
    const int64_t need = (count + 4 * 256 - 1) / (4 * 256);
    const int grid = (int)(need < 256 * 16 ? need : 256 * 16);
    (void)hipGetLastError();
    hipLaunchKernelGGL(sot::sot_scale_inplace_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), data, count, scalar);
    return sot::launch_status();
}

int sot_w1d_loss(const sot_problem* prob, float* row_loss, double denom, int apply_hinge, float hinge_threshold, float* mean_out,
                 double* sum_out, uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream)
{
    return sot::loss_call(sot::Elem::f32, prob, row_loss, denom, apply_hinge, hinge_threshold, mean_out, sum_out, completion_counters, workspace,
                          workspace_bytes, stream);
}

int sot_w1d_position_grad(const sot_problem* prob, const float* grad_row, int64_t grad_row_stride, float grad_scale, float* grad_xpos,
                          float* grad_ypos, void* workspace, size_t workspace_bytes, void* stream)
{
    if (grad_row_stride != 0 && grad_row_stride != 1) return SOT_ERR_BAD_SHAPE;
    return sot::run_position_grad(prob, grad_row, grad_row_stride, grad_scale, grad_xpos, grad_ypos, workspace, workspace_bytes, stream);
}

int sot_w1d_quantiles_backward(const sot_problem* prob, const float* grad_uq, const float* grad_vq, const float* grad_Q, const float* grad_U,
                               const float* grad_V, float* grad_x, float* grad_y, float* grad_xpos, float* grad_ypos, void* workspace,
                               size_t workspace_bytes, void* stream)
{
    return sot::run_quantiles_backward(prob, grad_uq, grad_vq, grad_Q, grad_U, grad_V, grad_x, grad_y, grad_xpos, grad_ypos, workspace,
                                       workspace_bytes, stream);
}

int sot_column_sum(const float* rows, int64_t B, int32_t n, int64_t row_stride, float* out, void* stream)
{
    if (B < 0 || n < 1 || row_stride < n) return SOT_ERR_BAD_SHAPE;
    if (out == nullptr || (B > 0 && rows == nullptr)) return SOT_ERR_NULL_POINTER;
    return sot::run_column_sum(rows, B, (int)n, row_stride, out, stream);
}

int sot_segmented_sort(const float* keys, int64_t B, int32_t n, int64_t row_stride, float* sorted_keys, int64_t* indices,
                       void* stream)
{
    if (B < 0 || n < 1 || row_stride < n) return SOT_ERR_BAD_SHAPE;
    if (B == 0) return SOT_OK;
    if (keys == nullptr) return SOT_ERR_NULL_POINTER;
    if (n <= 2048) {   // one wavefront per row (round 6)
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        if (n <= 128) return sot::launch_segmented_sort_wave<2>(keys, B, (int)n, row_stride, sorted_keys, indices, st);
        if (n <= 512) return sot::launch_segmented_sort_wave<8>(keys, B, (int)n, row_stride, sorted_keys, indices, st);
        if (n <= 1024) return sot::launch_segmented_sort_wave<16>(keys, B, (int)n, row_stride, sorted_keys, indices, st);
        return sot::launch_segmented_sort_wave<32>(keys, B, (int)n, row_stride, sorted_keys, indices, st);
    }
    const int npad = sot::sort16_npad((int)n);
    if (npad > 16 * 1024) return SOT_ERR_UNSUPPORTED_SIZE;   // one block of 16 elements per thread
    const size_t lds = (size_t)sot::align4(sot::sort16_capacity(npad)) * 8;
    if (lds > sot::kLdsLimit) return SOT_ERR_UNSUPPORTED_SIZE;
    sot::allow_full_lds_once<sot::sot_segmented_sort_kernel>();
    int block = 64;                                    // one thread per block of 16 elements (whole wavefronts)
    while (block < 1024 && npad > 16 * block) block <<= 1;
    int per_cu = (int)(sot::kLdsLimit / lds);
    const int wave_cap = 32 / (block / 64);            // at most 8 wavefronts per SIMD
    if (per_cu > wave_cap) per_cu = wave_cap;
    if (per_cu > 16) per_cu = 16;
    const int grid = sot::capped_grid(B, per_cu);
    (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
    hipLaunchKernelGGL(sot::sot_segmented_sort_kernel, dim3(grid), dim3(block), lds, reinterpret_cast<hipStream_t>(stream), keys, B,
                       (int)n, row_stride, sorted_keys, indices);
    return sot::launch_status();
}

}  // extern "C"
