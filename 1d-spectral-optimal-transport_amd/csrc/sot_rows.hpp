// sot_rows.hpp -- device side of the 1-D spectral optimal-transport row kernels (gfx950): LDS row layout, kernel argument
// blocks, the per-row context and the generic (run-time geometry) forward and backward kernel templates.  Included by every
// row-kernel object; the host side is sot_launch.hpp, the kernel objects are listed in build.py (OBJECTS).
//
// Reference semantics: losses.py:129-313 (Wasserstein1D.forward, wasserstein_1d,
// quantile_function) and utils.py:135-142 (safe_divide) of
// bernardo-torres/1d-spectral-optimal-transport; the reference composes ~25 ATen ops
// (SURVEY.md table 2.2), this file replaces them with one fused, LDS-resident pipeline per row.
//
// Data layout: x [B,n], y [B,m] fp32 row-major in HBM, read exactly once with 16-byte-per-lane
// coalesced loads; one row pair lives in LDS as four arrays U|V|PX|PY (CDFs and support
// positions, each with one sentinel slot) from staging to the final reduction; HBM traffic per
// row is 4(n+m) bytes in and 4 bytes out (the algorithmic minimum of SURVEY §8d).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <mutex>
#include <type_traits>

#include "../../include/sot_hip.h"
#include "sot_device.hpp"
#include "sot_wave_sort.hpp"

// Waves inside the partition search + merge walk (dependent LDS chains) run at raised priority so that they win issue
// slots over co-resident waves in throughput phases: measured -2.7 % kernel time (interleaved A/B, steady state).
constexpr int kWalkPrio = 1;
constexpr int kMassPrio = 2;
#define SOT_WALK_UNROLL 2  /* merge walk unroll (a #pragma needs the literal): 58.85 us against 59.45 for the compiler's x4 */

namespace sot {

// ---------------------------------------------------------------------------------------------
// LDS layout of one row group (identical arithmetic on host and device)
// ---------------------------------------------------------------------------------------------
struct RowLayout {
    int padcap;          // spare floats in front of U and of PX (front padding of the merge walk)
    int nU, nV;          // floats reserved for U (padcap + n+1 incl. sentinel) and V (m+1), multiples of 4
    int poff;            // PX = U + poff, PY = V + poff
    int part_x, part_y;  // chunk-sum scratch of the two row masses
    int colbuf;          // 2 x 32 column totals of the row masses (16-B aligned)
    int wtot;            // 2 * NW doubles (float offset, 8-B aligned)
    int red;             // NW floats + 2 floats (S_x, S_y)
    int grad;            // backward only: offset of the gradient arrays from U / V (regions mirror [U|V])
    int row_floats;      // total, multiple of 4
};

__host__ __device__ constexpr int align4(int v) { return (v + 3) & ~3; }
__host__ __device__ constexpr int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }
__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }

// merged elements handled by one thread: ceil(K / G) forced odd, so that the per-lane LDS address stride of
// the merge walk (~E/2 floats) is not a multiple of the 32-bank period on regular data
__host__ __device__ constexpr int merge_steps(int K, int G)
{
    const int e = (K + G - 1) / G;
    return e | 1;
}

__host__ __device__ constexpr RowLayout make_layout(int n, int m, int G, bool rowpos, bool with_grad = false)
{
    RowLayout L{};
    // The U and PX regions start with `padcap` spare floats: the forward walk prepends pad < E zero-valued
    // levels to U (zero width => zero contribution) so that every thread walks exactly E merged elements.
    L.padcap = align4(merge_steps(n + m, G));
    L.nU = L.padcap + align4(n + 1);
    L.nV = align4(m + 1);
    if (rowpos) {  // the per-row position sort works on power-of-two arrays in a skewed image (sot_device.hpp: sort16_capacity)
        L.nU = imax(L.nU, L.padcap + align4(sort16_capacity(sort16_npad(n))));
        L.nV = imax(L.nV, align4(sort16_capacity(sort16_npad(m))));
    }
    L.poff = L.nU + L.nV;
    const int nchx = (((n >= 8) ? (n >> 5) : 0) + 15) >> 4;
    const int nchy = (((m >= 8) ? (m >> 5) : 0) + 15) >> 4;
    L.part_x = 2 * L.poff;
    L.part_y = L.part_x + 32 * nchx;
    L.colbuf = align4(L.part_y + 32 * nchy);
    L.wtot = L.colbuf + 64;
    const int NW = G / kWave;
    L.red = L.wtot + 4 * NW;  // 2 arrays * NW doubles = 4*NW floats
    L.grad = align4(L.red + NW + 4);  // red[NW] | S_x, S_y | 1/S_x^, 1/S_y^ (guarded masses' reciprocals)
    L.row_floats = with_grad ? L.grad + L.nU + L.nV : L.grad;  // GU = U + grad, GV = V + grad
    return L;
}

// Diagnostic build only: compile ONE kernel object with -DSOT_STAMPS (build.build(extra_flags=["-DSOT_STAMPS"], only=(<object>,),
// out=...); tools/stamps.py).  Workgroup 0 stamps the shader clock at the phase boundaries of its second row into a buffer of that
// object's own (device code is not relocatable: the buffer cannot be shared across objects); no output value depends on a stamp.
// The reader below has external linkage on purpose: two objects compiled with the flag fail at link time with a duplicate symbol.
#ifdef SOT_STAMPS
static __device__ unsigned long long g_stamps[64];
extern "C" int sot_debug_read_stamps(unsigned long long* host_out, int count)   // copies the stamps to the host (synchronises)
{
    if (count > 64) count = 64;
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * count) == hipSuccess ? 0 : -1;
}
#define SOT_STAMP(i) do { if (stamp_on) { __builtin_amdgcn_sched_barrier(0); g_stamps[i] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define SOT_STAMP(i) do { } while (0)
#endif

struct FwdArgs {
    const float* x; const float* y;
    const float* xpos; const float* ypos;   // sorted positions when !ROWPOS
    const int* xperm; const int* yperm;     // shared-position sort permutations (may be null)
    const int* ident;                       // [2] device flags: permutation is the identity (may be null)
    uint16_t* perm_out; const uint16_t* perm_in;   // per-row positions: [B, n + m] sort permutations written / reused (may be null)
    int64_t B; int n, m;
    int64_t xs, ys, xps, yps;               // row strides (elements)
    float p; uint32_t flags;
    float* row_loss;
    // optional outputs of the quantile variant
    float* oUq; float* oVq; float* oQ; float* oU; float* oV;
    // CSR (ragged) input form: row r owns entries [off[r], off[r+1]) of the concatenated weights/positions;
    // n, m above are then the MAXIMUM row lengths (LDS is sized for them)
    const int64_t* xoff; const int64_t* yoff;
    // batch mean by the last workgroup to finish (sot_device.hpp: batch_mean_tail); mt.counters == nullptr: not requested
    MeanTail mt;
};

// ---------------------------------------------------------------------------------------------
// Per-row-group context shared by the forward and backward kernels
// ---------------------------------------------------------------------------------------------
template <int G>
struct RowCtx {
    static constexpr int NW = G / kWave;
    float* base; float* U; float* V; float* PX; float* PY;
    float* partx; float* party; float* colbuf; double* wtot; float* red;
    float* GU; float* GV;  // backward only
    RowLayout L;
    MassPlan mpx, mpy;
    int n, m, K, E, Ga, pad, topk;
    int t, lane, wv;
    bool sq, dn, lim, do_sort, prenorm, x_ident, y_ident;
    float p;
};

template <int G, bool ROWPOS>
__device__ __forceinline__ RowCtx<G> make_ctx(const FwdArgs& a, float* smem, bool with_grad_arrays)
{
    RowCtx<G> c;
    const int tid = threadIdx.x;
    const int rg = tid / G;
    c.t = tid - rg * G;
    c.lane = tid & (kWave - 1);
    c.wv = c.t >> 6;
    c.n = a.n; c.m = a.m;
    c.L = make_layout(a.n, a.m, G, ROWPOS, with_grad_arrays);
    c.base = smem + rg * c.L.row_floats;
    c.U = c.base + c.L.padcap; c.V = c.base + c.L.nU; c.PX = c.U + c.L.poff; c.PY = c.V + c.L.poff;
    c.partx = c.base + c.L.part_x; c.party = c.base + c.L.part_y;
    c.colbuf = c.base + c.L.colbuf;
    c.wtot = reinterpret_cast<double*>(c.base + c.L.wtot);
    c.red = c.base + c.L.red;
    c.GU = c.U + c.L.grad; c.GV = c.V + c.L.grad;  // same offset from U and from V
    c.prenorm = a.flags & SOT_FLAG_PRENORMALIZED;
    c.sq = !c.prenorm && (a.flags & SOT_FLAG_SQUARE);
    c.dn = c.prenorm || (a.flags & SOT_FLAG_DONT_NORMALIZE);
    c.lim = a.flags & SOT_FLAG_LIMIT_Q;
    c.do_sort = a.flags & SOT_FLAG_REQUIRE_SORT;
    c.p = a.p;
    c.mpx = make_mass_plan(a.n); c.mpy = make_mass_plan(a.m);
    c.K = a.n + a.m;
    c.E = merge_steps(c.K, G);
    c.Ga = (c.K + c.E - 1) / c.E;       // threads that take part in the walk
    c.pad = c.Ga * c.E - c.K;           // zero-valued levels prepended to U: 0 <= pad < E <= padcap
    c.topk = merge_steps_top(min(c.n + c.pad, c.m));
    for (int e = c.t; e < c.pad; e += G) c.U[e - c.pad] = 0.0f;
    c.x_ident = true; c.y_ident = true;
    if (!ROWPOS) {
        if (a.ident != nullptr) { c.x_ident = a.ident[0] != 0; c.y_ident = a.ident[1] != 0; }
        // issue every position load before the first LDS store (independent loads: one memory round trip, not one per
        // element), in batches of 8 per array so that any row length is covered
        for (int e0 = 0; e0 < max(c.n, c.m); e0 += 8 * G) {
            float px[8], py[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = e0 + c.t + k * G;
                px[k] = (e < c.n) ? a.xpos[e] : 0.0f;
                py[k] = (e < c.m) ? a.ypos[e] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = e0 + c.t + k * G;
                if (e < c.n) c.PX[e] = px[k];
                if (e < c.m) c.PY[e] = py[k];
            }
        }
        for (int e = c.t; e < c.pad; e += G) c.PX[e - c.pad] = a.xpos[0];  // any finite value: the width is 0
        if (c.t == 0) {
            c.PX[c.n] = a.xpos[c.n - 1];  // clamp of losses.py:220: ranks beyond the last index reuse it
            c.PY[c.m] = a.ypos[c.m - 1];
            c.U[c.n] = INFINITY;          // sentinels: an exhausted side never wins the merge
            c.V[c.m] = INFINITY;
        }
    }
    return c;
}

// per-row support sizes (CSR form): everything derived from n, m is recomputed; the LDS layout stays that of
// the maximum lengths.  E (and with it pad < E) can only shrink, so the front padding still fits.
template <int G>
__device__ __forceinline__ void set_row_lengths(RowCtx<G>& c, int n, int m)
{
    c.n = n; c.m = m;
    c.mpx = make_mass_plan(n); c.mpy = make_mass_plan(m);
    c.K = n + m;
    c.E = merge_steps(c.K, G);
    c.Ga = (c.K + c.E - 1) / c.E;
    c.pad = c.Ga * c.E - c.K;
    c.topk = merge_steps_top(min(n + c.pad, m));
}

// ---- global -> register -> LDS staging of one row (VEC: 16 B per lane, rows 16-B aligned) ------------
template <int G, int CPT, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ src, int len, int t, float (&r)[CPT])
{
    if (VEC) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int k = 0; k < CPT / 4; ++k) {
            const int q = t + k * G;
            if (4 * q < len) {
                const float4 v = s4[q];
                r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t + k * G;
            if (e < len) r[k] = src[e];
        }
    }
}

template <int G, int CPT, bool VEC>
__device__ __forceinline__ void store_row(float* dst, int len, int t, const float (&r)[CPT])
{
    if (VEC) {
        float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
        for (int k = 0; k < CPT / 4; ++k) {
            const int q = t + k * G;
            if (4 * q < len) d4[q] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t + k * G;
            if (e < len) dst[e] = r[k];
        }
    }
}

// ---- P0 (ROWPOS): this row's positions -> LDS, sorted with an index payload when REQUIRE_SORT ---------
// On return ix/iy hold, for the CPT contiguous elements this thread owns in SORTED order, their
// original column.  Ends with a barrier (U/V may be overwritten by the weights afterwards).
// MERGE: the stable merge sort of sot_device.hpp (round 4; its two 16-register output arrays cost the register-capped CSR kernel
// occupancy -- 26.5 -> 34.7 us on config 4's rows, which never need the sort -- so that instantiation keeps the bitonic network)
// perm_in (round 5): this row's two sort permutations from an earlier call on the same positions ([n + m] uint16): the sorted supports are
// GATHERED through them, nothing is sorted (the backward and position-gradient kernels of a training step).  perm_out: where this call
// leaves them.
// (An instantiation WITHOUT the sort code, launched when perm_in is given, was measured: the position-gradient kernel drops from 233 to 200
// registers -- still two waves per SIMD -- and both kernels get slower, 143.9 -> 151.5 us and 166.1 -> 173.2 us at 4096 x 2048: not kept.)
template <int G, int CPT, bool MERGE = true>
__device__ __forceinline__ void rowpos_prepare(const RowCtx<G>& c, const float* xp, const float* yp, int nmax, int mmax,
                                               int (&ix)[CPT], int (&iy)[CPT], const uint16_t* perm_in = nullptr, uint16_t* perm_out = nullptr)
{
    const int n = c.n, m = c.m, t = c.t;
    const bool gather = perm_in != nullptr && c.do_sort;   // (an image is always complete: the pre-sort kernel and the sorting row kernels both write every row)
    if (gather) {            // uniform over the threads that share barriers
        // The row's positions arrive COALESCED (element t + k G per thread), are staged in natural order in the U / V regions (free until the
        // weights arrive) and gathered from LDS through the permutation: 16 scattered 4-byte loads per thread from global memory -- up to 64
        // cache lines per wave instruction -- cost the gathering forward 83 us where rows that arrive sorted take 71 (4096 x 2048, round 6).
        float vx[CPT], vy[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t + k * G;
            vx[k] = (e < n) ? xp[e] : 0.0f;
            vy[k] = (e < m) ? yp[e] : 0.0f;
        }
        // this thread's CPT consecutive entries of each permutation: one 16-byte load where eight 16-bit entries are 16-byte aligned
        const bool vec = CPT == 8 && ((n | m) & 7) == 0 && (reinterpret_cast<uintptr_t>(perm_in) & 15) == 0;
        if (vec) {
            uint4 qx = make_uint4(0, 0, 0, 0), qy = make_uint4(0, 0, 0, 0);
            if (t * CPT < n) qx = *reinterpret_cast<const uint4*>(perm_in + t * CPT);
            if (t * CPT < m) qy = *reinterpret_cast<const uint4*>(perm_in + n + t * CPT);
            const uint32_t wx[4] = {qx.x, qx.y, qx.z, qx.w}, wy[4] = {qy.x, qy.y, qy.z, qy.w};
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int e = t * CPT + k;
                ix[k] = (e < n) ? (int)((wx[(k >> 1) & 3] >> (16 * (k & 1))) & 0xFFFFu) : e;
                iy[k] = (e < m) ? (int)((wy[(k >> 1) & 3] >> (16 * (k & 1))) & 0xFFFFu) : e;
            }
        } else {
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int e = t * CPT + k;
                ix[k] = (e < n) ? (int)perm_in[e] : e;
                iy[k] = (e < m) ? (int)perm_in[n + e] : e;
            }
        }
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t + k * G;
            if (e < n) c.U[e] = vx[k];
            if (e < m) c.V[e] = vy[k];
        }
        row_sync<G / kWave>();
        float gx[CPT], gy[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t * CPT + k;
            gx[k] = (e < n) ? c.U[min(ix[k], n - 1)] : 0.0f;     // (clamped: a stale or foreign image must not become a wild LDS address)
            gy[k] = (e < m) ? c.V[min(iy[k], m - 1)] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t * CPT + k;
            if (e < n) c.PX[e] = gx[k];
            if (e < m) c.PY[e] = gy[k];
        }
        row_sync<G / kWave>();
        if (t == 0) { c.PX[n] = c.PX[n - 1]; c.PY[m] = c.PY[m - 1]; }
        for (int e = t; e < c.pad; e += G) { c.PX[e - c.pad] = c.PX[0]; c.U[e - c.pad] = 0.0f; }
        return;
    }
    int* const IX = reinterpret_cast<int*>(c.U);  // index payloads alias U/V until the weights arrive
    int* const IY = reinterpret_cast<int*>(c.V);
    // barriers are workgroup-wide, so the sort network is sized by the maximum lengths (identical for every
    // row group of the workgroup); rows whose positions are already sorted skip it altogether
    const int npx = MERGE ? sort16_npad(nmax) : next_pow2(nmax), npy = MERGE ? sort16_npad(mmax) : next_pow2(mmax);
    int unsorted = 0;
    // The thread's CPT slots (elements t + k G) are fetched with a compile-time trip count: all loads of a row are in flight together
    // (a runtime loop waits for each element before it requests the next: sixteen L2 round trips per row at 8 elements per thread).
    float vx[CPT], vy[CPT], wx1[CPT], wy1[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int e = t + k * G;
        vx[k] = (e < n) ? xp[e] : INFINITY;
        vy[k] = (e < m) ? yp[e] : INFINITY;
        wx1[k] = (c.do_sort && e + 1 < n) ? xp[e + 1] : INFINITY;   // right neighbours for the sortedness test
        wy1[k] = (c.do_sort && e + 1 < m) ? yp[e + 1] : INFINITY;
    }
    if (c.do_sort) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t + k * G;
            if (e < npx) { c.PX[e] = vx[k]; IX[e] = (e < n) ? e : INT_MAX; }
            if (e < npy) { c.PY[e] = vy[k]; IY[e] = (e < m) ? e : INT_MAX; }
            unsorted |= (vx[k] > wx1[k]) | (vy[k] > wy1[k]);        // +inf on the right of the last element: never "unsorted"
        }
        for (int e = t + CPT * G; e < npx; e += G) { c.PX[e] = INFINITY; IX[e] = INT_MAX; }   // padding of the sort network past the slots
        for (int e = t + CPT * G; e < npy; e += G) { c.PY[e] = INFINITY; IY[e] = INT_MAX; }
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t + k * G;
            if (e < n) c.PX[e] = vx[k];
            if (e < m) c.PY[e] = vy[k];
        }
    }
    const bool need_sort = row_any<G / kWave>(unsorted != 0);  // also the barrier after the loads
    if (need_sort) {
        if constexpr (MERGE) {
            // both arrays in one barrier sequence, 16 elements per thread (sot_device.hpp: merge_sort16_kv2): npx + npy <= 2 next_pow2(G CPT), i.e.
            // one block of 16 per thread for the 8-element geometries, two for 12 / 16 elements per thread (a second, never used block
            // costs the 256 x 8 kernel 32 registers)
            constexpr int MAXB = (CPT > 8) ? 2 : 1;
            const SortJob jx{c.PX, IX, n, npx}, jy{c.PY, IY, m, npy};
            merge_sort16_kv2<MAXB>(jx, jy, t, G, [] { row_sync<G / kWave>(); });
        } else {
            bitonic_sort_kv(c.PX, IX, npx, t, G, [] { row_sync<G / kWave>(); });
            bitonic_sort_kv(c.PY, IY, npy, t, G, [] { row_sync<G / kWave>(); });
        }
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int e = t * CPT + k;
        // (clamped: a NaN position orders above the +inf pads, so a pad's index INT_MAX can surface among the first n outputs -- ADVICE r4;
        // NaN positions have no defined order here or in the reference's loss, but they must not become wild gather / store indices)
        ix[k] = (need_sort && e < n) ? min(IX[e], n - 1) : e;
        iy[k] = (need_sort && e < m) ? min(IY[e], m - 1) : e;
    }
    if (perm_out != nullptr && c.do_sort) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t * CPT + k;
            if (e < n) perm_out[e] = (uint16_t)ix[k];
            if (e < m) perm_out[n + e] = (uint16_t)iy[k];
        }
    }
    row_sync<G / kWave>();
    if (t == 0) { c.PX[n] = c.PX[n - 1]; c.PY[m] = c.PY[m - 1]; }
    for (int e = t; e < c.pad; e += G) { c.PX[e - c.pad] = c.PX[0]; c.U[e - c.pad] = 0.0f; }  // pads sit at the first position
}

// ---- P2-P3: row masses, safe_divide, weight gather, fp64-accumulated CDFs -----------------------------
// Entry: U/V hold the raw weights in ORIGINAL column order (a barrier has been passed since they were
// written).  Exit (after its final barrier): U/V hold the CDFs.  Each thread owns the CPT contiguous
// elements [t*CPT, t*CPT + CPT) of each array in sorted order; wx/wy receive their ORIGINAL (unsquared)
// weights (only consumed by the backward kernel).
// SQM: square_dist known at compile time (0 = no, 1 = yes) or read from the flags (2)
template <int G, int CPT, bool ROWPOS, int SQM = 2>
__device__ __forceinline__ void build_cdfs(const FwdArgs& a, const RowCtx<G>& c, const int (&ix)[CPT], const int (&iy)[CPT],
                                           float (&wx)[CPT], float (&wy)[CPT], float& Sx_out, float& Sy_out,
                                           const bool stamp_on = false)
{
    (void)stamp_on;
    constexpr int NW = G / kWave;
    const int n = c.n, m = c.m, t = c.t;
    float* const U = c.U; float* const V = c.V;
    const bool sq = (SQM == 2) ? c.sq : (SQM == 1);
    const int e0 = t * CPT;

    // ---- P2: row masses in ATen order (losses.py:177,184; the reference sums BEFORE it sorts, so the
    //      staged row is still in its original column order here) -----------------------------------
    float Sx = 1.0f, Sy = 1.0f;  // prenormalised: w / 1.0f == w exactly, weights enter the CDF unchanged
    float rSx = 1.0f, rSy = 1.0f;  // reciprocals of the guarded masses (computed once per row by the fold waves)
    if (!c.prenorm) {
        if (sq) {
            mass_chunk_sums<G, true>(U, c.partx, c.mpx, t);
            if (!c.dn) mass_chunk_sums<G, true>(V, c.party, c.mpy, (t + G / 2) & (G - 1));
        } else {
            mass_chunk_sums<G, false>(U, c.partx, c.mpx, t);
            if (!c.dn) mass_chunk_sums<G, false>(V, c.party, c.mpy, (t + G / 2) & (G - 1));
        }
        row_sync<G / kWave>();
        SOT_STAMP(2);
        // columns + fold by ONE wave per array (wave 0: x, wave 1: y; a single-wave row group does both
        // in its two half-waves): the 32 column totals are exchanged through this wave's own LDS slots.
        // (Doing this redundantly in every wave to save the barrier below was measured 10 % SLOWER.)
        float* const Sv = c.red + NW;
        __builtin_amdgcn_s_setprio(kMassPrio);
        if (NW >= 2) {
            if (c.wv < 2 && !(c.wv == 1 && c.dn)) {
                const float* raw = c.wv ? V : U;
                const float* part = c.wv ? c.party : c.partx;
                const MassPlan& mp = c.wv ? c.mpy : c.mpx;
                float* cb = c.colbuf + 32 * c.wv;
                if (c.lane < 32) cb[c.lane] = sq ? mass_column<true>(raw, part, mp, c.lane) : mass_column<false>(raw, part, mp, c.lane);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const float S = sq ? mass_fold<true>(raw, cb, mp.n) : mass_fold<false>(raw, cb, mp.n);
                if (c.lane == 0) { Sv[c.wv] = S; Sv[2 + c.wv] = 1.0f / guard_mass(S); }  // IEEE reciprocal, once per row
            }
        } else {
            const int half = c.lane >> 5, col = c.lane & 31;
            const bool use_y = half && !c.dn;
            const float* raw = use_y ? V : U;
            const float* part = use_y ? c.party : c.partx;
            const MassPlan& mp = use_y ? c.mpy : c.mpx;
            float* cb = c.colbuf + 32 * half;
            cb[col] = sq ? mass_column<true>(raw, part, mp, col) : mass_column<false>(raw, part, mp, col);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const float S = sq ? mass_fold<true>(raw, cb, mp.n) : mass_fold<false>(raw, cb, mp.n);
            if (col == 0) { Sv[half] = S; Sv[2 + half] = 1.0f / guard_mass(S); }
        }
        __builtin_amdgcn_s_setprio(0);
        row_sync<G / kWave>();
        SOT_STAMP(3);
        Sx = Sv[0];
        Sy = c.dn ? Sx : Sv[1];
        rSx = Sv[2];
        rSy = c.dn ? rSx : Sv[3];
    }
    Sx_out = Sx; Sy_out = Sy;

    // ---- P3: safe_divide (utils.py:135-142), weight gather by the position sort (losses.py:289-290)
    //      and fp64-accumulated CDFs (losses.py:292-293) --------------------------------------------
    const float Sxh = guard_mass(Sx);
    const float Syh = guard_mass(Sy);
    const bool x_perm = ROWPOS ? c.do_sort : !c.x_ident;
    const bool y_perm = ROWPOS ? c.do_sort : !c.y_ident;
    const bool fullx = (e0 + CPT <= n), fully = (e0 + CPT <= m);
    // identity order + full chunk: two 16-B LDS reads per array; otherwise element-wise (also the gather)
    if (!x_perm && fullx) {
#pragma unroll
        for (int k = 0; k < CPT; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(U + e0 + k);
            wx[k] = v.x; wx[k + 1] = v.y; wx[k + 2] = v.z; wx[k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = e0 + k;
            int sx = e;
            if (ROWPOS) sx = ix[k]; else if (x_perm && e < n) sx = a.xperm[e];
            wx[k] = (e < n) ? U[sx] : 0.0f;
        }
    }
    if (!y_perm && fully) {
#pragma unroll
        for (int k = 0; k < CPT; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(V + e0 + k);
            wy[k] = v.x; wy[k + 1] = v.y; wy[k + 2] = v.z; wy[k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = e0 + k;
            int sy = e;
            if (ROWPOS) sy = iy[k]; else if (y_perm && e < m) sy = a.yperm[e];
            wy[k] = (e < m) ? V[sy] : 0.0f;
        }
    }
    double px[CPT], py[CPT];
    double runx = 0.0, runy = 0.0;
    {
        // quotients: reciprocal + FMA residual correction (exact, see div_by_row_constant); the chunk is
        // redone with the IEEE sequence if an operand was small enough for the residual to underflow
        const float rx = rSx, ry = rSy;
        float qx[CPT], qy[CPT];
        uint32_t risk = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            qx[k] = div_by_row_constant(sq ? wx[k] * wx[k] : wx[k], Sxh, rx, risk);
            qy[k] = div_by_row_constant(sq ? wy[k] * wy[k] : wy[k], Syh, ry, risk);
        }
        // Rare fallback, taken by the whole wave if any lane needs it.  The ballot makes the branch wave-uniform and
        // the asm statement keeps hipcc from if-converting it (it would otherwise execute the 16 IEEE divisions
        // unconditionally and select afterwards: +176 VALU per thread per row, seen in the ISA).
        const bool slow = (risk < kFastDivMinBits) || !(Sxh <= 0x1p40f) || !(Syh <= 0x1p40f);
        if (__builtin_amdgcn_ballot_w64(slow) != 0ull) {
            asm volatile("; IEEE division fallback" ::: "memory");
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                qx[k] = (sq ? wx[k] * wx[k] : wx[k]) / Sxh;  // IEEE division (built without fast-math)
                qy[k] = (sq ? wy[k] * wy[k] : wy[k]) / Syh;
            }
        }
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const bool okx = (e0 + k < n), oky = (e0 + k < m);
            runx += okx ? (double)qx[k] : 0.0;
            runy += oky ? (double)qy[k] : 0.0;
            px[k] = runx;
            py[k] = runy;
        }
    }
    const double inx = wave_incl_scan(runx), iny = wave_incl_scan(runy);
    double exx = wave_shift_right1(inx), exy = wave_shift_right1(iny);
    if (NW > 1 && c.lane == kWave - 1) { c.wtot[c.wv] = inx; c.wtot[NW + c.wv] = iny; }
    SOT_STAMP(4);
    row_sync<G / kWave>();  // every raw weight has been read (also through permutations) before U/V are rewritten
    if (NW > 1) {
        double ox = 0.0, oy = 0.0;
        for (int w = 0; w < c.wv; ++w) { ox += c.wtot[w]; oy += c.wtot[NW + w]; }
        exx += ox;
        exy += oy;
    }
    if (fullx) {
#pragma unroll
        for (int k = 0; k < CPT; k += 4)
            *reinterpret_cast<float4*>(U + e0 + k) = make_float4((float)(exx + px[k]), (float)(exx + px[k + 1]),
                                                                 (float)(exx + px[k + 2]), (float)(exx + px[k + 3]));
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) if (e0 + k < n) U[e0 + k] = (float)(exx + px[k]);
    }
    if (fully) {
#pragma unroll
        for (int k = 0; k < CPT; k += 4)
            *reinterpret_cast<float4*>(V + e0 + k) = make_float4((float)(exy + py[k]), (float)(exy + py[k + 1]),
                                                                 (float)(exy + py[k + 2]), (float)(exy + py[k + 3]));
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) if (e0 + k < m) V[e0 + k] = (float)(exy + py[k]);
    }
    if (ROWPOS && t == 0) { U[n] = INFINITY; V[m] = INFINITY; }
    __builtin_amdgcn_s_setprio(0);
    row_sync<G / kWave>();
}

// left rank of q in a sorted LDS array: #{A_i < q}  (torch.searchsorted side='left', losses.py:219)
__device__ __forceinline__ int lower_rank(const float* A, int len, float q)
{
    int lo = 0, hi = len;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (A[mid] < q) lo = mid + 1; else hi = mid; }
    return lo;
}

// ---------------------------------------------------------------------------------------------
// Forward kernel.
//   G      threads per row (a whole number of wavefronts); 256-thread workgroups hold 256/G rows
//   CPT    contiguous elements of each array owned by a thread during the scan (G*CPT >= max(n,m))
//   ROWPOS positions differ per row (sorted in LDS when REQUIRE_SORT)
//   QUANT  also emit the return_quantiles tensors
//   PM     cost specialisation: 1 -> p == 1, 2 -> p == 2, 0 -> powf
//   LIM    limit_quantile_range: levels Q_k > 1 contribute nothing
//   VEC    rows are 16-B aligned and n, m multiples of 4: 16-B-per-lane global loads
//   SQM    square_dist at compile time (0 / 1) in the specialised p = 1 / p = 2 variants (-2.8 % kernel time), 2 = runtime flag
// Row pipeline: the NEXT row's weights are fetched into registers while the current row is being
// processed in LDS, so HBM latency overlaps the scan/merge work of the same workgroup.
// ---------------------------------------------------------------------------------------------
// Register cap (waves per SIMD) of the one-wave-per-row CSR kernel: 146 VGPRs = three waves per SIMD without it; compiled for four
// (128 VGPRs) config 4's 8192 ragged rows take 30.8 instead of 33.0 us (five: 42.4, six: 56.5 -- spills).  The dense generic kernels
// keep their registers: the same cap on 8192 x 1000 costs 46 -> 58 us (12 elements per thread spill).
constexpr int kCsrMinWaves = 4;
// Register cap of the per-row-position FORWARD kernels on 256-thread workgroups (the in-register block sort of merge_sort16_kv2 pushes them
// to 168 ... 212 VGPRs = two waves per SIMD, i.e. two of the four workgroups the LDS would hold): kRowposMinWaves waves per SIMD (7 dwords
// spilled).  Measured 4096 x 2048 paper mode: unsorted rows 246 -> 192 us, sorted rows 77 -> 63 us (one sort block per thread + the cap).
constexpr int kRowposMinWaves = 3;
// (The generic shared-position kernels of the 2048-point geometry also sit just above a register step in some instantiations -- forward 129 ... 140
// VGPRs, backward 176 -- but holding them to the step changes nothing: forward 52.8 vs 52.8 us, both-gradient backward 120.1 vs 119.7 us at 8192 x 2048.)
template <int G, int CPT, bool ROWPOS, bool QUANT, int PM, bool LIM, bool VEC, bool CSR = false, int SQM = 2>
__global__ __launch_bounds__((G < 256 ? 256 : G), ((CSR && G == 64) ? kCsrMinWaves : (ROWPOS && !CSR && G <= 256 && CPT == 8) ? kRowposMinWaves : 1)) void sot_forward_kernel(const FwdArgs a)
{
    static_assert(!CSR || (ROWPOS && !VEC && !QUANT), "the CSR form has per-row positions and unaligned rows");
    constexpr int BLOCK = (G < 256 ? 256 : G);
    constexpr int RPW = BLOCK / G;   // rows processed concurrently by one workgroup
    constexpr int NW = G / kWave;    // wavefronts per row
    extern __shared__ __attribute__((aligned(16))) float smem[];
#ifdef SOT_STAMPS
    const bool wg_stamp = (threadIdx.x == 0) && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1);
    unsigned long long* const wgs = g_stamps + (blockIdx.x == 0 ? 32 : 48);
    int wg_row = 0;
    if (wg_stamp) wgs[0] = __builtin_readcyclecounter();
#endif
    RowCtx<G> c = make_ctx<G, ROWPOS>(a, smem, false);
    const int rg = threadIdx.x / G;
    const int t = c.t;
    float* const U = c.U; float* const V = c.V; float* const PX = c.PX; float* const PY = c.PY;

    const int64_t row_step = (int64_t)gridDim.x * RPW;
    int64_t row0 = (int64_t)blockIdx.x * RPW;
    float rx[CPT], ry[CPT];
    if (!CSR && row0 < a.B) {
        const int64_t r = min(row0 + rg, a.B - 1);
        load_row<G, CPT, VEC>(a.x + r * a.xs, c.n, t, rx);
        load_row<G, CPT, VEC>(a.y + r * a.ys, c.m, t, ry);
    }
#ifdef SOT_STAMPS
    if (wg_stamp) wgs[1] = __builtin_readcyclecounter();
#endif
    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rg;
        const bool valid = row < a.B;
        const int64_t rowc = valid ? row : a.B - 1;
#ifdef SOT_STAMPS
        const bool stamp_on = (blockIdx.x == 0) && (threadIdx.x == 0) && (row0 == row_step);
#endif
        SOT_STAMP(0);
        const float* xp = nullptr; const float* yp = nullptr;
        bool bad_row = false;  // CSR: empty or over-long support -> NaN
        if (CSR) {
            const int64_t xo = a.xoff[rowc], xe = a.xoff[rowc + 1], yo = a.yoff[rowc], ye = a.yoff[rowc + 1];
            const int64_t nr = xe - xo, mr = ye - yo;
            bad_row = (nr < 1) || (mr < 1) || (nr > a.n) || (mr > a.m);
            set_row_lengths(c, bad_row ? 1 : (int)nr, bad_row ? 1 : (int)mr);
            const int64_t xb = bad_row ? 0 : xo, yb = bad_row ? 0 : yo;  // entry 0 exists (nnz >= 1 is checked on the host)
            xp = a.xpos + xb; yp = a.ypos + yb;
            load_row<G, CPT, false>(a.x + xb, c.n, t, rx);
            load_row<G, CPT, false>(a.y + yb, c.m, t, ry);
        } else if (ROWPOS) {
            xp = a.xpos + rowc * a.xps; yp = a.ypos + rowc * a.yps;
        }
        const int n = c.n, m = c.m, K = c.K;
        int ix[CPT], iy[CPT];
        if (ROWPOS) {
            const int64_t pw = (int64_t)a.n + a.m;
            rowpos_prepare<G, CPT, !CSR>(c, xp, yp, a.n, a.m, ix, iy, (!CSR && a.perm_in) ? a.perm_in + rowc * pw : nullptr,
                                         (!CSR && a.perm_out && valid) ? a.perm_out + rowc * pw : nullptr);
        }
        // ---- P1: registers -> LDS (original column order), then fetch the next row into the registers --
        store_row<G, CPT, VEC>(U, n, t, rx);
        store_row<G, CPT, VEC>(V, m, t, ry);
        if (!CSR && row0 + row_step < a.B) {
            const int64_t r = min(row0 + row_step + rg, a.B - 1);
            load_row<G, CPT, VEC>(a.x + r * a.xs, n, t, rx);
            load_row<G, CPT, VEC>(a.y + r * a.ys, m, t, ry);
        }
        row_sync<G / kWave>();
        SOT_STAMP(1);
        float wx[CPT], wy[CPT];
        float Sx, Sy;
#ifdef SOT_STAMPS
        build_cdfs<G, CPT, ROWPOS, SQM>(a, c, ix, iy, wx, wy, Sx, Sy, stamp_on);
#else
        build_cdfs<G, CPT, ROWPOS, SQM>(a, c, ix, iy, wx, wy, Sx, Sy);
#endif
        SOT_STAMP(5);

        // ---- P4: merge of the two CDFs = sort(cat(U,V)) + searchsorted + take_along_dim -----------
        //      (losses.py:295-298), level widths, cutoff mask, |.|^p, weighted sum (:301-313)
        float acc = 0.0f;
        __builtin_amdgcn_s_setprio(kWalkPrio);
        if (t < c.Ga) {
            // Walk over (Uw, V) where Uw = pad zero levels ++ U: exactly E steps for every thread.
            const float* const Uw = U - c.pad;
            const float* const PXw = PX - c.pad;
            const int nw = n + c.pad;
            const int D0 = t * c.E;
            const uint32_t ub1 = lds_addr(Uw) - 4u;  // partition search on LDS byte addresses (merge_path_steps32)
            const int i0 = (int)((merge_path_steps32(ub1, lds_addr(V) + 4u * (uint32_t)D0 + ub1, nw, m, D0, c.topk) - ub1) >> 2);
            SOT_STAMP(6);
            const int j0 = D0 - i0;
            float qprev = 0.0f;  // Q_0 := 0 (the pad of losses.py:301)
            if (i0 > 0) qprev = Uw[i0 - 1];
            if (j0 > 0) qprev = fmaxf(qprev, V[j0 - 1]);
            float ua = Uw[i0], vb = V[j0], xa = PXw[i0], yb = PY[j0];
            // Byte offsets from Uw: Uw[i] at 4i; V[j] at 4(voff + j) with i + j = k => 4(voff + k) - 4i.
            const char* const lb = reinterpret_cast<const char*>(Uw);
            const uint32_t poff4 = 4u * (uint32_t)c.L.poff;
            const int voff = (int)(V - Uw);
            uint32_t iu = (uint32_t)i0;
            if (!QUANT) {
                // "Loser" form of the two-way merge (see sot_full_fwd.hpp: merge_walk_full): (w, wp) is the head fetched last, (r, rp) the
                // head that lost the previous comparison; only the consumed head's stream is read again, so the fetched
                // level and position become the new (w, wp) without a select.  Equal heads may be consumed in either
                // order: the pair of heads, hence the consumed level, its width and its cost factor, is the same, and the
                // second member of a tie has zero width -- the sum is bit-identical to the canonical order's.
                float w = ua, wp = xa, r = vb, rp = yb;
                const uint32_t lb32 = lds_addr(lb);  // 32-bit LDS addresses: one VGPR per stream, no re-basing add per access
                uint32_t pw = lb32 + 4u * (uint32_t)i0 + 4u, pr = lb32 + 4u * (uint32_t)(voff + j0) + 4u;
#pragma unroll SOT_WALK_UNROLL
                for (int s = 0; s < c.E; ++s) {
                    const bool cw = w <= r;
                    const float q = cw ? w : r;
                    const float cost = transport_cost<PM>(wp, rp, c.p);
                    float delta = q - qprev;
                    if (LIM && q > 1.0f) delta = 0.0f;
                    acc = fmaf(delta, cost, acc);  // fused: no worse than the reference's separate rounding
                    qprev = q;
                    const uint32_t nx = cw ? pw : pr;
                    pr = cw ? pr : pw;
                    pw = nx + 4u;
                    r = cw ? r : w;
                    rp = cw ? rp : wp;
                    w = lds_load(nx);
                    wp = lds_load(nx + poff4);
                }
            } else
#pragma unroll SOT_WALK_UNROLL
            for (int s = 0; s < c.E; ++s) {
                const bool tu = ua <= vb;
                const float q = tu ? ua : vb;
                const float cost = transport_cost<PM>(xa, yb, c.p);
                float delta = q - qprev;
                if (LIM && q > 1.0f) delta = 0.0f;
                acc = fmaf(delta, cost, acc);  // fused: no worse than the reference's separate rounding
                if (QUANT && valid) {
                    const int k = D0 + s - c.pad;  // index among the real merged levels
                    if (k >= 0) {
                        const int64_t o = row * (int64_t)K + k;
                        if (a.oQ) a.oQ[o] = q;
                        if (a.oUq || a.oVq) {
                            float uqv = xa, vqv = yb;
                            if (q == qprev && k > 0) {  // inside a tie run: searchsorted ranks of its first member
                                uqv = PX[lower_rank(U, n, q)];
                                vqv = PY[lower_rank(V, m, q)];
                            }
                            if (a.oUq) a.oUq[o] = uqv;
                            if (a.oVq) a.oVq[o] = vqv;
                        }
                    }
                }
                qprev = q;
                iu += tu ? 1u : 0u;
                const uint32_t vk = (uint32_t)(voff + D0 + s + 1);  // uniform across the wave up to D0
                const uint32_t off = 4u * (tu ? iu : (vk - iu));
                const float nv = *reinterpret_cast<const float*>(lb + off);
                const float np = *reinterpret_cast<const float*>(lb + off + poff4);
                ua = tu ? nv : ua;
                xa = tu ? np : xa;
                vb = tu ? vb : nv;
                yb = tu ? yb : np;
            }
        }
        if (QUANT && valid) {
            if (a.oU) for (int e = t; e < n; e += G) a.oU[row * (int64_t)n + e] = U[e];
            if (a.oV) for (int e = t; e < m; e += G) a.oV[row * (int64_t)m + e] = V[e];
        }
        SOT_STAMP(7);
        __builtin_amdgcn_s_setprio(0);
        acc = wave_sum(acc);
        if (CSR && bad_row) acc = __int_as_float(0x7fc00000);
        if (NW == 1) {
            if (t == 0 && valid && a.row_loss) store_row_loss(a.row_loss, row, acc, a.mt.counters != nullptr);
            row_sync<G / kWave>();  // this row's LDS reads are done before the next row's staging
        } else {
            if (c.lane == 0) c.red[c.wv] = acc;
            row_sync<G / kWave>();
            if (t == 0 && valid && a.row_loss) {
                float tot = c.red[0];
                for (int w = 1; w < NW; ++w) tot += c.red[w];
                store_row_loss(a.row_loss, row, tot, a.mt.counters != nullptr);  // NaN propagates from any wave of a bad CSR row
            }
        }
        SOT_STAMP(8);
#ifdef SOT_STAMPS
        if (wg_stamp && wg_row < 12) wgs[2 + wg_row++] = __builtin_readcyclecounter();
#endif
    }
    if (a.mt.counters != nullptr) batch_mean_tail<BLOCK>(a.mt, a.row_loss, a.B, reinterpret_cast<double*>(smem));
}

// ---- tail of the weight gradients, shared by sot_backward_kernel and sot_quantiles_backward_kernel ---------------------------
// Entry (a barrier has been passed since they were written): GU / GV hold dL/dU_i, dL/dV_j per CDF entry in sorted order.
// Reverse cumsums (fp64), normalisation terms, square_dist factor, scatter to the original columns through the sort permutation.
// UP: upU / upV (this row's [n] / [m], sorted order, or null) are added to the slots on the way.
template <int G, int CPT, bool ROWPOS, bool VEC, bool UP = false>
__device__ __forceinline__ void weight_grad_tail(const FwdArgs& a, const RowCtx<G>& c, const int (&ix)[CPT], const int (&iy)[CPT],
                                                 const float (&wx)[CPT], const float (&wy)[CPT], float Sx, float Sy,
                                                 const float* grad_row, int64_t grad_row_stride, float grad_scale, float* gx, float* gy,
                                                 int64_t row, int64_t rowc, bool valid, const float* upU = nullptr, const float* upV = nullptr)
{
    constexpr int NW = G / kWave;
    const int n = c.n, m = c.m, t = c.t;
    const int e0 = t * CPT;
    double ga[CPT], gb[CPT];
    double runx = 0.0, runy = 0.0;
#pragma unroll
    for (int k = CPT - 1; k >= 0; --k) {
        const bool okx = (e0 + k < n), oky = (e0 + k < m);
        runx += okx ? (double)c.GU[e0 + k] : 0.0;
        runy += oky ? (double)c.GV[e0 + k] : 0.0;
        if constexpr (UP) {   // upstream gradients of the CDF entries themselves (sorted order, like the slots)
            if (upU != nullptr && okx) runx += (double)upU[e0 + k];
            if (upV != nullptr && oky) runy += (double)upV[e0 + k];
        }
        ga[k] = runx;
        gb[k] = runy;
    }
    // exclusive suffix over lanes = wave total - inclusive prefix (fp64: the cancellation is harmless)
    const double pinx = wave_incl_scan(runx), piny = wave_incl_scan(runy);
    const double totwx = wave_last(pinx), totwy = wave_last(piny);
    double exx = totwx - pinx, exy = totwy - piny;
    if (NW > 1) {
        if (c.lane == 0) { c.wtot[c.wv] = totwx; c.wtot[NW + c.wv] = totwy; }
        row_sync<G / kWave>();
        double ox = 0.0, oy = 0.0;
        for (int w = NW - 1; w > c.wv; --w) { ox += c.wtot[w]; oy += c.wtot[NW + w]; }
        exx += ox;
        exy += oy;
    }
    // dot products  sum ga_i * w_i  (w = staged weight, squared if square_dist)
    double dotx = 0.0, doty = 0.0;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        ga[k] += exx;
        gb[k] += exy;
        const bool okx = (e0 + k < n), oky = (e0 + k < m);
        const float sx = c.sq ? wx[k] * wx[k] : wx[k];
        const float sy = c.sq ? wy[k] * wy[k] : wy[k];
        dotx += okx ? ga[k] * (double)sx : 0.0;
        doty += oky ? gb[k] * (double)sy : 0.0;
    }
    dotx = wave_sum(dotx);
    doty = wave_sum(doty);
    double totx = dotx, toty = doty;
    if (NW > 1) {
        row_sync<G / kWave>();  // wtot is reused
        if (c.lane == 0) { c.wtot[c.wv] = dotx; c.wtot[NW + c.wv] = doty; }
        row_sync<G / kWave>();
        totx = 0.0; toty = 0.0;
        for (int w = 0; w < NW; ++w) { totx += c.wtot[w]; toty += c.wtot[NW + w]; }
    }
    const double dx = (double)guard_mass(Sx), dy = (double)guard_mass(Sy);
    const double rdx = 1.0 / dx, rdy = 1.0 / dy;
    double gSx = -totx, gSy = -toty;
    if (c.dn) { gSx += gSy; gSy = 0.0; }
    gSx = (!c.prenorm && Sx > kMassEps) ? gSx * rdx * rdx : 0.0;
    gSy = (!c.prenorm && Sy > kMassEps) ? gSy * rdy * rdy : 0.0;
    const double gr = (grad_row ? (double)grad_row[rowc * grad_row_stride] : 1.0) * (double)grad_scale;
    if (valid) {
        const bool x_perm = ROWPOS ? c.do_sort : !c.x_ident;
        const bool y_perm = ROWPOS ? c.do_sort : !c.y_ident;
        float ox[CPT], oy[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            double g = ga[k] * rdx + gSx;
            if (c.sq) g *= 2.0 * (double)wx[k];
            ox[k] = (float)(g * gr);
            double h = gb[k] * rdy + gSy;
            if (c.sq) h *= 2.0 * (double)wy[k];
            oy[k] = (float)(h * gr);
        }
        if (gx) {
            float* dst = gx + row * (int64_t)n;
            if (VEC && !x_perm && (e0 + CPT <= n)) {
#pragma unroll
                for (int k = 0; k < CPT; k += 4)
                    *reinterpret_cast<float4*>(dst + e0 + k) = make_float4(ox[k], ox[k + 1], ox[k + 2], ox[k + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    const int e = e0 + k;
                    if (e < n) dst[ROWPOS ? (x_perm ? ix[k] : e) : (x_perm ? a.xperm[e] : e)] = ox[k];
                }
            }
        }
        if (gy) {
            float* dst = gy + row * (int64_t)m;
            if (VEC && !y_perm && (e0 + CPT <= m)) {
#pragma unroll
                for (int k = 0; k < CPT; k += 4)
                    *reinterpret_cast<float4*>(dst + e0 + k) = make_float4(oy[k], oy[k + 1], oy[k + 2], oy[k + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    const int e = e0 + k;
                    if (e < m) dst[ROWPOS ? (y_perm ? iy[k] : e) : (y_perm ? a.yperm[e] : e)] = oy[k];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Backward kernel: closed form of the autograd graph of losses.py:172-313.
// Recomputes the CDFs in LDS, then
//   g_k  = m_k d_k - m_{k+1} d_{k+1}   per merged level; searchsorted ranks are constant along a run
//          of equal levels, so g is non-zero only at a run's LAST member (stable order: U before V,
//          lower index first), which receives  d(run) - d(next run);
//   ga_i = sum_{i' >= i} gU_i'  (reverse cumsum, fp64);   gS = -sum ga_i w_i / S^2  (if S > 1e-7);
//   dL/dx_i = (ga_i / S + gS) * (2 x_i if square_dist) * grad_row.
// ---------------------------------------------------------------------------------------------
struct BwdArgs {
    FwdArgs f;
    const float* grad_row;     // dL/d(row_loss): [B] (stride 1) or one broadcast scalar (stride 0); null = 1 for every row
    int64_t grad_row_stride;
    float grad_scale;          // multiplies every upstream gradient (1/B of the batch mean)
    float* gx; float* gy;
    const float* rescale;      // the 16-bit y-only full-row kernel alone (sot_full_bwd.hpp: fix-up mode): device scalar or null
};

template <int G, int CPT, bool ROWPOS, int PM, bool LIM, bool VEC>
__global__ __launch_bounds__((G < 256 ? 256 : G)) void sot_backward_kernel(const BwdArgs b)   // (per-row positions capped at three waves per SIMD like the per-row forward: 76 dwords spilled, 290 -> 449 us)
{
    constexpr int BLOCK = (G < 256 ? 256 : G);
    constexpr int RPW = BLOCK / G;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FwdArgs& a = b.f;
    const RowCtx<G> c = make_ctx<G, ROWPOS>(a, smem, true);
    const int rg = threadIdx.x / G;
    const int n = c.n, m = c.m, t = c.t;
    float* const U = c.U; float* const V = c.V; float* const PX = c.PX; float* const PY = c.PY;

    const int64_t row_step = (int64_t)gridDim.x * RPW;
    int64_t row0 = (int64_t)blockIdx.x * RPW;
    float rx[CPT], ry[CPT];
    if (row0 < a.B) {
        const int64_t r = min(row0 + rg, a.B - 1);
        load_row<G, CPT, VEC>(a.x + r * a.xs, n, t, rx);
        load_row<G, CPT, VEC>(a.y + r * a.ys, m, t, ry);
    }
    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rg;
        const bool valid = row < a.B;
        const int64_t rowc = valid ? row : a.B - 1;
        int ix[CPT], iy[CPT];
        if (ROWPOS) {
            const int64_t pw = (int64_t)a.n + a.m;
            rowpos_prepare<G, CPT>(c, a.xpos + rowc * a.xps, a.ypos + rowc * a.yps, a.n, a.m, ix, iy,
                                                   a.perm_in ? a.perm_in + rowc * pw : nullptr, (a.perm_out && valid) ? a.perm_out + rowc * pw : nullptr);
        }
        store_row<G, CPT, VEC>(U, n, t, rx);
        store_row<G, CPT, VEC>(V, m, t, ry);
        if (row0 + row_step < a.B) {
            const int64_t r = min(row0 + row_step + rg, a.B - 1);
            load_row<G, CPT, VEC>(a.x + r * a.xs, n, t, rx);
            load_row<G, CPT, VEC>(a.y + r * a.ys, m, t, ry);
        }
        row_sync<G / kWave>();
        float wx[CPT], wy[CPT];
        float Sx, Sy;
        build_cdfs<G, CPT, ROWPOS>(a, c, ix, iy, wx, wy, Sx, Sy);

        // ---- merge walk over (pad zero levels ++ U, V), exactly E steps per thread.  The gradient of a level
        //      is known one step later (it is non-zero only if the NEXT level starts a new run), so the store
        //      of element k-1 happens at step k; the thread's last element is closed by peeking at level D0+E.
        __builtin_amdgcn_s_setprio(kWalkPrio);
        if (t < c.Ga) {
            const float* const Uw = U - c.pad;
            const float* const PXw = PX - c.pad;
            const int nw = n + c.pad;
            const int D0 = t * c.E;
            const uint32_t ub1 = lds_addr(Uw) - 4u;
            const int i0 = (int)((merge_path_steps32(ub1, lds_addr(V) + 4u * (uint32_t)D0 + ub1, nw, m, D0, c.topk) - ub1) >> 2);
            const int j0 = D0 - i0;
            float qprev = 0.0f;
            if (i0 > 0) qprev = Uw[i0 - 1];
            if (j0 > 0) qprev = fmaxf(qprev, V[j0 - 1]);
            float ua = Uw[i0], vb = V[j0], xa = PXw[i0], yb = PY[j0];
            float dcur = 0.0f;
            if (D0 == 0) {
                qprev = __int_as_float(0x7fc00000);  // NaN: the very first level always starts a run
            } else if (fminf(ua, vb) == qprev) {      // we start inside a run: cost at its first member's ranks
                const float q0 = qprev;
                const float cst = transport_cost<PM>(PX[lower_rank(U, n, q0)], PY[lower_rank(V, m, q0)], c.p);
                dcur = (LIM && q0 > 1.0f) ? 0.0f : cst;
            }
            char* const lb = reinterpret_cast<char*>(const_cast<float*>(Uw));
            const uint32_t poff4 = 4u * (uint32_t)c.L.poff;
            const uint32_t goff4 = 4u * (uint32_t)c.L.grad;
            const int voff = (int)(V - Uw);
            uint32_t iu = (uint32_t)i0;
            uint32_t prev_off = 4u * (uint32_t)(c.pad + n);  // U[n]'s gradient slot: a scratch target for "no element yet"
            for (int s = 0; s < c.E; ++s) {
                const bool tu = ua <= vb;
                const float q = tu ? ua : vb;
                float cst = transport_cost<PM>(xa, yb, c.p);
                if (LIM && q > 1.0f) cst = 0.0f;
                const bool new_run = !(q == qprev);
                *reinterpret_cast<float*>(lb + prev_off + goff4) = new_run ? (dcur - cst) : 0.0f;
                dcur = new_run ? cst : dcur;
                qprev = q;
                const uint32_t vk = (uint32_t)(voff + D0 + s);
                prev_off = 4u * (tu ? iu : (vk - iu));  // slot of the element consumed now
                iu += tu ? 1u : 0u;
                const uint32_t off = prev_off + 4u;  // the consumed side's next element
                const float nv = *reinterpret_cast<const float*>(lb + off);
                const float np = *reinterpret_cast<const float*>(lb + off + poff4);
                ua = tu ? nv : ua;
                xa = tu ? np : xa;
                vb = tu ? vb : nv;
                yb = tu ? yb : np;
            }
            {   // close the last element with the level that follows this thread's range (0 cost past the end)
                const float qn = fminf(ua, vb);
                float cn = transport_cost<PM>(xa, yb, c.p);
                if ((LIM && qn > 1.0f) || (t == c.Ga - 1)) cn = 0.0f;
                const bool new_run = !(qn == qprev) || (t == c.Ga - 1);
                *reinterpret_cast<float*>(lb + prev_off + goff4) = new_run ? (dcur - cn) : 0.0f;
            }
        }
        __builtin_amdgcn_s_setprio(0);
        row_sync<G / kWave>();

        weight_grad_tail<G, CPT, ROWPOS, VEC>(a, c, ix, iy, wx, wy, Sx, Sy, b.grad_row, b.grad_row_stride, b.grad_scale, b.gx, b.gy, row, rowc, valid);
        row_sync<G / kWave>();  // GU/GV/wtot reads done before the next row reuses LDS
    }
}

}  // namespace sot
