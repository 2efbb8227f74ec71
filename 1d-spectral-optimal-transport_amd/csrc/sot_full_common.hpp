// sot_full_common.hpp -- what the forward and the backward full-row kernels (compile-time geometries) share, namespace sot: the row
// masses and row fetches with compile-time lengths, the partition search, the LDS layout and the facts of one geometry (FullLayout,
// FullGeo, FullCtx), the workgroup setup, the CDF builder and the row setup of per-row positions.  Included through sot_full_fwd.hpp
// (forward, area and half-wave kernels) and sot_full_bwd.hpp (backward kernel, merge-free training form), which hold the kernels and
// their launch and dispatch templates.
#pragma once
#include "sot_launch.hpp"

namespace sot {

// Diagnostic build only (-DSOT_STAMPS): thread 0 of one workgroup adds up, per phase of its rows, the shader clocks between
// consecutive checkpoints (sacc[i] += now - sacc[15]; sacc[15] = now) and stores the sums at the end; no output depends on them.
#ifdef SOT_STAMPS
#define SOT_PH(sacc, i) do { if ((sacc) != nullptr) { __builtin_amdgcn_sched_barrier(0); const unsigned long long now_ = __builtin_readcyclecounter(); \
                              (sacc)[i] += now_ - (sacc)[15]; (sacc)[15] = now_; __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define SOT_PH(sacc, i) do { } while (0)
#endif

// mass_column() / mass_fold() of sot_device.hpp with a compile-time row length (no left-over vectors, see FullGeo)
template <int NSTEPS>
__device__ __forceinline__ float mass_column_nx(const float* part, int c)
{
    constexpr int NFULL = NSTEPS >> 4;
    constexpr int NREAD = NFULL + ((NSTEPS & 15) ? 1 : 0);
    float pre[NREAD];
#pragma unroll
    for (int h = 0; h < NREAD; ++h) pre[h] = part[(h << 5) + c];  // independent reads: one LDS round trip
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
    for (int h = 0; h < NFULL; ++h) {
        a0 = pre[h];
        a1 += a0; a0 = 0.0f;
        if ((((h + 1) << 4) & (15 << 4)) == 0) {
            a2 += a1; a1 = 0.0f;
            if ((((h + 1) << 4) & (15 << 8)) == 0) { a3 += a2; a2 = 0.0f; }
        }
    }
    if (NSTEPS & 15) a0 = pre[NFULL];
    return ((a0 + a1) + a2) + a3;
}

// staged (swizzled, see full_build_cdfs) index of raw element e
__host__ __device__ constexpr int staged_index(int e, bool swz) { return swz ? (e ^ (((e >> 5) & 1) << 2)) : e; }

template <bool SQ, int N, bool SWZ>
__device__ __forceinline__ float mass_fold_nx(const float* raw, const float* colbuf)
{
    const float4* c4 = reinterpret_cast<const float4*>(colbuf);
    const float4 a0 = c4[0], a1 = c4[1], b0 = c4[2], b1 = c4[3], c0 = c4[4], c1 = c4[5], d0 = c4[6], d1 = c4[7];
    const float p0 = ((a0.x + b0.x) + c0.x) + d0.x, p1 = ((a0.y + b0.y) + c0.y) + d0.y;
    const float p2 = ((a0.z + b0.z) + c0.z) + d0.z, p3 = ((a0.w + b0.w) + c0.w) + d0.w;
    const float p4 = ((a1.x + b1.x) + c1.x) + d1.x, p5 = ((a1.y + b1.y) + c1.y) + d1.y;
    const float p6 = ((a1.z + b1.z) + c1.z) + d1.z, p7 = ((a1.w + b1.w) + c1.w) + d1.w;
    float fin = 0.0f;
#pragma unroll
    for (int k = (N >> 3) << 3; k < N; ++k) { const float w = raw[staged_index(k, SWZ)]; fin += SQ ? w * w : w; }  // scalar tail first
    fin += p0; fin += p1; fin += p2; fin += p3; fin += p4; fin += p5; fin += p6; fin += p7;
    return fin;
}

// Unroll factor of the merge walks in this file (trip count E is a compile-time constant, 3 ... 17).  Round 3: 32 = complete unrolling
// (the loop-carried register moves of the partially unrolled form disappear): paper-mode forward 8192 x 2048 45.9 -> 44.1 us, training
// form 79.7 -> 78.7 us (profiles/r3_walk_experiments_ab.txt); round 1-2 default was 2 (SOT_WALK_UNROLL of the generic kernels).
#define SOT_FULL_WALK_UNROLL 32
// (Round 3: two / three / four shorter merge segments per thread in the forward kernel, their search and walk chains interleaved, were
// slower -- paper-mode forward 45.8 -> 49.1 / 54.3 / 57.8 us: these phases are bound by instructions issued, not by the latency of their chains.)

// merge_path_steps32() of sot_device.hpp with compile-time lengths: the rounds unroll completely and the probe offsets
// fold into the LDS instructions (5 VALU per round).  ub1 = LDS address of U[-1], vd1 = LDS address of V[D] + ub1; returns
// the address of U[i0 - 1] (i0 = number of U elements among the first D merged elements).
// (Measured on 8192x2048: divergent bisection 48.7 us, this search with steps 2^k 47.9 us, with steps 2^k + 1 45.6 us; a
// 4-ary search with three probes per round 49.0 us -- the search is bound by LDS bank conflicts and LDS reads, not by
// its number of dependent rounds.)
template <int NU, int NV>
__device__ __forceinline__ uint32_t merge_path_fixed32(uint32_t ub1, uint32_t vd1, int D)
{
    constexpr int TOPK = merge_steps_top(NU < NV ? NU : NV);
    const int lo = max(0, D - NV), hi = min(D, NU);
    uint32_t posb = ub1 + 4u * (uint32_t)lo;         // address of U[pos - 1]
    const uint32_t hib = ub1 + 4u * (uint32_t)hi;
#pragma unroll
    for (int k = TOPK; k >= -1; --k) {
        const uint32_t step4 = 4u * (uint32_t)(k >= 1 ? (1 << k) + 1 : (k == 0 ? 2 : 1));  // ..., 9, 5, 3, 2, 1
        const uint32_t candb = posb + step4;          // address of U[cand - 1]
        const float u = lds_load(candb);
        const float v = lds_load(vd1 - candb);        // V[D - cand]
        const int take = (int)(candb <= hib) & (int)(u <= v);  // bitwise: no branch around the LDS reads
        posb = take ? candb : posb;
    }
    return posb;
}

// rows of N floats at any alignment: element t + k*G in rx[k] (coalesced dword loads)
template <int G, int CPT, int N>
__device__ __forceinline__ void fetch_row_dwords(const float* __restrict__ x, const float* __restrict__ y, int t, float (&rx)[CPT],
                                                 float (&ry)[CPT])
{
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        if (k * G < N) {
            const int e = t + k * G;
            const bool ok = ((k + 1) * G <= N) || (e < N);
            rx[k] = ok ? x[e] : 0.0f;
            ry[k] = ok ? y[e] : 0.0f;
        }
    }
}

// One row of n floats as a raw buffer (gfx9 resource word 3 = 32-bit raw data; the row pointer is wave-uniform): a load past the
// row returns 0, a store past it is dropped, per dword -- also inside a merged multi-dword access (the ISA range-checks
// load/store_dwordx{2,3,4} per component) -- so rows whose length is not the geometry's need neither predicates nor branches around
// their memory instructions, and an address is one 32-bit byte offset instead of a 64-bit pointer per element.
// Against predicated global loads / stores (training form, run-time lengths): 8192 x 2000 109.0 -> 106.5 us.  For the compile-time odd
// lengths the same stores change nothing or lose (513 bins: 24.7 -> 26.2 us), so those keep their predicated stores.
typedef __amdgpu_buffer_rsrc_t RowBuffer;
__device__ __forceinline__ RowBuffer row_buffer(const float* row, int n)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), (short)0, n * 4, 0x00020000);
}
__device__ __forceinline__ float row_buffer_load(RowBuffer rb, int element)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, element * 4, 0, 0));
}
__device__ __forceinline__ void row_buffer_store(RowBuffer rb, int element, float v)
{
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v), rb, element * 4, 0, 0);
}

// the same for a row length known only at run time (n <= G * CPT): elements past the row read as zero weights
template <int G, int CPT>
__device__ __forceinline__ void fetch_row_dwords_rt(const float* __restrict__ x, const float* __restrict__ y, int t, int n, float (&rx)[CPT],
                                                    float (&ry)[CPT])
{
    const RowBuffer bx = row_buffer(x, n), by = row_buffer(y, n);
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        rx[k] = row_buffer_load(bx, t + k * G);
        ry[k] = row_buffer_load(by, t + k * G);
    }
}

// one row's loads in the form its geometry takes (NX == 0: 16-B loads, NX > 0: dword loads with a compile-time length, NX < 0: run time)
// WT: the element type of the weight rows in memory -- float, or uint16_t for bfloat16 rows (NX == 0 only; a.x / a.y then point at 16-bit
// elements and the row strides count them).  A fetched bfloat16 is widened in the register, float(bits << 16): exact, so everything behind
// the fetch is the float32 code and returns the bits of the float32 call on the upcast rows.
template <int G, int CPT, int NX, class WT = float>
__device__ __forceinline__ void fetch_row(const float* __restrict__ x, const float* __restrict__ y, int t, int n, float (&rx)[CPT], float (&ry)[CPT]);

// row r of a weight array whose elements are WT and whose row stride counts them (the pointer travels as const float* whatever WT is)
template <class WT>
__device__ __forceinline__ const float* weight_row(const float* base, int64_t r, int64_t stride)
{
    if constexpr (std::is_same<WT, float>::value) return base + r * stride;
    else return reinterpret_cast<const float*>(reinterpret_cast<const WT*>(base) + r * stride);
}

// float32 -> bfloat16, round to nearest even: the one narrowing of the library (the row-conversion kernel of sot_bf16.hip and the 16-bit
// gradient stores of sot_full_bwd.hpp), the bits of torch's .to(torch.bfloat16).
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f)
{
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)0x7FC0;      // NaN stays NaN (the payload is not kept)
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);       // ties to even; past the largest finite value: the carry makes +-inf
}

template <int G, int CPT>
__device__ __forceinline__ void fetch_full_row(const float* __restrict__ x, const float* __restrict__ y, int t, float (&rx)[CPT],
                                               float (&ry)[CPT])
{
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* y4 = reinterpret_cast<const float4*>(y);
#pragma unroll
    for (int k = 0; k < CPT / 4; ++k) {
        const float4 vx = x4[t + k * G], vy = y4[t + k * G];
        rx[4 * k] = vx.x; rx[4 * k + 1] = vx.y; rx[4 * k + 2] = vx.z; rx[4 * k + 3] = vx.w;
        ry[4 * k] = vy.x; ry[4 * k + 1] = vy.y; ry[4 * k + 2] = vy.z; ry[4 * k + 3] = vy.w;
    }
}

// Rows that fill their geometry (NX == 0: n == m == 8 G), round 4: COLUMN fetch.  ATen's row sum (sot_device.hpp) is 32 interleaved
// columns x chunks of 16 steps; such a row has exactly G (column, chunk) tasks over both arrays, one per thread.  Thread t therefore
// fetches the 16 elements of ITS task -- array (x for t < G/2, y above), column c = t & 31, chunk h = (t mod G/2) >> 5: elements
// 32 (16 h + s) + c, s = 0 ... 15, i.e. per load instruction two whole 128-byte lines per wave -- adds them up in ATen's order straight
// from the registers and stages them for the owner reads (full_build_cdfs P1).  Against the float4 fetch (thread t: float4 t and t + G of
// both arrays): the chunk sums no longer read the staged row back from LDS (16 ds_read_b32 per thread) and the workgroup barrier between
// staging and chunk sums is gone; 16 dword loads and 16 ds_write_b32 per thread instead of 4 + 4 sixteen-byte ones.
// rx[k] = step k, ry[k] = step 8 + k of the thread's task (both of ONE array).
// forward kernels in square_dist mode stage the SQUARED weights (the chunk sums need the squares anyway; the owner's division then reads
// them instead of squaring again); the backward kernels keep the raw weights (their output arithmetic needs them)
// WT = uint16_t (bfloat16 rows): the same tasks, the same registers and therefore the same summation order, read with 16-bit loads -- per
// load instruction a wave then touches two half-used 128-byte lines, which the 16 steps of the task use up between them.
template <int G, int CPT, class WT = float>
__device__ __forceinline__ void fetch_row_columns(const float* __restrict__ x, const float* __restrict__ y, int t, float (&rx)[CPT], float (&ry)[CPT])
{
    static_assert(CPT == 8, "16 steps per task: two registers arrays of 8");
    const bool isy = t >= G / 2;
    const int task = isy ? t - G / 2 : t;
    if constexpr (std::is_same<WT, float>::value) {
        const float* const src = (isy ? y : x) + ((task >> 5) << 9) + (task & 31);
#pragma unroll
        for (int k = 0; k < 8; ++k) { rx[k] = src[k << 5]; ry[k] = src[(8 + k) << 5]; }
    } else {
        static_assert(std::is_same<WT, uint16_t>::value, "weight rows are float32 or bfloat16");
        const uint16_t* const src = reinterpret_cast<const uint16_t*>(isy ? y : x) + ((task >> 5) << 9) + (task & 31);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            rx[k] = __uint_as_float((uint32_t)src[k << 5] << 16);
            ry[k] = __uint_as_float((uint32_t)src[(8 + k) << 5] << 16);
        }
    }
}

// The same for the one-sided spectra (NX = 129 / 257 / 513 / 1025 / 2049 bins on their odd geometries): the 2 NT = 64 ceil(NSTEPS / 16) tasks
// of both arrays are one per thread (two for the one-wave rows of 1025 bins), a task has CHUNK = min(16, NSTEPS) steps, and the row's last
// element (N mod 8 == 1: ATen's scalar tail) is fetched by thread 0 (x) / thread 1 (y).  Register j of the thread's TPT * CHUNK (+ 1) values
// is rx[j] for j < CPT and ry[j - CPT] above.
template <int G, int CPT, int N>
struct ColumnsNX {
    static constexpr int NSTEPS = N >> 5, NCH = (NSTEPS + 15) >> 4, NT = 32 * NCH, CHUNK = NSTEPS < 16 ? NSTEPS : 16;
    static constexpr int TPT = (2 * NT) / G;                 // tasks per thread
    static constexpr int NV = TPT * CHUNK;                   // column values per thread; slot NV holds the tail element (threads 0 and 1)
    // Measured (round 4, interleaved A/B, profiles/r4d_column_fetch_nx_ab.txt): 16384 x 1025 paper-mode forward 39.4 -> 38.8 us, merge-free p = 1
    // 29.0 -> 28.2 us, 4096 x 2049 forward 26.0 -> 25.1 us; the training kernels do not move (79.7 vs 79.8 us); the short one-wave rows LOSE
    // (16384 x 257 forward 15.2 -> 16.8 us, 8192 x 513 training 24.8 -> 25.6 us: 8 / 16 dword loads per thread instead of 5 / 9 for the same bytes):
    // 1025 bins and up only.
    static constexpr int MIN_BINS = 1025;
    static constexpr bool OK = (2 * NT) % G == 0 && TPT >= 1 && NV + 1 <= 2 * CPT && (N & 7) == 1 && N >= MIN_BINS;
};
template <int CPT>
__device__ __forceinline__ float& column_slot(float (&rx)[CPT], float (&ry)[CPT], int j) { return j < CPT ? rx[j] : ry[j - CPT]; }

template <int G, int CPT, int N>
__device__ __forceinline__ void fetch_row_columns_nx(const float* __restrict__ x, const float* __restrict__ y, int t, float (&rx)[CPT], float (&ry)[CPT])
{
    using C = ColumnsNX<G, CPT, N>;
#pragma unroll
    for (int i = 0; i < C::TPT; ++i) {
        const int id = t + i * G;
        const bool isy = id >= C::NT;
        const int task = isy ? id - C::NT : id;
        const float* const src = (isy ? y : x) + ((task >> 5) << 9) + (task & 31);
#pragma unroll
        for (int k = 0; k < C::CHUNK; ++k) column_slot<CPT>(rx, ry, i * C::CHUNK + k) = src[k << 5];
    }
    float tail = 0.0f;
    if (t < 2) tail = (t ? y : x)[N - 1];
    column_slot<CPT>(rx, ry, C::NV) = tail;
}

template <int G, int CPT, int NX, class WT>
__device__ __forceinline__ void fetch_row(const float* __restrict__ x, const float* __restrict__ y, int t, int n, float (&rx)[CPT], float (&ry)[CPT])
{
    static_assert(std::is_same<WT, float>::value || NX == 0, "16-bit rows: the geometries that a row fills (16-byte aligned rows) only");
    if constexpr (NX == 0) fetch_row_columns<G, CPT, WT>(x, y, t, rx, ry);
    else if constexpr (NX > 0 && ColumnsNX<G, CPT, (NX > 0 ? NX : 129)>::OK) fetch_row_columns_nx<G, CPT, NX>(x, y, t, rx, ry);
    else if constexpr (NX == 0) fetch_full_row<G, CPT>(x, y, t, rx, ry);
    else if constexpr (NX > 0) fetch_row_dwords<G, CPT, NX>(x, y, t, rx, ry);
    else fetch_row_dwords_rt<G, CPT>(x, y, t, n, rx, ry);
}

struct FullLayout {
    int padcap;        // spare floats in front of U (front padding of the merge walk + the virtual predecessor)
    int nU, nV;        // floats of the U and V regions (incl. sentinel and spare slots)
    int part;          // 2 * NT chunk sums (x then y)
    int colbuf;        // 2 x 32 column totals
    int wtot;          // 2 * NW doubles
    int red;           // NW floats + S_x, S_y, 1/S_x^, 1/S_y^
    int grad;          // backward only: first float of the gradient region
    int goff;          // backward only: gradient slot of the level at float offset o = o + goff (GRAD 1: a region mirroring
                       // [pad | U | V]; GRAD 2, gradient w.r.t. y only: a region mirroring V alone -- U levels have no slot)
    int rowf;          // floats per row region
    int posf;          // floats of the shared position region [padcap | PX | PY]
    int total;         // floats per workgroup
};

// NX: row length when it is smaller than the geometry's capacity G*CPT (the paper's 257 / 513 / 1025 bins); 0 = G*CPT;
// NX < 0 (round 3): the row length n <= G*CPT is a RUN-TIME argument.  Such a row is processed as a row of G*CPT points whose points
// past n carry zero weight and sit at the row's LAST position: zero-weight points are inert as long as they do not move
// the clamp target of losses.py:220, which a duplicate of the last position does not; in the backward their level ties with U_{n-1}
// may take over a run's gradient, which the suffix sums hand back to every real point (their own gradients are never stored).
// Only the row mass has to follow the real length (ATen's summation plan depends on n): it runs the generic mass_* functions.
// The U / V regions always span the capacity: threads past the row read zeros there (set once), the sentinel sits at N.
// GRAD: 0 forward, 1 backward w.r.t. x and y, 2 backward w.r.t. y only (the training step)
template <int G, int CPT, int ROWS, int GRAD = 0, int NX = 0>
__host__ __device__ constexpr FullLayout full_layout()
{
    constexpr int CAP = G * CPT, N = NX > 0 ? NX : CAP, NW = G / kWave, NT = 32 * (((N >> 5) + 15) >> 4);
    FullLayout L{};
    L.padcap = align4(merge_steps(2 * N, G)) + 4;  // + the virtual predecessor slot
    L.nU = L.padcap + CAP + 4;
    L.nV = CAP + 4;
    L.part = L.nU + L.nV;
    L.colbuf = L.part + 2 * NT;
    L.wtot = L.colbuf + 64;
    L.red = L.wtot + 4 * NW;
    L.grad = align4(L.red + NW + 4);
    L.goff = GRAD == 2 ? L.grad - L.nU : L.grad;
    L.rowf = GRAD == 2 ? L.grad + L.nV : GRAD ? L.grad + L.nU + L.nV : L.grad;
    L.posf = L.nU + L.nV;
    L.total = ROWS * L.rowf + L.posf;
    return L;
}

// compile-time facts of one geometry
template <int G, int CPT, int ROWS, int GRAD, int NX = 0>
struct FullGeo {
    static_assert(ROWS >= 1 && ROWS <= 4, "row groups per workgroup");
    static constexpr int CAP = G * CPT;              // elements the row group's threads own (CPT contiguous ones each)
    static constexpr bool RT = NX < 0;               // the row length is a run-time argument (<= CAP); N below is then the capacity
    static constexpr int N = NX > 0 ? NX : CAP;      // row length (n == m)
    static constexpr bool ALIGNED = (NX == 0);       // rows are whole float4s on 16-B boundaries (checked by the host)
    static constexpr int NSTEPS = N >> 5;            // ATen: steps of each of the 32 columns
    static_assert(N <= CAP && N >= 64 && CPT >= 2 && CPT <= 17, "the row fits its geometry");
    static_assert(!ALIGNED || CPT == 8, "rows that fill their geometry: 8 contiguous elements (two 16-B halves) per thread");
    static constexpr bool SWZ = CPT == 8 && !RT;   // staging swizzle (see full_build_cdfs): 8-element owners only
    static_assert(NX <= 0 || CAP - N >= 1, "NX is for rows shorter than the capacity");
    static_assert(RT || NSTEPS < 16 || NSTEPS % 16 == 0, "every column is either one partial chunk or whole 16-step chunks");
    static_assert(RT || (N >> 3) == NSTEPS * 4, "no left-over 8-lane vectors (N mod 32 < 8)");
    static_assert(!SWZ || ((N >> 5) & 1) == 0 || (N & 7) == 0, "the scalar tail sits in an unswapped staging block");
    static_assert(((G >> 5) & 1) == 0, "the staging swizzle of element t + k*G must not depend on k");
    static constexpr int BLOCK = ROWS * G;
    static constexpr int NW = G / kWave;
    static constexpr int K = 2 * N;
    static constexpr int E = merge_steps(K, G);      // 17 at N = 2048; 18, 19 and 21 were measured 2-4 % slower, 16 13 % slower
    static constexpr int GA = (K + E - 1) / E;       // threads that take part in the walk
    static constexpr int PAD = GA * E - K;           // zero-valued levels in front of U
    static constexpr int NCH = (NSTEPS + 15) >> 4;   // chunks per ATen column
    static constexpr int CHUNK = NSTEPS < 16 ? NSTEPS : 16;  // steps per chunk
    static constexpr int NT = 32 * NCH;              // chunk-sum tasks per array
    static constexpr FullLayout L = full_layout<G, CPT, ROWS, GRAD, NX>();
    static_assert(PAD + 1 <= L.padcap, "room for the virtual predecessor in front of the padding");
};

// per-thread view of its row group
struct FullCtx {
    float* U; float* V; float* part; float* colbuf; double* wtot; float* red; float* Sv;
    const float* Uw;           // U with its zero-valued front padding
    const float* PX; const float* PY;  // the workgroup's shared positions
    int rg, t, lane, wv;       // row group (wave-uniform), thread within it, lane, wave within the row group (uniform)
    bool dn, x_ident, y_ident;
};

// Once per workgroup: the shared support positions (sorted) behind the row regions; per row group: front padding,
// sentinels and virtual predecessors.
template <int G, int CPT, int ROWS, int GRAD, int NX = 0, bool RP = false>
__device__ __forceinline__ FullCtx full_setup(const FwdArgs& a, float* smem)
{
    using Geo = FullGeo<G, CPT, ROWS, GRAD, NX>;
    constexpr FullLayout L = Geo::L;
    constexpr int N = Geo::N, PAD = Geo::PAD;
    FullCtx c;
    const int tid = threadIdx.x;
    c.rg = __builtin_amdgcn_readfirstlane(tid / G);
    c.t = tid - c.rg * G;
    c.lane = tid & (kWave - 1);
    c.wv = __builtin_amdgcn_readfirstlane(c.t >> 6);
    c.dn = a.flags & SOT_FLAG_DONT_NORMALIZE;
    float* const base = smem + c.rg * L.rowf;
    c.U = base + L.padcap;
    c.V = base + L.nU;
    c.part = base + L.part;
    c.colbuf = base + L.colbuf;
    c.wtot = reinterpret_cast<double*>(base + L.wtot);
    c.red = base + L.red;
    c.Sv = c.red + Geo::NW;
    c.Uw = c.U - PAD;
    c.x_ident = true; c.y_ident = true;
    if (a.ident != nullptr) { c.x_ident = a.ident[0] != 0; c.y_ident = a.ident[1] != 0; }
    float* const PX = smem + ROWS * L.rowf + L.padcap;
    float* const PY = smem + ROWS * L.rowf + L.nU;
    c.PX = PX; c.PY = PY;
    const int nlast = (Geo::RT ? a.n : N) - 1;    // index of the row's last real point
    if (!RP) {   // (RP: every row brings its own positions, see sot_forward_full_kernel)
#pragma unroll
        for (int e = tid; e < N; e += Geo::BLOCK) {   // run-time length: the points past the row sit at its last position
            const int es = Geo::RT ? min(e, nlast) : e;
            PX[e] = a.xpos[es]; PY[e] = a.ypos[es];
        }
        if (tid < PAD) PX[tid - PAD] = a.xpos[0];  // any finite value: the padded levels have zero width
        if (tid == 0) {
            PX[N] = a.xpos[nlast];  // clamp of losses.py:220: ranks beyond the last index reuse it
            PY[N] = a.ypos[nlast];
        }
    }
    if (c.t < PAD) c.U[c.t - PAD] = 0.0f;
    for (int e = N + 1 + c.t; e < Geo::CAP; e += G) { c.U[e] = 0.0f; c.V[e] = 0.0f; }  // owned slots past the row: weight 0, forever
    if (c.t == 0) {
        c.U[N] = INFINITY; c.V[N] = INFINITY;             // sentinels: an exhausted side never wins the merge
        c.U[-PAD - 1] = -INFINITY; c.V[-1] = -INFINITY;   // virtual predecessors: never win the fmaxf that rebuilds Q_{k-1}
        if (Geo::RT) { c.U[N + 1] = 0.0f; c.V[N + 1] = 0.0f; }   // the zero slot that permuted owner reads of points past the row hit
    }
    return c;
}

// full_build_cdfs adds up the totals of the waves in front of a wave either in a loop over them (one LDS round trip per wave) or, for rows
// of at most this many waves, from all totals read at once under wave-uniform selects.  The second form holds 4 (NW - 1) more registers
// while it runs: at 8 and 16 waves per row (512- and 1024-thread rows) it cost kernels their fourth wave per SIMD (126 -> 129, 125 -> 138
// VGPRs in the backward) or put them into scratch (8192-bin forward and merge-free kernels: 60-112 bytes); up to four waves no kernel lost a
// wave per SIMD or gained scratch.  Forward kernels (GRAD == 0) only: 1024- and 1500-bin forwards gained 0.5-0.7 us per 16384-32768 rows, but the
// backward kernels moved both ways (both gradients at 1500 bins 200.7 -> 199.4 us, y only at 1024 bins 70.0 -> 70.4 us, where the form
// gave the kernel a fourth wave per SIMD, 130 -> 116 VGPRs) and keep the loop.
constexpr int kPrefixSelectMaxWaves = 4;

struct NoRowHook { __device__ __forceinline__ void operator()() const {} };   // full_build_cdfs: nothing to do behind barrier 1

// P1-P3 of one row: raw weights -> LDS, row masses in ATen order, safe_divide, fp64-accumulated CDFs into U / V (ends
// with the barrier that publishes them).  rx / ry: this row's weights (coalesced float4 layout), refilled with the next
// row's (nxt_x / nxt_y, null at the end); wx / wy: the CPT contiguous raw weights this thread owns in sorted order.
// TO_LDS = false (the merge-free p = 1 kernel): the CDFs of the thread's own CPT elements are only returned in cu / cv,
// nothing is written to U / V and the closing barrier is left out (the barrier behind the raw reads already orders the next
// row's staging behind this row's last LDS read of the raw weights).
// RAW_OUT: wx / wy must be the weights as given (a gradient needs them); otherwise square_dist rows may be staged as their squares
// WT: the weight rows' element type in memory (fetch_row), which only the next-row prefetch at the end sees.
// PLAIN (the fast body of sot_area_full_kernel): the caller has checked, once per launch, that both permutations are the identity and
// that the rows are normalised; c.dn / c.x_ident / c.y_ident are then compile-time constants here and the permuted owner reads are not
// compiled.  after_b1(): called by every thread behind barrier 1 (that body's deferred row-loss store).  PLAIN and after_b1 belong to
// that one caller: the merge, backward and training kernels leave both at their defaults.
template <int G, int CPT, int ROWS, int GRAD, bool SQ, int NX = 0, bool TO_LDS = true, bool RAW_OUT = (GRAD != 0), bool PLAIN = false,
          class AfterB1 = NoRowHook, class WT = float>
__device__ __forceinline__ void full_build_cdfs(const FwdArgs& a, const FullCtx& c, float (&rx)[CPT], float (&ry)[CPT],
                                                const float* nxt_x, const float* nxt_y, float (&wx)[CPT], float (&wy)[CPT],
                                                float& Sx, float& Sy, float (&cu)[CPT], float (&cv)[CPT], unsigned long long* sacc = nullptr,
                                                const int* psx = nullptr, const int* psy = nullptr, AfterB1 after_b1 = AfterB1{})
{
    // psx / psy (forward kernels, round 4): the staged LDS indices of the thread's CPT owned elements on a PERMUTED shared grid, looked up
    // once per workgroup instead of once per row (the plan's permutation is row-invariant; the compiler cannot hoist the loads itself:
    // 8192 x 2048 paper mode on an unsorted grid 83.5 us with a lookup per row)
    (void)sacc;
    using Geo = FullGeo<G, CPT, ROWS, GRAD, NX>;
    constexpr int N = Geo::N, NW = Geo::NW, NT = Geo::NT, CHUNK = Geo::CHUNK;
    constexpr bool ALIGNED = Geo::ALIGNED, RT = Geo::RT;
    float* const U = c.U; float* const V = c.V; float* const part = c.part; float* const colbuf = c.colbuf;
    double* const wtot = c.wtot; float* const Sv = c.Sv;
    const int t = c.t, lane = c.lane, wv = c.wv;
    const bool dn = PLAIN ? false : c.dn, x_ident = PLAIN ? true : c.x_ident, y_ident = PLAIN ? true : c.y_ident;
    // The RAW weights are staged with the two 16-B halves of every second 32-B block swapped (float index e lives at
    // e ^ 4 when bit 5 of e is set): the owner reads below (16 B per lane at a 32-B lane stride) then touch all 32 banks
    // instead of every bank twice.  Every address involved is a per-thread constant; the CDFs are written unswizzled.
    // Owners of CPT != 8 elements (the one-sided spectra: 129 / 257 / 513 / 1025 / 2049 bins on 3 / 5 / 9 elements per thread) read
    // and write their elements one dword at a time at a lane stride of CPT dwords -- odd, hence conflict-free -- and need no swizzle.
    constexpr bool SWZ = Geo::SWZ;
    static_assert(G % 16 == 0, "whole 16-lane groups per row");
    const int q0s = SWZ ? (t ^ ((t >> 3) & 1)) : t;  // float4 slot of this thread's coalesced chunk t (+ k*G)
    const int ownf = SWZ ? ((t >> 2) & 1) : 0;       // this thread's 8 owned elements sit in a swapped block
    // ---- P1: registers -> LDS in original column order; fetch the next row into the registers
    constexpr bool COLUMNS_NX = (NX > 0) && ColumnsNX<G, CPT, (NX > 0 ? NX : 129)>::OK;   // fetch_row_columns_nx
    constexpr bool COLUMNS = ALIGNED || COLUMNS_NX;   // staging and chunk sum of the thread's own task(s)
    constexpr bool PRESQ = COLUMNS && SQ && !RAW_OUT;   // the staged values are the squares
    if constexpr (COLUMNS_NX) {
        using C = ColumnsNX<G, CPT, (NX > 0 ? NX : 129)>;
        static_assert(!COLUMNS_NX || (C::NT == NT && C::CHUNK == CHUNK && !SWZ), "the task layout of the chunk sums below");
#pragma unroll
        for (int i = 0; i < C::TPT; ++i) {
            const int id = t + i * G;
            const bool isy = id >= NT;
            const int task = isy ? id - NT : id;
            float* const dst = (isy ? V : U) + ((task >> 5) << 9) + (task & 31);
            float v[C::CHUNK];
#pragma unroll
            for (int k = 0; k < C::CHUNK; ++k) { const float w = column_slot<CPT>(rx, ry, i * C::CHUNK + k); v[k] = PRESQ ? w * w : w; }
#pragma unroll
            for (int k = 0; k < C::CHUNK; ++k) dst[k << 5] = v[k];
            if (!(isy && dn)) {
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < C::CHUNK; ++k) acc += (SQ && !PRESQ) ? v[k] * v[k] : v[k];
                part[id] = acc;
            }
        }
        if (t < 2) { const float w = column_slot<CPT>(rx, ry, C::NV); (t ? V : U)[N - 1] = PRESQ ? w * w : w; }   // ATen's scalar tail (mass_fold_nx reads it)
    } else if constexpr (COLUMNS) {
        static_assert(2 * NT == G, "one (column, chunk) task per thread");
        const bool isy = t >= NT;
        const int task = isy ? t - NT : t;
        float* const dst = (isy ? V : U) + ((task >> 5) << 9) + (task & 31);
        float* const dsto = (isy ? V : U) + ((task >> 5) << 9) + ((task & 31) ^ (SWZ ? 4 : 0));   // odd steps: bit 5 of the element index set
        float v[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = PRESQ ? rx[k] * rx[k] : rx[k]; v[8 + k] = PRESQ ? ry[k] * ry[k] : ry[k]; }
#pragma unroll
        for (int k = 0; k < 16; ++k) ((k & 1) ? dsto : dst)[k << 5] = v[k];
        if (!(isy && dn)) {   // ATen's chunk sum of this task, in its order (0 + v0 + v1 + ...)
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) acc += (SQ && !PRESQ) ? v[k] * v[k] : v[k];
            part[t] = acc;
        }
    } else if constexpr (ALIGNED) {
#pragma unroll
        for (int k = 0; k < CPT / 4; ++k) {
            reinterpret_cast<float4*>(U)[q0s + k * G] = make_float4(rx[4 * k], rx[4 * k + 1], rx[4 * k + 2], rx[4 * k + 3]);
            reinterpret_cast<float4*>(V)[q0s + k * G] = make_float4(ry[4 * k], ry[4 * k + 1], ry[4 * k + 2], ry[4 * k + 3]);
        }
    } else {  // element t + k*G; its staging slot differs from it by a per-thread constant (bit 5 of t decides the swap)
        const int es = SWZ ? (t ^ (((t >> 5) & 1) << 2)) : t;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            if (RT || (k * G < N && (((k + 1) * G <= N) || (t + k * G < N)))) { U[es + k * G] = rx[k]; V[es + k * G] = ry[k]; }
        }
    }
    SOT_PH(sacc, 1);   // staging stores issued (includes the wait for this row's loads)
    row_sync<NW>();
    SOT_PH(sacc, 2);   // barrier 1
    after_b1();

    // ---- P2: row masses in ATen order (sot_device.hpp)
    const MassPlan mp = make_mass_plan(RT ? a.n : N);   // used by the run-time-length rows only
    if constexpr (COLUMNS) {
        // chunk sums came out of the fetched registers in P1
    } else if constexpr (RT) {   // the summation plan follows the REAL length: the generic chunk sums (sot_device.hpp), x then y
        mass_chunk_sums<G, SQ>(U, part, mp, t);
        if (!dn) mass_chunk_sums<G, SQ>(V, part + NT, mp, t);
    } else {
#pragma unroll
    for (int id0 = 0; id0 < 2 * NT; id0 += G) {
        const int id = id0 + t;
        const bool isy = id >= NT;
        if (id < 2 * NT && !(isy && dn)) {
            const int task = isy ? id - NT : id;
            const float* src = (isy ? V : U) + ((task >> 5) << 9) + (task & 31);
            const float* srco = (isy ? V : U) + ((task >> 5) << 9) + ((task & 31) ^ (SWZ ? 4 : 0));  // odd steps: bit 5 set
            float v[CHUNK];
#pragma unroll
            for (int s2 = 0; s2 < CHUNK; ++s2) { const float w = ((s2 & 1) ? srco : src)[s2 << 5]; v[s2] = SQ ? w * w : w; }
            float acc = 0.0f;
#pragma unroll
            for (int s2 = 0; s2 < CHUNK; ++s2) acc += v[s2];
            part[id] = acc;
        }
    }
    }
    SOT_PH(sacc, 3);   // chunk sums
    if constexpr (!COLUMNS) row_sync<NW>();
    SOT_PH(sacc, 4);   // barrier 2
    // ... columns + fold by one wave per array (wave 0: x, wave 1: y; a one-wave row uses its half-waves)
    __builtin_amdgcn_s_setprio(kMassPrio);
    if (NW >= 2) {
        if (wv < 2 && !(wv == 1 && dn)) {
            const float* raw = wv ? V : U;
            float* cb = colbuf + 32 * wv;
            if (lane < 32) {
                if constexpr (RT) cb[lane] = mass_column<SQ>(raw, part + wv * NT, mp, lane);
                else cb[lane] = mass_column_nx<Geo::NSTEPS>(part + wv * NT, lane);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float S;
            if constexpr (RT) S = mass_fold<SQ>(raw, cb, mp.n);
            else S = mass_fold_nx<(SQ && !PRESQ), N, SWZ>(raw, cb);
            if (lane == 0) { Sv[wv] = S; Sv[2 + wv] = 1.0f / guard_mass(S); }
        }
    } else {
        const int half = lane >> 5, col = lane & 31;
        const bool use_y = half && !dn;
        float* cb = colbuf + 32 * half;
        if constexpr (RT) cb[col] = mass_column<SQ>(use_y ? V : U, part + (use_y ? NT : 0), mp, col);
        else cb[col] = mass_column_nx<Geo::NSTEPS>(part + (use_y ? NT : 0), col);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float S;
        if constexpr (RT) S = mass_fold<SQ>(use_y ? V : U, cb, mp.n);
        else S = mass_fold_nx<(SQ && !PRESQ), N, SWZ>(use_y ? V : U, cb);
        if (col == 0) { Sv[half] = S; Sv[2 + half] = 1.0f / guard_mass(S); }
    }
    __builtin_amdgcn_s_setprio(0);
    // the CPT contiguous elements this thread owns in sorted order (overlaps the other waves' fold)
    const int e0 = t * CPT;
    const int h0 = e0 + 4 * ownf, h1 = e0 + 4 * (1 - ownf);  // where the first / second half of the owned block is staged
    if (x_ident) {
        if constexpr (CPT == 8) {
            const float4 v0 = *reinterpret_cast<const float4*>(U + h0), v1 = *reinterpret_cast<const float4*>(U + h1);
            wx[0] = v0.x; wx[1] = v0.y; wx[2] = v0.z; wx[3] = v0.w; wx[4] = v1.x; wx[5] = v1.y; wx[6] = v1.z; wx[7] = v1.w;
        } else {
#pragma unroll
            for (int k = 0; k < CPT; ++k) wx[k] = U[e0 + k];
        }
    } else if (psx != nullptr) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) wx[k] = U[psx[k]];
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int sx = (e0 + k < (RT ? a.n : N)) ? a.xperm[e0 + k] : N + 1;  // N + 1: a zero slot (or spare, masked below)
            wx[k] = U[SWZ ? (sx ^ (((sx >> 5) & 1) << 2)) : sx];
        }
    }
    if (y_ident) {
        if constexpr (CPT == 8) {
            const float4 v0 = *reinterpret_cast<const float4*>(V + h0), v1 = *reinterpret_cast<const float4*>(V + h1);
            wy[0] = v0.x; wy[1] = v0.y; wy[2] = v0.z; wy[3] = v0.w; wy[4] = v1.x; wy[5] = v1.y; wy[6] = v1.z; wy[7] = v1.w;
        } else {
#pragma unroll
            for (int k = 0; k < CPT; ++k) wy[k] = V[e0 + k];
        }
    } else if (psy != nullptr) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) wy[k] = V[psy[k]];
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int sy = (e0 + k < (RT ? a.n : N)) ? a.yperm[e0 + k] : N + 1;
            wy[k] = V[SWZ ? (sy ^ (((sy >> 5) & 1) << 2)) : sy];
        }
    }
    if ((N < Geo::CAP || RT) && e0 + CPT > (RT ? a.n : N)) {  // the thread holding the end of the row, and those past it: sentinel / spare slots -> weight 0
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            if (e0 + k >= (RT ? a.n : N)) { wx[k] = 0.0f; wy[k] = 0.0f; }
        }
    }
    SOT_PH(sacc, 5);   // fold (waves 0, 1) / owner reads
    row_sync<NW>();
    SOT_PH(sacc, 6);   // barrier 3

    // ---- P3: safe_divide + fp64-accumulated CDFs (the sequence of build_cdfs)
    Sx = Sv[0]; Sy = dn ? Sx : Sv[1];
    const float rSx = Sv[2], rSy = dn ? rSx : Sv[3];
    const float Sxh = guard_mass(Sx), Syh = guard_mass(Sy);
    double px[CPT], py[CPT];
    double runx = 0.0, runy = 0.0;
    {
        float qx[CPT], qy[CPT];
        uint32_t risk = 0xFFFFFFFFu;
        if constexpr (PLAIN && CPT % 2 == 0) {
            // the owned elements sit in consecutive registers (two 16-byte LDS reads per array): the division on pairs, written out so
            // that it does not hang on the vectoriser.  The operand screen costs one v_min3_u32 per two elements instead of a subtraction
            // per element on top: `low` is the smallest operand pattern, zeros included, and no operand in [1, 2^-78] can hide above it,
            // so the exact test (which tells a zero from a tiny weight) runs only in waves that hold a zero or a tiny weight
            static_assert(!(SQ && !PRESQ), "the plain loop stages squares: the operands are wx / wy as read");
            uint32_t low = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < CPT; k += 2) {
                const f32x2 q = div_by_row_constant(f32x2{wx[k], wx[k + 1]}, Sxh, rSx), r = div_by_row_constant(f32x2{wy[k], wy[k + 1]}, Syh, rSy);
                qx[k] = q.x; qx[k + 1] = q.y; qy[k] = r.x; qy[k + 1] = r.y;
            }
#pragma unroll
            for (int k = 0; k < CPT; ++k) low = min(min(low, __float_as_uint(wx[k])), __float_as_uint(wy[k]));
            if (__builtin_amdgcn_ballot_w64(low <= kFastDivMinBits) != 0ull) {   // risk < kFastDivMinBits implies this
#pragma unroll
                for (int k = 0; k < CPT; ++k) risk = min(risk, min(__float_as_uint(wx[k]) - 1u, __float_as_uint(wy[k]) - 1u));
            }
        } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            qx[k] = div_by_row_constant((SQ && !PRESQ) ? wx[k] * wx[k] : wx[k], Sxh, rSx, risk);
            qy[k] = div_by_row_constant((SQ && !PRESQ) ? wy[k] * wy[k] : wy[k], Syh, rSy, risk);
        }
        }
        const bool slow = (risk < kFastDivMinBits) || !(Sxh <= 0x1p40f) || !(Syh <= 0x1p40f);
        if (__builtin_amdgcn_ballot_w64(slow) != 0ull) {  // rare, wave-uniform (see build_cdfs)
            asm volatile("; IEEE division fallback" ::: "memory");
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                qx[k] = ((SQ && !PRESQ) ? wx[k] * wx[k] : wx[k]) / Sxh;
                qy[k] = ((SQ && !PRESQ) ? wy[k] * wy[k] : wy[k]) / Syh;
            }
        }
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            runx += (double)qx[k]; runy += (double)qy[k];
            px[k] = runx; py[k] = runy;
        }
    }
    const double inx = wave_incl_scan(runx), iny = wave_incl_scan(runy);
    double exx = wave_shift_right1(inx), exy = wave_shift_right1(iny);
    if (NW > 1 && lane == kWave - 1) { wtot[wv] = inx; wtot[NW + wv] = iny; }
    SOT_PH(sacc, 7);   // division, fp64 accumulation, wave scans
    row_sync<NW>();  // raw weights are consumed, wave totals are visible
    SOT_PH(sacc, 8);   // barrier 4
    if constexpr (NW > 1 && (NW > kPrefixSelectMaxWaves || GRAD != 0)) {   // totals of the waves in front of this one, added in wave order ((0 + w0) + w1) + ...
        double ox = 0.0, oy = 0.0;
        for (int w = 0; w < wv; ++w) { ox += wtot[w]; oy += wtot[NW + w]; }
        exx += ox; exy += oy;
    } else if constexpr (NW > 1) {
        // the same sum in the same order for forward rows of up to four waves: every total is read at its fixed address in one LDS round trip and
        // the sum is formed with wave-uniform selects -- no loop whose trip count is the wave's index
        double tx[NW - 1], ty[NW - 1];
#pragma unroll
        for (int w = 0; w < NW - 1; ++w) { tx[w] = wtot[w]; ty[w] = wtot[NW + w]; }
        double ox = 0.0, oy = 0.0;
        if constexpr (PLAIN) {
            // the plain loop: the same sums under an early exit on the wave's index -- as compiled, wave 0 branches around the LDS reads and the
            // adds, waves 1 ... 3 pick their sum with 8 v_cndmask instead of 12.  (A switch over the wave's index, no select at all, measured
            // no better: profiles/area_valu_diet.txt)
#pragma unroll
            for (int w = 0; w < NW - 1; ++w) {
                if (w >= wv) break;
                ox += tx[w]; oy += ty[w];
            }
        } else {
#pragma unroll
        for (int w = 0; w < NW - 1; ++w) {
            const double sx = ox + tx[w], sy = oy + ty[w];
            ox = (w < wv) ? sx : ox; oy = (w < wv) ? sy : oy;
        }
        }
        exx += ox; exy += oy;
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) { cu[k] = (float)(exx + px[k]); cv[k] = (float)(exy + py[k]); }
    if constexpr (TO_LDS) {
        if (CPT % 4 == 0 && (N == Geo::CAP || e0 + CPT <= N)) {
#pragma unroll
            for (int k = 0; k + 3 < CPT; k += 4) {
                *reinterpret_cast<float4*>(U + e0 + k) = make_float4(cu[k], cu[k + 1], cu[k + 2], cu[k + 3]);
                *reinterpret_cast<float4*>(V + e0 + k) = make_float4(cv[k], cv[k + 1], cv[k + 2], cv[k + 3]);
            }
        } else {  // the end of the row: the sentinel at N and the zero slots behind it stay as they are
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                if (e0 + k < N) { U[e0 + k] = cu[k]; V[e0 + k] = cv[k]; }
            }
        }
    }
    // the next row's loads are issued here (not in P1): their 2*CPT destination registers are then live only during the merge
    // phases, whose register demand is small, instead of across the register-hungry division / scan (8192 x 2048: 45.6 -> 44.8 us).
    // The merge-free kernel has no walk to hide them behind, yet issuing them right behind barrier 1 in its plain loop (no more
    // registers: 118 either way) was slower, 33.4 against 32.2 us per headline step (profiles/f8_area_plain_loop.txt)
    if (nxt_x != nullptr) fetch_row<G, CPT, NX, WT>(nxt_x, nxt_y, t, a.n, rx, ry);
    if constexpr (TO_LDS) row_sync<NW>();
}

// RP (per-row positions through handed-over permutations, see sot_forward_full_kernel): row `rowc`'s sorted positions into the position copy behind
// the row region, its permutations into ix / iy (original columns of the thread's CPT owned sorted elements) and psx / psy (their staged LDS indices).
// Two row barriers: the natural positions are staged in the U / V regions, which full_build_cdfs then overwrites with the weights.
template <int G, int CPT, int ROWS, int GRAD, int NX>
__device__ __forceinline__ void rowpos_row_setup(const FwdArgs& a, const FullCtx& c, int64_t rowc, int (&ix)[CPT], int (&iy)[CPT], int (&psx)[CPT], int (&psy)[CPT])
{
    using Geo = FullGeo<G, CPT, ROWS, GRAD, NX>;
    constexpr int N = Geo::N, NW = Geo::NW, PAD = Geo::PAD;
    static_assert(ROWS == 1 && NX == 0 && CPT == 8, "per-row positions: one row per workgroup, rows that fill the 8-element geometry");
    const int t = c.t;
    const uint16_t* const pr = a.perm_in + rowc * (2 * (int64_t)N);
    const float* const xp = a.xpos + rowc * a.xps;
    const float* const yp = a.ypos + rowc * a.yps;
    const uint4 qx = *reinterpret_cast<const uint4*>(pr + t * CPT), qy = *reinterpret_cast<const uint4*>(pr + N + t * CPT);
    float vx[CPT], vy[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) { vx[k] = xp[t + k * G]; vy[k] = yp[t + k * G]; }
    const uint32_t wqx[4] = {qx.x, qx.y, qx.z, qx.w}, wqy[4] = {qy.x, qy.y, qy.z, qy.w};
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        ix[k] = (int)((wqx[k >> 1] >> (16 * (k & 1))) & (uint32_t)(N - 1));     // (masked: never outside the row)
        iy[k] = (int)((wqy[k >> 1] >> (16 * (k & 1))) & (uint32_t)(N - 1));
        psx[k] = Geo::SWZ ? (ix[k] ^ (((ix[k] >> 5) & 1) << 2)) : ix[k];
        psy[k] = Geo::SWZ ? (iy[k] ^ (((iy[k] >> 5) & 1) << 2)) : iy[k];
    }
    float* const Um = c.U; float* const Vm = c.V;
#pragma unroll
    for (int k = 0; k < CPT; ++k) { Um[t + k * G] = vx[k]; Vm[t + k * G] = vy[k]; }
    row_sync<NW>();
    float gx[CPT], gy[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) { gx[k] = Um[ix[k]]; gy[k] = Vm[iy[k]]; }
    float* const PXw = const_cast<float*>(c.PX); float* const PYw = const_cast<float*>(c.PY);
    *reinterpret_cast<float4*>(PXw + t * CPT) = make_float4(gx[0], gx[1], gx[2], gx[3]);
    *reinterpret_cast<float4*>(PXw + t * CPT + 4) = make_float4(gx[4], gx[5], gx[6], gx[7]);
    *reinterpret_cast<float4*>(PYw + t * CPT) = make_float4(gy[0], gy[1], gy[2], gy[3]);
    *reinterpret_cast<float4*>(PYw + t * CPT + 4) = make_float4(gy[4], gy[5], gy[6], gy[7]);
    if (t < PAD) PXw[t - PAD] = gx[0];                                  // any finite value: the padded levels have zero width
    if (t == G - 1) { PXw[N] = gx[CPT - 1]; PYw[N] = gy[CPT - 1]; }     // clamp of losses.py:220: ranks beyond the last index reuse it
    row_sync<NW>();   // the gathers are done before the weights are staged over them; the position copy is published by the barriers of the CDF build
}

}  // namespace sot
