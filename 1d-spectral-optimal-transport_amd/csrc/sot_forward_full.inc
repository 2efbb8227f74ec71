// sot_forward_full.inc -- kernel and launch templates of the full-row kernels (compile-time geometries), namespace sot.  Included by
// the four objects that instantiate them: sot_full_fwd.hip, sot_full_bwd.hip (compile-time row lengths), sot_full_rt_fwd.hip,
// sot_full_rt_bwd.hip (run-time row lengths).  The non-template dispatch functions live there: dispatch_forward_full and
// dispatch_area_full in sot_full_fwd.hip, dispatch_backward_full and dispatch_area_train in sot_full_bwd.hip.
//
// Full-row forward kernel: the row pipeline of sot_forward_kernel for row lengths known at compile time: rows that fill
// their geometry exactly (n == m == G*CPT = 512, 2048 or 8192; 16-B aligned rows) and the paper's 257 / 513 / 1025 bins
// (n_fft 512 / 1024 / 2048; any alignment; template parameter NX); shared positions, p in {1, 2}, not pre-normalised.
// Every length, the LDS layout, the ATen summation plan and the merge-walk trip count are compile-time
// constants: no per-element bounds predicates, no generic chunk loops, LDS offsets folded into the
// instructions, and the walk advances two LDS byte offsets instead of recomputing addresses from indices.
// Same arithmetic, operation for operation, as the generic kernel: for 512 / 2048 / 8192 bins row losses and gradients
// are bit-identical (tests/test_gpu_parity.py::test_full_row_kernel_matches_generic); for 257 / 513 / 1025 bins the
// thread geometry differs from the generic kernel's, so sums are associated differently (agreement to ~1e-7).
// A workgroup holds ROWS rows (one row group of G threads each) and ONE copy of the support positions, placed behind
// the row regions with the same internal offsets, so that "position of the element at LDS offset o of row r" is
// o + (ROWS - r) * rowf: a compile-time immediate per row group (512-bin rows: four rows per 256-thread workgroup).
// Reference semantics: losses.py:172-196, :271-313, :214-220; utils.py:135-142.
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

// the one-wave-per-row forward kernels of 1025-bin rows (17 elements per thread): 152 / 154 VGPRs = three waves per SIMD; held to four
// (128 VGPRs, spills): 16384 x 1025 paper mode 41.5 -> 77.4 us, p = 1 28.8 -> 47.0 us -- left alone
constexpr int kFwd17MinWaves = 1;
// Unroll factor of the merge walks in this file (trip count E is a compile-time constant, 3 ... 17).  Round 3: 32 = complete unrolling
// (the loop-carried register moves of the partially unrolled form disappear): paper-mode forward 8192 x 2048 45.9 -> 44.1 us, training
// form 79.7 -> 78.7 us (profiles/r3_walk_experiments_ab.txt); round 1-2 default was 2 (SOT_WALK_UNROLL of the generic kernels).
#define SOT_FULL_WALK_UNROLL 32
// (Round 3: two / three / four shorter merge segments per thread in the forward kernel, their search and walk chains interleaved, were
// slower -- paper-mode forward 45.8 -> 49.1 / 54.3 / 57.8 us: these phases are bound by instructions issued, not by the latency of their chains.)

constexpr int kFwd1025OneWaveRows = 6144;   // batches of at least this many 1025-bin rows: one wave per row in the forward kernel
constexpr int kRt1024OneWaveRows = 8192;    // the same for run-time lengths on the 1024-point geometry (16 elements per thread)

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
template <int G, int CPT, int NX>
__device__ __forceinline__ void fetch_row(const float* __restrict__ x, const float* __restrict__ y, int t, int n, float (&rx)[CPT], float (&ry)[CPT]);

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
template <int G, int CPT>
__device__ __forceinline__ void fetch_row_columns(const float* __restrict__ x, const float* __restrict__ y, int t, float (&rx)[CPT], float (&ry)[CPT])
{
    static_assert(CPT == 8, "16 steps per task: two registers arrays of 8");
    const bool isy = t >= G / 2;
    const int task = isy ? t - G / 2 : t;
    const float* const src = (isy ? y : x) + ((task >> 5) << 9) + (task & 31);
#pragma unroll
    for (int k = 0; k < 8; ++k) { rx[k] = src[k << 5]; ry[k] = src[(8 + k) << 5]; }
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

template <int G, int CPT, int NX>
__device__ __forceinline__ void fetch_row(const float* __restrict__ x, const float* __restrict__ y, int t, int n, float (&rx)[CPT], float (&ry)[CPT])
{
    if constexpr (NX == 0) fetch_row_columns<G, CPT>(x, y, t, rx, ry);
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
// past n carry zero weight and sit at the row's LAST position: zero-weight points are inert (SURVEY A.2) as long as they do not move
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

// E steps of the merge for one thread (losses.py:295-313) in "loser" form: (w, wp) is the head fetched last, (r, rp) the
// head that lost the previous comparison; the smaller one is consumed and only ITS stream is read again, so the fetched
// level and position become the new (w, wp) without any select: 10 VALU per step instead of 15.  Equal heads may be
// consumed in either order (w first here, U first in the canonical stable order): the pair of heads is the same either
// way, so the consumed level, its width and its cost factor are identical, and the second member of a tie has zero
// width -- the accumulated sum is bit-identical to the canonical order's.
// ou / ov: 32-bit LDS byte addresses of the two heads; the position of the element at address o is at o + POFF4.
// (Carrying generic pointers instead costs one more select per step: 3.6 % slower.)
template <int E, int PM, bool LIM, uint32_t POFF4>
__device__ __forceinline__ float merge_walk_full(uint32_t ou, uint32_t ov, bool first, float p)
{
    float w = lds_load(ou), wp = lds_load(ou + POFF4);
    float r = lds_load(ov), rp = lds_load(ov + POFF4);
    float qprev = fmaxf(lds_load(ou - 4u), lds_load(ov - 4u));
    if (first) qprev = 0.0f;  // Q_0 := 0 (the pad of losses.py:301)
    uint32_t pw = ou + 4u, pr = ov + 4u;  // next unread element of w's / r's stream
    float acc = 0.0f;
#pragma unroll SOT_FULL_WALK_UNROLL
    for (int s2 = 0; s2 < E; ++s2) {
        const bool c = w <= r;
        const float q = c ? w : r;
        const float cost = transport_cost<PM>(wp, rp, p);
        float delta = q - qprev;
        if (LIM && q > 1.0f) delta = 0.0f;
        acc = fmaf(delta, cost, acc);  // fused: no worse than the reference's separate rounding
        qprev = q;
        const uint32_t nx = c ? pw : pr;
        pr = c ? pr : pw;
        pw = nx + 4u;
        r = c ? r : w;
        rp = c ? rp : wp;
        w = lds_load(nx);
        wp = lds_load(nx + POFF4);
    }
    return acc;
}

// P1-P3 of one row: raw weights -> LDS, row masses in ATen order, safe_divide, fp64-accumulated CDFs into U / V (ends
// with the barrier that publishes them).  rx / ry: this row's weights (coalesced float4 layout), refilled with the next
// row's (nxt_x / nxt_y, null at the end); wx / wy: the CPT contiguous raw weights this thread owns in sorted order.
// TO_LDS = false (the merge-free p = 1 kernel): the CDFs of the thread's own CPT elements are only returned in cu / cv,
// nothing is written to U / V and the closing barrier is left out (the barrier behind the raw reads already orders the next
// row's staging behind this row's last LDS read of the raw weights).
// RAW_OUT: wx / wy must be the weights as given (a gradient needs them); otherwise square_dist rows may be staged as their squares
template <int G, int CPT, int ROWS, int GRAD, bool SQ, int NX = 0, bool TO_LDS = true, bool RAW_OUT = (GRAD != 0)>
__device__ __forceinline__ void full_build_cdfs(const FwdArgs& a, const FullCtx& c, float (&rx)[CPT], float (&ry)[CPT],
                                                const float* nxt_x, const float* nxt_y, float (&wx)[CPT], float (&wy)[CPT],
                                                float& Sx, float& Sy, float (&cu)[CPT], float (&cv)[CPT], unsigned long long* sacc = nullptr,
                                                const int* psx = nullptr, const int* psy = nullptr)
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
    const bool dn = c.dn, x_ident = c.x_ident, y_ident = c.y_ident;
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
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            qx[k] = div_by_row_constant((SQ && !PRESQ) ? wx[k] * wx[k] : wx[k], Sxh, rSx, risk);
            qy[k] = div_by_row_constant((SQ && !PRESQ) ? wy[k] * wy[k] : wy[k], Syh, rSy, risk);
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
    if constexpr (NW > 1) {
        double ox = 0.0, oy = 0.0;
        for (int w = 0; w < wv; ++w) { ox += wtot[w]; oy += wtot[NW + w]; }
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
    // phases, whose register demand is small, instead of across the register-hungry division / scan (8192 x 2048: 45.6 -> 44.8 us)
    if (nxt_x != nullptr) fetch_row<G, CPT, NX>(nxt_x, nxt_y, t, a.n, rx, ry);
    if constexpr (TO_LDS) row_sync<NW>();
}

// staged LDS indices of the CPT elements thread t owns in sorted order on a permuted shared grid (see full_build_cdfs: psx / psy)
template <int G, int CPT, int ROWS, int NX>
__device__ __forceinline__ void owner_perm_slots(const FwdArgs& a, const int* perm, int t, int (&ps)[CPT])
{
    using Geo = FullGeo<G, CPT, ROWS, false, NX>;
    constexpr int N = Geo::N;
    const int nreal = Geo::RT ? a.n : N;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int sx = (t * CPT + k < nreal) ? perm[t * CPT + k] : N + 1;
        ps[k] = Geo::SWZ ? (sx ^ (((sx >> 5) & 1) << 2)) : sx;
    }
}

// Geometry experiments on 8192 x 2048 (all slower than one 256-thread row per workgroup, 4 workgroups per CU, 44.8 us):
// two rows per 512-thread workgroup sharing the positions: 46.5 us at the same 4 rows per CU; held to 96 VGPRs 52.3 us,
// to 80 VGPRs (6 rows per CU, 26 dwords spilled) 74 us; 512 threads x 4 elements per row 53-54 us.
constexpr int kFwdMinWaves = 1;
// (The run-time-length kernel of the 4096-point geometry came out at 129 VGPRs: one 512-thread workgroup per CU instead of the two its LDS allows;
//  held to 128 -- four waves per SIMD -- 4096 x 4000 paper mode: see profiles/r4p_segmented_sort.txt, "register steps".)
constexpr int kRt512MinWaves = 4;

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

// RP (round 6): PER-ROW positions whose sort permutations are handed in (a.perm_in: [B, 2 N] uint16, written by sot_rowpos_sort_kernel or an earlier
// forward): every row brings its own positions -- loaded coalesced, staged in the U / V regions, gathered through the permutation into the
// position copy behind the row region -- and its weights are read through the same permutation (the psx / psy path of a permuted shared grid).
// One row per workgroup only (the position copy is the row's own), rows that fill their geometry (NX == 0).
template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX = 0, bool RP = false>
__global__ __launch_bounds__(ROWS * G, (G == 512 && NX < 0) ? kRt512MinWaves : (CPT == 17) ? kFwd17MinWaves : kFwdMinWaves) void sot_forward_full_kernel(const FwdArgs a)
{
    static_assert(!RP || (ROWS == 1 && NX == 0 && CPT == 8), "per-row positions: one row per workgroup, rows that fill the 8-element geometry");
    using Geo = FullGeo<G, CPT, ROWS, false, NX>;
    constexpr FullLayout L = Geo::L;
    constexpr int N = Geo::N, NW = Geo::NW, E = Geo::E, GA = Geo::GA, PAD = Geo::PAD;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t row_step = (int64_t)gridDim.x * ROWS;
    int64_t row0 = (int64_t)blockIdx.x * ROWS;
    float rx[CPT], ry[CPT];
    FullCtx cm = full_setup<G, CPT, ROWS, false, NX, RP>(a, smem);
    if constexpr (RP) { cm.x_ident = false; cm.y_ident = false; }
    const FullCtx c = cm;
    if constexpr (NW == 1) __syncthreads();   // the position copy is shared by the row groups, whose rows then run wave-synchronised
    const int rg = c.rg, t = c.t, lane = c.lane, wv = c.wv;
    float* const V = c.V; float* const red = c.red;
    const float* const Uw = c.Uw;
    if (row0 < a.B) {
        const int64_t r = min(row0 + rg, a.B - 1);
        fetch_row<G, CPT, NX>(a.x + r * a.xs, a.y + r * a.ys, t, a.n, rx, ry);
    }

#ifdef SOT_STAMPS
    unsigned long long sbuf[16] = {};
    unsigned long long* const sacc = (threadIdx.x == 0 && blockIdx.x == gridDim.x / 2) ? sbuf : nullptr;
#else
    constexpr unsigned long long* sacc = nullptr;
#endif
    // (2 CPT registers for the whole row loop: only where they do not cost a wave per SIMD -- the 17-element one-wave rows keep the per-row lookup)
    constexpr bool HOIST_PERM = CPT <= 9;
    int psx[HOIST_PERM ? CPT : 1] = {}, psy[HOIST_PERM ? CPT : 1] = {};
    if constexpr (HOIST_PERM && !RP) {
        if (!c.x_ident) owner_perm_slots<G, CPT, ROWS, NX>(a, a.xperm, t, psx);
        if (!c.y_ident) owner_perm_slots<G, CPT, ROWS, NX>(a, a.yperm, t, psy);
    }
    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rg;
        const bool valid = row < a.B;
        const bool more = row0 + row_step < a.B;
        const int64_t rn = min(row0 + row_step + rg, a.B - 1);
        float wx[CPT], wy[CPT], cu[CPT], cv[CPT];
        float Sx, Sy;
#ifdef SOT_STAMPS
        if (sacc != nullptr) sacc[15] = __builtin_readcyclecounter();
#endif
        if constexpr (RP) {
            int ix[CPT], iy[CPT];
            rowpos_row_setup<G, CPT, ROWS, false, NX>(a, c, min(row, a.B - 1), ix, iy, psx, psy);
        }
        full_build_cdfs<G, CPT, ROWS, false, SQ, NX>(a, c, rx, ry, more ? a.x + rn * a.xs : nullptr,
                                                     more ? a.y + rn * a.ys : nullptr, wx, wy, Sx, Sy, cu, cv, sacc, HOIST_PERM ? psx : nullptr,
                                                     HOIST_PERM ? psy : nullptr);
        SOT_PH(sacc, 9);   // wave totals, CDF values to LDS, next row's loads issued, barrier

        // ---- P4: merge of the two CDFs (losses.py:295-313), E steps per thread
        float acc = 0.0f;
        __builtin_amdgcn_s_setprio(kWalkPrio);
        // (Thread t merges segment t.  Permuting the segments over the lanes -- segment 19 t mod G etc., to change the LDS bank
        // pattern of the walk -- was measured 1.5-6 % slower for ten multipliers; E = 16 instead of 17 is 13 % slower.)
        if (GA == G || t < GA) {
            constexpr int VOFF = L.nU - L.padcap + PAD;  // V - Uw in floats
            const int D0 = t * E;
            (void)VOFF;
            const uint32_t ub1 = lds_addr(Uw) - 4u;                        // address of Uw[-1]
            const uint32_t vd1 = lds_addr(V) + 4u * (uint32_t)D0 + ub1;    // address of V[D0], + ub1
            const uint32_t pb = merge_path_fixed32<N + PAD, N>(ub1, vd1, D0);  // address of Uw[i0 - 1]
            SOT_PH(sacc, 10);  // partition search
            const uint32_t ou = pb + 4u;     // address of Uw[i0]
            const uint32_t ov = vd1 - pb;    // address of V[D0 - i0]
            constexpr uint32_t ROWB = 4u * (uint32_t)L.rowf;  // the positions lie (ROWS - rg) row regions behind this row
            if (ROWS == 1 || rg == ROWS - 1) acc = merge_walk_full<E, PM, LIM, ROWB>(ou, ov, D0 == 0, a.p);
            else if (ROWS == 2 || rg == ROWS - 2) acc = merge_walk_full<E, PM, LIM, 2u * ROWB>(ou, ov, D0 == 0, a.p);
            else if (ROWS == 3 || rg == ROWS - 3) acc = merge_walk_full<E, PM, LIM, 3u * ROWB>(ou, ov, D0 == 0, a.p);
            else acc = merge_walk_full<E, PM, LIM, 4u * ROWB>(ou, ov, D0 == 0, a.p);
        }
        __builtin_amdgcn_s_setprio(0);
        SOT_PH(sacc, 11);  // merge walk
        acc = wave_sum(acc);
        if (NW == 1) {
            if (lane == 0 && valid && a.row_loss) store_row_loss(a.row_loss, row, acc, a.mt.counters != nullptr);
            row_sync<NW>();  // this row's LDS reads are done before the next row's staging
        } else {
            if (lane == 0) red[wv] = acc;
            row_sync<NW>();
            if (t == 0 && valid && a.row_loss) {
                float tot = red[0];
#pragma unroll
                for (int w = 1; w < NW; ++w) tot += red[w];
                store_row_loss(a.row_loss, row, tot, a.mt.counters != nullptr);
            }
        }
        SOT_PH(sacc, 12);  // wave sum, barrier, store
#ifdef SOT_STAMPS
        if (sacc != nullptr) sacc[0] += 1;
#endif
    }
#ifdef SOT_STAMPS
    if (sacc != nullptr) { for (int i = 0; i < 16; ++i) g_stamps[i] = sacc[i]; }
#endif
    if (a.mt.counters != nullptr) batch_mean_tail<ROWS * G>(a.mt, a.row_loss, a.B, reinterpret_cast<double*>(smem));
}

// ---------------------------------------------------------------------------------------------
// Merge-free forward for p = 1 when both measures live on ONE sorted grid (SOT_FLAG_SAME_GRID; every reference call site:
// y_pos = x_pos.clone() in trainer.py:191, the fixed_x buffer of metrics.py:148), no quantile cutoff.
//
// For p = 1 the loss  sum_k (Q_k - Q_{k-1}) |uq_k - vq_k|  (losses.py:301-313) is the area between the two inverse CDFs
// q -> xs[min(#{U < q}, n-1)] and q -> ys[min(#{V < q}, m-1)] over q in (0, max(U_last, V_last)].  Read along the position
// axis instead of the level axis, the same area is  integral |U~(s) - V~(s)| ds  with U~(s) = U_i on [xs_i, xs_{i+1}) and
// U~ = V~ = max(U_last, V_last) from the last support point on (the clamp of losses.py:220 maps every level beyond a
// measure's total mass to its last point).  On a common grid both step functions jump at the same places, hence
//        loss = sum_{i < n-1} |U_i - V_i| (xs_{i+1} - xs_i):
// no sort of cat(U, V), no searchsorted, no gather -- the CDF values never leave the registers of the thread that
// scanned them.  Same fp32 U, V as the merge kernel (shared CDF builder); the two closed forms differ only in the rounding
// of 2047 non-negative products and their sum (observed <= 3e-7 relative; tests pin it to the reference at 1e-5).
// The row pipeline shrinks to staging, ATen-ordered masses, division, fp64 scans and one fused multiply-add per element:
// 5 barriers per row instead of 8, 18 KB of LDS per 2048-bin row instead of 34.5 KB.
// ---------------------------------------------------------------------------------------------
constexpr int kAreaMinWaves = 1;
template <int G, int CPT, int ROWS, bool SQ, int NX = 0>
__global__ __launch_bounds__(ROWS * G, (CPT == 17) ? kFwd17MinWaves : kAreaMinWaves) void sot_area_full_kernel(const FwdArgs a)
{
    using Geo = FullGeo<G, CPT, ROWS, false, NX>;
    constexpr FullLayout L = Geo::L;
    constexpr int N = Geo::N, NW = Geo::NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];   // ROWS row regions; no position copy
    const int64_t row_step = (int64_t)gridDim.x * ROWS;
    int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int tid = threadIdx.x;
    FullCtx c;
    c.rg = __builtin_amdgcn_readfirstlane(tid / G);
    c.t = tid - c.rg * G;
    c.lane = tid & (kWave - 1);
    c.wv = __builtin_amdgcn_readfirstlane(c.t >> 6);
    const int rg = c.rg, t = c.t, lane = c.lane, wv = c.wv;
    float rx[CPT], ry[CPT];
    if (row0 < a.B) {
        const int64_t r = min(row0 + rg, a.B - 1);
        fetch_row<G, CPT, NX>(a.x + r * a.xs, a.y + r * a.ys, t, a.n, rx, ry);
    }
    c.dn = a.flags & SOT_FLAG_DONT_NORMALIZE;
    float* const base = smem + rg * L.rowf;
    c.U = base + L.padcap; c.V = base + L.nU; c.part = base + L.part; c.colbuf = base + L.colbuf;
    c.wtot = reinterpret_cast<double*>(base + L.wtot);
    c.red = base + L.red; c.Sv = c.red + NW;
    c.Uw = c.U; c.PX = nullptr; c.PY = nullptr;
    c.x_ident = true; c.y_ident = true;
    if (a.ident != nullptr) { c.x_ident = a.ident[0] != 0; c.y_ident = a.ident[1] != 0; }
    // widths of the grid cells behind the CPT elements this thread owns (sorted order); 0 behind the last point.  (Kept in
    // registers: a table in LDS read per row -- 97 -> 96 VGPRs, 5 waves per SIMD -- measured 31.0 instead of 30.3 us.)
    float dx[CPT];
    {
        const int e0 = t * CPT;
        float pe[CPT + 1];
        const int nreal = Geo::RT ? a.n : N;   // points past a run-time-length row sit at its last position: cells of width 0
#pragma unroll
        for (int k = 0; k <= CPT; ++k) pe[k] = a.xpos[min(e0 + k, nreal - 1)];
#pragma unroll
        for (int k = 0; k < CPT; ++k) dx[k] = (e0 + k + 1 < nreal) ? pe[k + 1] - pe[k] : 0.0f;
    }
    float* const red = c.red;
#ifdef SOT_STAMPS
    unsigned long long sbuf[16] = {};
    unsigned long long* const sacc = (threadIdx.x == 0 && blockIdx.x == gridDim.x / 2) ? sbuf : nullptr;
#endif

    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rg;
        const bool valid = row < a.B;
        const bool more = row0 + row_step < a.B;
        const int64_t rn = min(row0 + row_step + rg, a.B - 1);
        float wx[CPT], wy[CPT], cu[CPT], cv[CPT];
        float Sx, Sy;
#ifdef SOT_STAMPS
        if (sacc != nullptr) sacc[15] = __builtin_readcyclecounter();
        full_build_cdfs<G, CPT, ROWS, false, SQ, NX, false>(a, c, rx, ry, more ? a.x + rn * a.xs : nullptr,
                                                            more ? a.y + rn * a.ys : nullptr, wx, wy, Sx, Sy, cu, cv, sacc);
        SOT_PH(sacc, 9);   // wave totals, CDF values, next row's loads issued
#else
        full_build_cdfs<G, CPT, ROWS, false, SQ, NX, false>(a, c, rx, ry, more ? a.x + rn * a.xs : nullptr,
                                                            more ? a.y + rn * a.ys : nullptr, wx, wy, Sx, Sy, cu, cv);
#endif
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < CPT; ++k) acc = fmaf(fabsf(cu[k] - cv[k]), dx[k], acc);
        acc = wave_sum(acc);
        if (NW == 1) {
            if (lane == 0 && valid && a.row_loss) store_row_loss(a.row_loss, row, acc, a.mt.counters != nullptr);
            row_sync<NW>();  // red / Sv of this row are consumed before the next row rewrites them
        } else {
            if (lane == 0) red[wv] = acc;
            row_sync<NW>();
            if (t == 0 && valid && a.row_loss) {
                float tot = red[0];
#pragma unroll
                for (int w = 1; w < NW; ++w) tot += red[w];
                store_row_loss(a.row_loss, row, tot, a.mt.counters != nullptr);
            }
        }
#ifdef SOT_STAMPS
        SOT_PH(sacc, 10);  // area, wave sum, barrier 5, store
        if (sacc != nullptr) sacc[0] += 1;
#endif
    }
#ifdef SOT_STAMPS
    if (sacc != nullptr) { for (int i = 0; i < 16; ++i) g_stamps[i] = sacc[i]; }
#endif
    if (a.mt.counters != nullptr) batch_mean_tail<ROWS * G>(a.mt, a.row_loss, a.B, reinterpret_cast<double*>(smem));
}

// ---------------------------------------------------------------------------------------------
// Merge-free p = 1 kernel for SHORT rows, TWO rows per wavefront (round 3).  A 257-bin row on 64 lanes x 5 elements leaves a fifth of
// the wave idle and pays every per-row fixed cost (scans, reductions, the mass fold, the store) for 257 points; here a row is
// owned by HALF a wave -- 32 lanes x CPT elements (9 for 257 bins, 5 for 129) -- so one instruction stream serves two rows.  The scans
// stop at the half-wave (the DPP row_bcast:31 step is left out), row state that the one-wave kernels keep in scalar registers is per
// lane, and ATen's 32 summation columns are exactly the 32 lanes: a column's sum comes from the registers the lane fetched (elements
// l, l + 32, ...), only the eight-way fold goes through LDS.  No workgroup barrier; arithmetic and its order per row are those of
// sot_area_full_kernel (the thread-local grouping of the sums differs: equal to ~1e-7, not bit for bit).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double half_incl_scan(double v)   // inclusive scan over each 32-lane half
{
    v += dpp_f64_shr<kRowShr1>(v);
    v += dpp_f64_shr<kRowShr2>(v);
    v += dpp_f64_shr<kRowShr4>(v);
    v += dpp_f64_shr<kRowShr8>(v);
    v += dpp_f64<kRowBcast15, 0xA>(v);
    return v;
}
__device__ __forceinline__ double half_shift_right1(double v, int l)   // lanes 0 and 32 get 0
{
    const double s = dpp_f64<kWaveShr1>(v);
    return l == 0 ? 0.0 : s;
}
__device__ __forceinline__ float half_sum(float v, int h)   // each half's total in all of its lanes
{
    v += dpp_f32<kRowShr1>(v);
    v += dpp_f32<kRowShr2>(v);
    v += dpp_f32<kRowShr4>(v);
    v += dpp_f32<kRowShr8>(v);
    v += dpp_f32<kRowBcast15, 0xA>(v);
    const float t0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
    const float t1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    return h ? t1 : t0;
}

// one half-wave row: element l + 32 k of the row at x / y
template <int CPT, int N>
__device__ __forceinline__ void half_fetch(const float* __restrict__ x, const float* __restrict__ y, int l, float (&rx)[CPT], float (&ry)[CPT])
{
    constexpr int NK = (N + 31) >> 5;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        rx[k] = 0.0f; ry[k] = 0.0f;
        if (k < NK) {
            const int e = l + 32 * k;
            if ((k + 1) * 32 <= N || e < N) { rx[k] = x[e]; ry[k] = y[e]; }
        }
    }
}

// staging (original column order) and ATen's column sums: column l = elements l, l + 32, ... in that order, straight from the registers
template <int CPT, bool SQ, int N>
__device__ __forceinline__ void half_stage(float* U, float* V, float* colbuf, int l, const float (&rx)[CPT], const float (&ry)[CPT])
{
    constexpr int NSTEPS = N >> 5, NK = (N + 31) >> 5;
    float ax = 0.0f, ay = 0.0f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int e = l + 32 * k;
        if ((k + 1) * 32 <= N || e < N) { U[e] = rx[k]; V[e] = ry[k]; }
        if (k < NSTEPS) { ax += SQ ? rx[k] * rx[k] : rx[k]; ay += SQ ? ry[k] * ry[k] : ry[k]; }
    }
    colbuf[l] = ax; colbuf[32 + l] = ay;
}

// row masses (the eight-way fold of ATen's columns + its scalar tail), the owned elements in sorted order, safe_divide and the
// fp64-accumulated CDFs of full_build_cdfs (P2 / P3) for a half-wave row: cu / cv = CDF values of the CPT owned elements
template <int CPT, bool SQ, int N>
__device__ __forceinline__ void half_cdfs(const FwdArgs& a, const float* U, const float* V, const float* colbuf, int l, bool dn, bool x_ident,
                                          bool y_ident, float (&cu)[CPT], float (&cv)[CPT])
{
    const int e0 = l * CPT;
    const float Sx = mass_fold_nx<SQ, N, false>(U, colbuf);
    const float Sy = dn ? Sx : mass_fold_nx<SQ, N, false>(V, colbuf + 32);
    float wx[CPT], wy[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const bool in = e0 + k < N;
        const int sx = in ? (x_ident ? e0 + k : a.xperm[e0 + k]) : 0;
        const int sy = in ? (y_ident ? e0 + k : a.yperm[e0 + k]) : 0;
        wx[k] = in ? U[sx] : 0.0f;
        wy[k] = in ? V[sy] : 0.0f;
    }
    const float Sxh = guard_mass(Sx), Syh = guard_mass(Sy);
    const float rSx = 1.0f / Sxh, rSy = 1.0f / Syh;
    double px[CPT], py[CPT];
    double runx = 0.0, runy = 0.0;
    {
        float qx[CPT], qy[CPT];
        uint32_t risk = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            qx[k] = div_by_row_constant(SQ ? wx[k] * wx[k] : wx[k], Sxh, rSx, risk);
            qy[k] = div_by_row_constant(SQ ? wy[k] * wy[k] : wy[k], Syh, rSy, risk);
        }
        const bool slow = (risk < kFastDivMinBits) || !(Sxh <= 0x1p40f) || !(Syh <= 0x1p40f);
        if (__builtin_amdgcn_ballot_w64(slow) != 0ull) {  // rare; exact either way, so the two rows of a wave may share the decision
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                qx[k] = (SQ ? wx[k] * wx[k] : wx[k]) / Sxh;
                qy[k] = (SQ ? wy[k] * wy[k] : wy[k]) / Syh;
            }
        }
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            runx += (double)qx[k]; runy += (double)qy[k];
            px[k] = runx; py[k] = runy;
        }
    }
    const double exx = half_shift_right1(half_incl_scan(runx), l), exy = half_shift_right1(half_incl_scan(runy), l);
#pragma unroll
    for (int k = 0; k < CPT; ++k) { cu[k] = (float)(exx + px[k]); cv[k] = (float)(exy + py[k]); }
}

template <int CPT, int ROWS, bool SQ, int N>
__global__ __launch_bounds__(ROWS * 32) void sot_area_half_kernel(const FwdArgs a)
{
    constexpr int CAP = 32 * CPT, NSTEPS = N >> 5, NK = (N + 31) >> 5;
    static_assert(ROWS % 2 == 0 && NK <= CPT && N <= CAP && NSTEPS >= 1 && NSTEPS < 16, "two half-wave rows per wave; one partial ATen chunk per column");
    static_assert((N >> 3) == NSTEPS * 4, "no left-over 8-lane vectors (N mod 32 < 8)");
    constexpr int ROWF = 2 * (CAP + 4) + 64 + 8;   // floats per row region: raw x, raw y, 2 x 32 column sums
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), l = lane & 31, h = lane >> 5, rs = tid >> 5;
    float* const U = smem + rs * ROWF;
    float* const V = U + CAP + 4;
    float* const colbuf = V + CAP + 4;
    const bool dn = a.flags & SOT_FLAG_DONT_NORMALIZE;
    bool x_ident = true, y_ident = true;
    if (a.ident != nullptr) { x_ident = a.ident[0] != 0; y_ident = a.ident[1] != 0; }
    const int64_t row_step = (int64_t)gridDim.x * ROWS;
    int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int e0 = l * CPT;
    float dx[CPT];   // widths of the grid cells behind the owned elements (sorted order); 0 behind the last point
    {
        float pe[CPT + 1];
#pragma unroll
        for (int k = 0; k <= CPT; ++k) pe[k] = a.xpos[min(e0 + k, N - 1)];
#pragma unroll
        for (int k = 0; k < CPT; ++k) dx[k] = (e0 + k + 1 < N) ? pe[k + 1] - pe[k] : 0.0f;
    }
    float rx[CPT], ry[CPT];
    if (row0 < a.B) { const int64_t r = min(row0 + rs, a.B - 1); half_fetch<CPT, N>(a.x + r * a.xs, a.y + r * a.ys, l, rx, ry); }

    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rs;
        const bool valid = row < a.B;
        half_stage<CPT, SQ, N>(U, V, colbuf, l, rx, ry);
        if (row0 + row_step < a.B) { const int64_t r = min(row0 + row_step + rs, a.B - 1); half_fetch<CPT, N>(a.x + r * a.xs, a.y + r * a.ys, l, rx, ry); }
        row_sync<1>();
        float cu[CPT], cv[CPT];
        half_cdfs<CPT, SQ, N>(a, U, V, colbuf, l, dn, x_ident, y_ident, cu, cv);
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < CPT; ++k) acc = fmaf(fabsf(cu[k] - cv[k]), dx[k], acc);
        acc = half_sum(acc, h);
        if (l == 0 && valid && a.row_loss) store_row_loss(a.row_loss, row, acc, a.mt.counters != nullptr);
        row_sync<1>();   // this row's LDS reads are done before the next row is staged
    }
    if (a.mt.counters != nullptr) batch_mean_tail<ROWS * 32>(a.mt, a.row_loss, a.B, reinterpret_cast<double*>(smem));
}

// The merge forward (sot_forward_full_kernel) in the same form: two rows per wave, each with its own copy of the positions behind its
// levels (the walk finds the position of the level at LDS address o at o + POFF4), 32 merge segments of E levels per row.
template <int CPT, int ROWS, int PM, bool LIM, bool SQ, int N>
struct HalfRowGeo {
    static constexpr int CAP = 32 * CPT, K = 2 * N, E = merge_steps(K, 32), GA = (K + E - 1) / E, PAD = GA * E - K;
    static constexpr int PADCAP = align4(E) + 4, NU = PADCAP + CAP + 4, NV = CAP + 4;
    static constexpr int POFF = NU + NV + 64;              // levels [pad | U | V], 2 x 32 column sums, then positions [pad | PX | PY]
    static constexpr int ROWF = POFF + NU + NV;
    static_assert(GA <= 32 && PAD + 1 <= PADCAP, "every lane walks at most one segment; room for the virtual predecessor");
};

template <int CPT, int ROWS, int PM, bool LIM, bool SQ, int N>
__global__ __launch_bounds__(ROWS * 32) void sot_forward_half_kernel(const FwdArgs a)
{
    using H = HalfRowGeo<CPT, ROWS, PM, LIM, SQ, N>;
    constexpr int CAP = H::CAP, NSTEPS = N >> 5, NK = (N + 31) >> 5, E = H::E, GA = H::GA, PAD = H::PAD;
    static_assert(ROWS % 2 == 0 && NK <= CPT && N <= CAP && NSTEPS >= 1 && NSTEPS < 16 && (N >> 3) == NSTEPS * 4, "see sot_area_half_kernel");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), l = lane & 31, h = lane >> 5, rs = tid >> 5;
    float* const base = smem + rs * H::ROWF;
    float* const U = base + H::PADCAP;
    float* const V = base + H::NU;
    float* const colbuf = base + H::NU + H::NV;
    float* const PX = U + H::POFF;
    float* const PY = V + H::POFF;
    const bool dn = a.flags & SOT_FLAG_DONT_NORMALIZE;
    bool x_ident = true, y_ident = true;
    if (a.ident != nullptr) { x_ident = a.ident[0] != 0; y_ident = a.ident[1] != 0; }
    // once: this row region's copy of the sorted positions, front padding, sentinels, virtual predecessors (full_setup)
    for (int e = l; e < N; e += 32) { PX[e] = a.xpos[e]; PY[e] = a.ypos[e]; }
    if (l < PAD) { PX[l - PAD] = a.xpos[0]; U[l - PAD] = 0.0f; }
    if (l == 0) {
        PX[N] = a.xpos[N - 1]; PY[N] = a.ypos[N - 1];      // clamp of losses.py:220
        U[N] = INFINITY; V[N] = INFINITY;                    // an exhausted side never wins the merge
        U[-PAD - 1] = -INFINITY; V[-1] = -INFINITY;          // never win the fmaxf that rebuilds Q_{k-1}
    }
    const int64_t row_step = (int64_t)gridDim.x * ROWS;
    int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int e0 = l * CPT;
    float rx[CPT], ry[CPT];
    if (row0 < a.B) { const int64_t r = min(row0 + rs, a.B - 1); half_fetch<CPT, N>(a.x + r * a.xs, a.y + r * a.ys, l, rx, ry); }
    row_sync<1>();

    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rs;
        const bool valid = row < a.B;
        half_stage<CPT, SQ, N>(U, V, colbuf, l, rx, ry);
        row_sync<1>();
        float cu[CPT], cv[CPT];
        half_cdfs<CPT, SQ, N>(a, U, V, colbuf, l, dn, x_ident, y_ident, cu, cv);
        row_sync<1>();   // every lane has read its raw weights: the levels may replace them
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            if (e0 + k < N) { U[e0 + k] = cu[k]; V[e0 + k] = cv[k]; }
        }
        if (row0 + row_step < a.B) { const int64_t r = min(row0 + row_step + rs, a.B - 1); half_fetch<CPT, N>(a.x + r * a.xs, a.y + r * a.ys, l, rx, ry); }
        row_sync<1>();
        float acc = 0.0f;
        if (GA == 32 || l < GA) {
            const int D0 = l * E;
            const uint32_t ub1 = lds_addr(U - PAD) - 4u;                  // address of Uw[-1]
            const uint32_t vd1 = lds_addr(V) + 4u * (uint32_t)D0 + ub1;   // address of V[D0], + ub1
            const uint32_t pb = merge_path_fixed32<N + PAD, N>(ub1, vd1, D0);
            acc = merge_walk_full<E, PM, LIM, 4u * (uint32_t)H::POFF>(pb + 4u, vd1 - pb, D0 == 0, a.p);
        }
        acc = half_sum(acc, h);
        if (l == 0 && valid && a.row_loss) store_row_loss(a.row_loss, row, acc, a.mt.counters != nullptr);
        row_sync<1>();   // this row's LDS reads are done before the next row is staged
    }
    if (a.mt.counters != nullptr) batch_mean_tail<ROWS * 32>(a.mt, a.row_loss, a.B, reinterpret_cast<double*>(smem));
}

template <int G, int CPT, int ROWS, bool SQ, int NX>
static hipError_t launch_area_full(const FwdArgs& a, hipStream_t s)
{
    auto kern = sot_area_full_kernel<G, CPT, ROWS, SQ, NX>;
    constexpr FullLayout L = full_layout<G, CPT, ROWS, false, NX>();
    const size_t lds = sizeof(float) * (size_t)ROWS * (size_t)L.rowf;
    constexpr int block = ROWS * G;
    static GridCache cache;
    const int grid_cap = cached_resident_grid(cache, kern, block, lds);
    const int64_t want = (a.B + ROWS - 1) / ROWS;
    const int grid = persistent_grid(want, grid_cap);
    (void)hipGetLastError();
    launch_maybe_profiled(kern, grid, block, lds, s, a);
    return hipGetLastError();
}

template <int G, int CPT, int ROWS, int NX = 0>
static hipError_t dispatch_area_full_g(const FwdArgs& a, hipStream_t s)
{
    return (a.flags & SOT_FLAG_SQUARE) ? launch_area_full<G, CPT, ROWS, true, NX>(a, s) : launch_area_full<G, CPT, ROWS, false, NX>(a, s);
}

template <int CPT, int ROWS, int N>
static hipError_t dispatch_area_half(const FwdArgs& a, hipStream_t s)
{
    constexpr size_t lds = sizeof(float) * (size_t)ROWS * (2 * (32 * CPT + 4) + 64 + 8);
    constexpr int block = ROWS * 32;
    const int64_t want = (a.B + ROWS - 1) / ROWS;
    (void)hipGetLastError();
    if (a.flags & SOT_FLAG_SQUARE) {
        auto kern = sot_area_half_kernel<CPT, ROWS, true, N>;
        static GridCache cache;
        launch_maybe_profiled(kern, persistent_grid(want, cached_resident_grid(cache, kern, block, lds)), block, lds, s, a);
    } else {
        auto kern = sot_area_half_kernel<CPT, ROWS, false, N>;
        static GridCache cache;
        launch_maybe_profiled(kern, persistent_grid(want, cached_resident_grid(cache, kern, block, lds)), block, lds, s, a);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Full-row backward kernel: sot_backward_kernel (closed form of the autograd graph, see there) for the same rows the
// full-row forward serves, sharing its CDF builder.  The gradient walk keeps the canonical stable order (U before V on
// ties): the gradient of a run of equal levels belongs to the run's last member.
// ---------------------------------------------------------------------------------------------
// 16-byte gradient store: plain (write-through or non-temporal forms measured no faster, profiles/r3_walk_experiments_ab.txt)
__device__ __forceinline__ void store_grad16(float* dst, float a, float b, float c, float d)
{
    *reinterpret_cast<float4*>(dst) = make_float4(a, b, c, d);
}

__device__ __forceinline__ void lds_store(uint32_t addr, float v)
{
    *reinterpret_cast<__attribute__((address_space(3))) float*>((uintptr_t)addr) = v;
}

// Gradient rows of the one-sided spectra (129 / 257 / 513 / 1025 / 2049 bins: rows of 4 N bytes, never a multiple of 16) leave the
// kernel through LDS (round 4).  Before: every thread stored its CPT contiguous gradients one dword at a time, i.e. CPT store
// instructions per wave at a lane stride of 4 CPT bytes, each touching every 128-B line of the wave's span partially.  The L2 answered
// the partial writes with line fills and partial write-backs: 16384 x 1025 training form FETCH 1.30 x / WRITE 1.13 x the algorithmic
// bytes (profiles/r3e_b16384n1025_cutoff_rocprofv3_summary.txt; VERDICT r3 weak #4).  Now a thread writes its gradients back into the
// row's own gradient slots in LDS -- shifted by `sh` = (float index of the row's first element in global memory) mod 4, so that LDS
// float index == global float index (mod 4) -- and the row group stores the row as 16-byte chunks on 16-byte boundaries of the GLOBAL
// address: one contiguous KiB per wave instruction, whole lines except the row's two ends (components outside the row are stored one
// dword at a time by the one or two lanes that own the ragged chunks).  The stores are issued at the top of the NEXT row iteration
// (after the barrier that closes this one): no extra barrier, and they overlap the next row's staging.
constexpr int kGradStagedMinBins = 1025;
template <int G, int N>
__device__ __forceinline__ void flush_row_grad(const float* lds_row, float* grow, int t)
{
    const int sh = (int)((reinterpret_cast<uintptr_t>(grow) >> 2) & 3u);   // wave-uniform
    float* const A = grow - sh;                                              // 16-byte aligned
    const int nch = (sh + N + 3) >> 2;
    const float4* const src = reinterpret_cast<const float4*>(lds_row);
    constexpr int NCH_MAX = (N + 3 + 3) >> 2;
#pragma unroll
    for (int i = 0; i < (NCH_MAX + G - 1) / G; ++i) {
        const int cidx = t + i * G;
        if (cidx < nch) {
            const float4 v = src[cidx];
            const int lo = 4 * cidx;
            if (lo >= sh && lo + 4 <= sh + N) {
                *reinterpret_cast<float4*>(A + lo) = v;
            } else {   // a ragged end of the row
                if (lo + 0 >= sh && lo + 0 < sh + N) A[lo + 0] = v.x;
                if (lo + 1 >= sh && lo + 1 < sh + N) A[lo + 1] = v.y;
                if (lo + 2 >= sh && lo + 2 < sh + N) A[lo + 2] = v.z;
                if (lo + 3 >= sh && lo + 3 < sh + N) A[lo + 3] = v.w;
            }
        }
    }
}

// WANT_X = false: only the gradient w.r.t. y is produced (b.gx == nullptr, the training step): the x side's reverse
// cumulative sum, scans, dot product and output arithmetic (fp64) are compiled out.  That variant also accumulates the
// row's LOSS during its walk (the forward kernel's arithmetic in the forward kernel's order: bit-identical) and stores it
// when f.row_loss is set, so that a training step needs this one kernel instead of forward + backward (sot_w1d_loss_and_grad).
// SLIM (y-only kernels): the row region has no gradient slots for U levels (FullLayout GRAD 2) and the walk masks their stores off.
// The masked store costs ~2 % (83.3 vs 81.5 us at 8192 x 2048, 90.6 vs 89.4 us at 16384 x 1025), so it is only used where the
// smaller region buys another resident row: 2048-bin rows, two per workgroup (79.7 us).
// MINB: second argument of __launch_bounds__ = waves per SIMD the kernel is compiled for (HIP's meaning; 4 -> at most 128 VGPRs, which
// for these 256-thread workgroups is four workgroups per CU), 1 = no constraint.
template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX = 0, bool WANT_X = true, bool SLIM = false, int MINB = 1, bool RP = false>
__global__ __launch_bounds__(ROWS * G, MINB) void sot_backward_full_kernel(const BwdArgs b)
{
    static_assert(!RP || (ROWS == 1 && NX == 0 && CPT == 8), "per-row positions (see sot_forward_full_kernel): one row per workgroup, rows that fill the 8-element geometry");
    static_assert(!(SLIM && WANT_X), "SLIM is a y-only layout");
    constexpr int GR = SLIM ? 2 : 1;
    using Geo = FullGeo<G, CPT, ROWS, GR, NX>;
    constexpr FullLayout L = Geo::L;
    constexpr int N = Geo::N, NW = Geo::NW, E = Geo::E, GA = Geo::GA, PAD = Geo::PAD;
    constexpr bool WITH_LOSS = !WANT_X;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FwdArgs& a = b.f;
    const int64_t row_step = (int64_t)gridDim.x * ROWS;
    int64_t row0 = (int64_t)blockIdx.x * ROWS;
    float rx[CPT], ry[CPT];
    FullCtx cm = full_setup<G, CPT, ROWS, GR, NX, RP>(a, smem);
    if constexpr (RP) { cm.x_ident = false; cm.y_ident = false; }
    const FullCtx c = cm;
    if constexpr (NW == 1) __syncthreads();   // shared position copy (see the forward kernel)
    const int rg = c.rg, t = c.t, lane = c.lane, wv = c.wv;
    float* const U = c.U; float* const V = c.V;
    const float* const Uw = c.Uw;
    const float* const GU = U + L.goff; const float* const GV = V + L.goff;   // SLIM: no GU region (never read: y only)
    double* const wtot = c.wtot;
    if (row0 < a.B) {
        const int64_t r = min(row0 + rg, a.B - 1);
        fetch_row<G, CPT, NX>(a.x + r * a.xs, a.y + r * a.ys, t, a.n, rx, ry);
    }

#ifdef SOT_STAMPS
    unsigned long long sbuf[16] = {};
    unsigned long long* const sacc = (threadIdx.x == 0 && blockIdx.x == gridDim.x / 2) ? sbuf : nullptr;
#else
    constexpr unsigned long long* sacc = nullptr;
#endif

    // gradient rows staged in LDS and stored one iteration later (flush_row_grad above): the compile-time odd lengths on identity permutations
    // Measured (round 4, interleaved A/B, training form unless noted; profiles/r4a_staged_gradient_stores.txt): 16384 x 1025 85.2 -> 79.3 us with
    // FETCH x 2 + WRITE 250.2 -> 204.3 MB (1.241 -> 1.014 x algorithmic), both-gradient backward 123.2 -> 103.0 us (1.010 x), 4096 x 1025
    // 28.8 -> 27.6 us, 4096 x 2049 52.5 -> 50.6 us; 8192 x 513 24.8 vs 24.9; one-wave rows lose (16384 x 257: 26.0 -> 26.6 us, traffic 1.023 x either
    // way; 32768 x 129: 33.1 -> 34.1 us): their CPT = 3 / 5 stores per thread already complete each line within a few instructions.
    constexpr bool STAGE_OUT = NX >= kGradStagedMinBins;
    const bool stage_x = STAGE_OUT && WANT_X && b.gx != nullptr && c.x_ident;
    const bool stage_y = STAGE_OUT && b.gy != nullptr && c.y_ident;
    int64_t pend_row = -1;   // wave-uniform: the row whose gradients wait in this row group's LDS slots
    (void)stage_x; (void)stage_y;

    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rg;
        const bool valid = row < a.B;
        const int64_t rowc = valid ? row : a.B - 1;
        const bool more = row0 + row_step < a.B;
        const int64_t rn = min(row0 + row_step + rg, a.B - 1);
        float wx[CPT], wy[CPT], cu[CPT], cv[CPT];
        float Sx, Sy;
#ifdef SOT_STAMPS
        if (sacc != nullptr) sacc[15] = __builtin_readcyclecounter();
#endif
        if constexpr (STAGE_OUT) {
            if (pend_row >= 0) {   // the previous row's gradients: its closing barrier has passed, the next write to these slots is this row's walk
                if constexpr (WANT_X) { if (stage_x) flush_row_grad<G, N>(GU, b.gx + pend_row * (int64_t)N, t); }
                if (stage_y) flush_row_grad<G, N>(GV, b.gy + pend_row * (int64_t)N, t);
            }
            pend_row = valid ? row : -1;
        }
        int ix[RP ? CPT : 1] = {}, iy[RP ? CPT : 1] = {}, psx[RP ? CPT : 1] = {}, psy[RP ? CPT : 1] = {};
        if constexpr (RP) rowpos_row_setup<G, CPT, ROWS, GR, NX>(a, c, rowc, ix, iy, psx, psy);
        full_build_cdfs<G, CPT, ROWS, GR, SQ, NX>(a, c, rx, ry, more ? a.x + rn * a.xs : nullptr,
                                                  more ? a.y + rn * a.ys : nullptr, wx, wy, Sx, Sy, cu, cv, sacc, RP ? psx : nullptr, RP ? psy : nullptr);
        SOT_PH(sacc, 9);   // wave totals, CDF values to LDS, next row's loads issued, barrier

        // ---- merge walk over (pad zero levels ++ U, V), exactly E steps per thread.  The gradient of a level is known one
        //      step later (it is non-zero only if the NEXT level starts a new run), so the store of element k-1 happens at
        //      step k; the thread's last element is closed by peeking at level D0+E.
        __builtin_amdgcn_s_setprio(kWalkPrio);
        float lacc = 0.0f, lq = 0.0f;   // WITH_LOSS: this thread's part of the row loss, the previous merged level
        if (GA == G || t < GA) {
            const uint32_t poff4 = 4u * (uint32_t)((ROWS - rg) * L.rowf);  // level -> its position (shared copy behind the rows)
            constexpr uint32_t GOFF4 = 4u * (uint32_t)L.goff;              // level -> its gradient slot
            bool slot = !SLIM;    // the element consumed last has a gradient slot (SLIM: V elements only; the other stores are masked off)
            const int D0 = t * E;
            const uint32_t uw32 = lds_addr(Uw);
            const uint32_t ub1 = uw32 - 4u;
            const uint32_t vd1 = lds_addr(V) + 4u * (uint32_t)D0 + ub1;
            const uint32_t pb = merge_path_fixed32<N + PAD, N>(ub1, vd1, D0);  // address of Uw[i0 - 1]
            const uint32_t ou = pb + 4u, ov = vd1 - pb;                        // addresses of Uw[i0], V[j0]
            float qprev = fmaxf(lds_load(pb), lds_load(ov - 4u));
            float ua = lds_load(ou), vb = lds_load(ov), xa = lds_load(ou + poff4), yb = lds_load(ov + poff4);
            float dcur = 0.0f;
            lq = (D0 == 0) ? 0.0f : qprev;           // loss: Q_0 := 0 (the pad of losses.py:301)
            if (D0 == 0) {
                qprev = __int_as_float(0x7fc00000);  // NaN: the very first level always starts a run
            } else if (fminf(ua, vb) == qprev) {      // we start inside a run: cost at its first member's ranks
                const float q0 = qprev;
                const float cst = transport_cost<PM>(c.PX[lower_rank(U, N, q0)], c.PY[lower_rank(V, N, q0)], a.p);
                dcur = (LIM && q0 > 1.0f) ? 0.0f : cst;
            }
            // (The forward kernel's loser form with the canonical tie order kept by a lane mask: no gain, profiles/r3_walk_experiments_ab.txt.)
            // LDS byte addresses of the next unread element of each stream, and of the element consumed last
            uint32_t pu = ou, pv = ov;
            uint32_t prev = uw32 + 4u * (uint32_t)(PAD + N);  // U[N]'s gradient slot: a scratch target for "no element yet"
#pragma unroll SOT_FULL_WALK_UNROLL
            for (int s2 = 0; s2 < E; ++s2) {
                const bool tu = ua <= vb;
                const float q = tu ? ua : vb;
                float cst = transport_cost<PM>(xa, yb, a.p);
                if constexpr (WITH_LOSS) {
                    float delta = q - lq;
                    if (LIM && q > 1.0f) delta = 0.0f;
                    lacc = fmaf(delta, cst, lacc);
                    lq = q;
                }
                if (LIM && q > 1.0f) cst = 0.0f;
                const bool new_run = !(q == qprev);
                if (!SLIM || slot) lds_store(prev + GOFF4, new_run ? (dcur - cst) : 0.0f);
                dcur = new_run ? cst : dcur;
                qprev = q;
                prev = tu ? pu : pv;             // slot of the element consumed now
                if constexpr (SLIM) slot = !tu;
                const uint32_t nx = prev + 4u;   // the consumed side's next element
                pu = tu ? nx : pu;
                pv = tu ? pv : nx;
                const float nv = lds_load(nx);
                const float np = lds_load(nx + poff4);
                ua = tu ? nv : ua;
                xa = tu ? np : xa;
                vb = tu ? vb : nv;
                yb = tu ? yb : np;
            }
            {   // close the last element with the level that follows this thread's range (0 cost past the end)
                const float qn = fminf(ua, vb);
                float cn = transport_cost<PM>(xa, yb, a.p);
                if ((LIM && qn > 1.0f) || (t == GA - 1)) cn = 0.0f;
                const bool new_run = !(qn == qprev) || (t == GA - 1);
                if (!SLIM || slot) lds_store(prev + GOFF4, new_run ? (dcur - cn) : 0.0f);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        SOT_PH(sacc, 10);  // partition search + gradient walk
        if constexpr (WITH_LOSS) {
            lacc = wave_sum(lacc);
            if (lane == 0) c.red[wv] = lacc;
        }
        row_sync<NW>();
        SOT_PH(sacc, 11);  // loss wave sum + barrier after the walk
        if constexpr (WITH_LOSS) {
            if (t == 0 && valid && a.row_loss) {
                float tot = c.red[0];
#pragma unroll
                for (int w = 1; w < NW; ++w) tot += c.red[w];
                store_row_loss(a.row_loss, row, tot, a.mt.counters != nullptr);
            }
        }

        // ---- reverse cumsums (fp64), normalisation terms, scatter to the original columns
        const int e0 = t * CPT;
        double ga[CPT], gb[CPT];
        double runx = 0.0, runy = 0.0;
        {
            float gu[CPT], gv[CPT];
            if constexpr (CPT % 4 == 0) {
#pragma unroll
                for (int k = 0; k + 3 < CPT; k += 4) {
                    float4 u4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if constexpr (WANT_X) u4 = *reinterpret_cast<const float4*>(GU + e0 + k);
                    const float4 v4 = *reinterpret_cast<const float4*>(GV + e0 + k);
                    gu[k] = u4.x; gu[k + 1] = u4.y; gu[k + 2] = u4.z; gu[k + 3] = u4.w;
                    gv[k] = v4.x; gv[k + 1] = v4.y; gv[k + 2] = v4.z; gv[k + 3] = v4.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < CPT; ++k) { gu[k] = WANT_X ? GU[e0 + k] : 0.0f; gv[k] = GV[e0 + k]; }
            }
            if (N < Geo::CAP && e0 + CPT > N) {  // slots at and past the end of the row hold no gradient (scratch / never written)
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    if (e0 + k >= N) { gu[k] = 0.0f; gv[k] = 0.0f; }
                }
            }
#pragma unroll
            for (int k = CPT - 1; k >= 0; --k) {
                if constexpr (WANT_X) runx += (double)gu[k];
                runy += (double)gv[k];
                ga[k] = runx;
                gb[k] = runy;
            }
        }
        // exclusive suffix over lanes = wave total - inclusive prefix (fp64: the cancellation is harmless)
        const double pinx = WANT_X ? wave_incl_scan(runx) : 0.0, piny = wave_incl_scan(runy);
        const double totwx = WANT_X ? wave_last(pinx) : 0.0, totwy = wave_last(piny);
        double exx = totwx - pinx, exy = totwy - piny;
        if (NW > 1) {
            if (lane == 0) { if constexpr (WANT_X) wtot[wv] = totwx; wtot[NW + wv] = totwy; }
            row_sync<NW>();
            double ox = 0.0, oy = 0.0;
            for (int w = NW - 1; w > wv; --w) { if constexpr (WANT_X) ox += wtot[w]; oy += wtot[NW + w]; }
            exx += ox;
            exy += oy;
        }
        SOT_PH(sacc, 12);  // gradient reads, fp64 reverse sums, wave scan, exchange across waves
        // dot products  sum ga_i * w_i  (w = staged weight, squared if square_dist).  In dont_normalize mode the y side's
        // mass term belongs to x's gradient: a y-only launch (the training step of the paper's configuration) needs neither
        // dot product, nor their wave sums, nor the two barriers of the exchange (kernel-uniform branch).
        const bool need_dots = WANT_X || !c.dn;
        double dotx = 0.0, doty = 0.0;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            gb[k] += exy;
            if constexpr (WANT_X) ga[k] += exx;
        }
        double totx = 0.0, toty = 0.0;
        if (need_dots) {
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const float sy = SQ ? wy[k] * wy[k] : wy[k];
                doty += gb[k] * (double)sy;
                if constexpr (WANT_X) {
                    const float sx = SQ ? wx[k] * wx[k] : wx[k];
                    dotx += ga[k] * (double)sx;
                }
            }
            if constexpr (WANT_X) dotx = wave_sum(dotx);
            doty = wave_sum(doty);
            totx = dotx; toty = doty;
            if (NW > 1) {
                row_sync<NW>();  // wtot is reused
                if (lane == 0) { if constexpr (WANT_X) wtot[wv] = dotx; wtot[NW + wv] = doty; }
                row_sync<NW>();
                totx = 0.0; toty = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) { if constexpr (WANT_X) totx += wtot[w]; toty += wtot[NW + w]; }
            }
        }
        const double dx = (double)guard_mass(Sx), dy = (double)guard_mass(Sy);
        const double rdx = 1.0 / dx, rdy = 1.0 / dy;
        double gSx = -totx, gSy = -toty;
        if (c.dn) { gSx += gSy; gSy = 0.0; }
        gSx = (Sx > kMassEps) ? gSx * rdx * rdx : 0.0;
        gSy = (Sy > kMassEps) ? gSy * rdy * rdy : 0.0;
        const double gr = (b.grad_row ? (double)b.grad_row[rowc * b.grad_row_stride] : 1.0) * (double)b.grad_scale;
        if (valid) {
            float ox[CPT], oy[CPT];
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                if constexpr (WANT_X) {
                    double g = ga[k] * rdx + gSx;
                    if (SQ) g *= 2.0 * (double)wx[k];
                    ox[k] = (float)(g * gr);
                }
                // (Collapsing this chain for the y-only dont_normalize case -- gSy == 0, so h = gb * (2 rdy gr wy): two fp64 products per
                // element instead of five operations -- was measured: 79.6 vs 79.6 us at 8192 x 2048, 86.7 vs 85.8 at 16384 x 1025.  Not kept.)
                double h = gb[k] * rdy + gSy;
                if (SQ) h *= 2.0 * (double)wy[k];
                oy[k] = (float)(h * gr);
            }
            const int nreal = Geo::RT ? a.n : N;
            if constexpr (STAGE_OUT) {   // into the row's own gradient slots (every read of them lies behind a barrier), shifted to the global alignment
                if constexpr (WANT_X) {
                    if (stage_x) {
                        float* const gs = const_cast<float*>(GU) + (int)((reinterpret_cast<uintptr_t>(b.gx + row * (int64_t)N) >> 2) & 3u);
#pragma unroll
                        for (int k = 0; k < CPT; ++k) { if (e0 + k < N) gs[e0 + k] = ox[k]; }
                    }
                }
                if (stage_y) {
                    float* const gs = const_cast<float*>(GV) + (int)((reinterpret_cast<uintptr_t>(b.gy + row * (int64_t)N) >> 2) & 3u);
#pragma unroll
                    for (int k = 0; k < CPT; ++k) { if (e0 + k < N) gs[e0 + k] = oy[k]; }
                }
            }
            if (WANT_X && b.gx && !stage_x) {
                float* dst = b.gx + row * (int64_t)nreal;
                if (Geo::ALIGNED && c.x_ident) {
#pragma unroll
                    for (int k = 0; k < CPT; k += 4)
                        store_grad16(dst + e0 + k, ox[k], ox[k + 1], ox[k + 2], ox[k + 3]);
                } else if (Geo::RT && c.x_ident) {   // run-time lengths: stores past the row are dropped by the buffer
                    const RowBuffer rb = row_buffer(dst, nreal);
#pragma unroll
                    for (int k = 0; k < CPT; ++k) row_buffer_store(rb, e0 + k, ox[k]);
                } else {
#pragma unroll
                    for (int k = 0; k < CPT; ++k) {
                        if ((N == Geo::CAP && !Geo::RT) || e0 + k < nreal) dst[c.x_ident ? e0 + k : (RP ? ix[RP ? k : 0] : a.xperm[e0 + k])] = ox[k];
                    }
                }
            }
            if (b.gy && !stage_y) {
                float* dst = b.gy + row * (int64_t)nreal;
                if (Geo::ALIGNED && c.y_ident) {
#pragma unroll
                    for (int k = 0; k < CPT; k += 4)
                        store_grad16(dst + e0 + k, oy[k], oy[k + 1], oy[k + 2], oy[k + 3]);
                } else if (Geo::RT && c.y_ident) {
                    const RowBuffer rb = row_buffer(dst, nreal);
#pragma unroll
                    for (int k = 0; k < CPT; ++k) row_buffer_store(rb, e0 + k, oy[k]);
                } else {
#pragma unroll
                    for (int k = 0; k < CPT; ++k) {
                        if ((N == Geo::CAP && !Geo::RT) || e0 + k < nreal) dst[c.y_ident ? e0 + k : (RP ? iy[RP ? k : 0] : a.yperm[e0 + k])] = oy[k];
                    }
                }
            }
        }
        SOT_PH(sacc, 13);  // dot products (if any), output arithmetic, stores issued
        row_sync<NW>();  // GU/GV/wtot reads done before the next row reuses LDS
        SOT_PH(sacc, 14);  // last barrier
#ifdef SOT_STAMPS
        if (sacc != nullptr) sacc[0] += 1;
#endif
    }
#ifdef SOT_STAMPS
    if (sacc != nullptr) { for (int i = 0; i < 16; ++i) g_stamps[i] = sacc[i]; }
#endif
    if constexpr (STAGE_OUT) {
        if (pend_row >= 0) {   // the last row's gradients
            if constexpr (WANT_X) { if (stage_x) flush_row_grad<G, N>(GU, b.gx + pend_row * (int64_t)N, t); }
            if (stage_y) flush_row_grad<G, N>(GV, b.gy + pend_row * (int64_t)N, t);
        }
    }
    if constexpr (WITH_LOSS) {
        if (a.mt.counters != nullptr) batch_mean_tail<ROWS * G>(a.mt, a.row_loss, a.B, reinterpret_cast<double*>(smem));
    }
}

// ---------------------------------------------------------------------------------------------
// Merge-free TRAINING FORM for p = 1 on one grid (round 4): row loss and d(grad_scale * sum_r row_loss) / dy out of
// sot_area_full_kernel's pipeline.  With loss = sum_{i < n-1} |U_i - V_i| (xs_{i+1} - xs_i) (see sot_area_full_kernel) and
// V_i = sum_{j <= i} b_j,  b_j = y_j^(2) / S:
//     d loss / d V_i = -sign(U_i - V_i) (xs_{i+1} - xs_i),      ga_j = sum_{i >= j} d loss / d V_i   (fp64 suffix sums),
//     d loss / d y_j = (ga_j / S + gS) * (2 y_j if square_dist),  gS = -sum_j ga_j b_j / S  (0 under dont_normalize: S is then x's mass)
// -- the closed form of sot_backward_kernel with the merge walk replaced by one compare per element.  Where the merge form is
// differentiable this is the same gradient (the same piecewise-linear function of the CDF values); at an exact tie U_i == V_i both
// give 0 (the merge form's run {U_i, V_i} meets cost 0 on either side on a common grid).  The CDF values never leave the registers
// of the thread that scanned them, nothing is merged and no gradient slot exists in LDS: staging, ATen-ordered masses, division,
// the fp64 scans, one compare and one suffix scan.  The row loss is sot_area_full_kernel's, operation for operation.
// ---------------------------------------------------------------------------------------------
// Register cap of the 9-element geometries (513 / 1025 / 2049 bins): uncapped they take 146 VGPRs = three waves per SIMD; four 256-thread
// workgroups per CU (128 VGPRs) measured (training form, p = 1, interleaved A/B): 16384 x 1025 72.6 -> 66.0 us, 4096 x 1025 23.4 -> 22.1 us,
// 4096 x 2049 42.1 -> 37.1 us (the merge backward: 77 / 27 / 45 us).  Skipping the gradient stores altogether changes nothing (73.1 vs
// 73.1 us): the kernel is bound by occupancy and issue, not by its unaligned dword stores.
constexpr int kAreaTrainMinWaves = 4;
template <int G, int CPT, int ROWS, bool SQ, int NX = 0>
__global__ __launch_bounds__(ROWS * G, (NX > 0 && CPT >= 9) ? kAreaTrainMinWaves : 1) void sot_area_train_kernel(const BwdArgs b)
{
    using Geo = FullGeo<G, CPT, ROWS, false, NX>;
    constexpr FullLayout L = Geo::L;
    constexpr int N = Geo::N, NW = Geo::NW;
    static_assert(!Geo::RT, "compile-time row lengths");
    extern __shared__ __attribute__((aligned(16))) float smem[];   // ROWS row regions, then 2 NW doubles per row (the exchanges across waves)
    const FwdArgs& a = b.f;
    const int64_t row_step = (int64_t)gridDim.x * ROWS;
    int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int tid = threadIdx.x;
    FullCtx c;
    c.rg = __builtin_amdgcn_readfirstlane(tid / G);
    c.t = tid - c.rg * G;
    c.lane = tid & (kWave - 1);
    c.wv = __builtin_amdgcn_readfirstlane(c.t >> 6);
    const int rg = c.rg, t = c.t, lane = c.lane, wv = c.wv;
    float rx[CPT], ry[CPT];
    if (row0 < a.B) {
        const int64_t r = min(row0 + rg, a.B - 1);
        fetch_row<G, CPT, NX>(a.x + r * a.xs, a.y + r * a.ys, t, a.n, rx, ry);
    }
    c.dn = a.flags & SOT_FLAG_DONT_NORMALIZE;
    float* const base = smem + rg * L.rowf;
    c.U = base + L.padcap; c.V = base + L.nU; c.part = base + L.part; c.colbuf = base + L.colbuf;
    c.wtot = reinterpret_cast<double*>(base + L.wtot);
    c.red = base + L.red; c.Sv = c.red + NW;
    c.Uw = c.U; c.PX = nullptr; c.PY = nullptr;
    c.x_ident = true; c.y_ident = true;
    if (a.ident != nullptr) { c.x_ident = a.ident[0] != 0; c.y_ident = a.ident[1] != 0; }
    double* const xw = reinterpret_cast<double*>(smem + ROWS * L.rowf) + rg * (2 * NW);   // [NW] suffix totals, [NW] dot products
    const int e0 = t * CPT;
    float dx[CPT];   // widths of the grid cells behind the CPT elements this thread owns (sorted order); 0 behind the last point
    {
        float pe[CPT + 1];
#pragma unroll
        for (int k = 0; k <= CPT; ++k) pe[k] = a.xpos[min(e0 + k, N - 1)];
#pragma unroll
        for (int k = 0; k < CPT; ++k) dx[k] = (e0 + k + 1 < N) ? pe[k + 1] - pe[k] : 0.0f;
    }
    float* const red = c.red;
    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rg;
        const bool valid = row < a.B;
        const int64_t rowc = valid ? row : a.B - 1;
        const bool more = row0 + row_step < a.B;
        const int64_t rn = min(row0 + row_step + rg, a.B - 1);
        float wx[CPT], wy[CPT], cu[CPT], cv[CPT];
        float Sx, Sy;
        full_build_cdfs<G, CPT, ROWS, false, SQ, NX, false, true>(a, c, rx, ry, more ? a.x + rn * a.xs : nullptr,
                                                            more ? a.y + rn * a.ys : nullptr, wx, wy, Sx, Sy, cu, cv);
        float acc = 0.0f;
        double gb[CPT];      // the thread's own suffix sums (as floats they save no register: the peak is inside full_build_cdfs)
        double runy = 0.0;
#pragma unroll
        for (int k = 0; k < CPT; ++k) acc = fmaf(fabsf(cu[k] - cv[k]), dx[k], acc);   // the loss: sot_area_full_kernel's chain
#pragma unroll
        for (int k = CPT - 1; k >= 0; --k) {
            const float d = cu[k] - cv[k];
            const float gvk = d > 0.0f ? -dx[k] : (d < 0.0f ? dx[k] : 0.0f);            // d loss / d V_k
            runy += (double)gvk;
            gb[k] = runy;
        }
        acc = wave_sum(acc);
        const double piny = wave_incl_scan(runy);
        const double totwy = wave_last(piny);
        double exy = totwy - piny;   // exclusive suffix over the lanes behind this one
        if (NW == 1) {
            if (lane == 0 && valid && a.row_loss) store_row_loss(a.row_loss, row, acc, a.mt.counters != nullptr);
        } else {
            if (lane == 0) { red[wv] = acc; xw[wv] = totwy; }
            row_sync<NW>();
            if (t == 0 && valid && a.row_loss) {
                float tot = red[0];
#pragma unroll
                for (int w = 1; w < NW; ++w) tot += red[w];
                store_row_loss(a.row_loss, row, tot, a.mt.counters != nullptr);
            }
            double oy = 0.0;
            for (int w = NW - 1; w > wv; --w) oy += xw[w];
            exy += oy;
        }
        double toty = 0.0;
        if (!c.dn) {   // the mass term of y's own normalisation (under dont_normalize y is divided by x's mass: no term)
            double doty = 0.0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const float sy = SQ ? wy[k] * wy[k] : wy[k];
                doty += (gb[k] + exy) * (double)sy;
            }
            doty = wave_sum(doty);
            toty = doty;
            if (NW > 1) {
                if (lane == 0) xw[NW + wv] = doty;
                row_sync<NW>();
                toty = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) toty += xw[NW + w];
            }
        }
        const double dy = (double)guard_mass(Sy);
        const double rdy = 1.0 / dy;
        double gSy = c.dn ? 0.0 : -toty;
        gSy = (Sy > kMassEps) ? gSy * rdy * rdy : 0.0;
        const double gr = (b.grad_row ? (double)b.grad_row[rowc * b.grad_row_stride] : 1.0) * (double)b.grad_scale;
        if (valid) {
            float oy[CPT];
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                double h = (gb[k] + exy) * rdy + gSy;
                if (SQ) h *= 2.0 * (double)wy[k];
                oy[k] = (float)(h * gr);
            }
            float* dst = b.gy + row * (int64_t)N;
            if (Geo::ALIGNED && c.y_ident) {
#pragma unroll
                for (int k = 0; k < CPT; k += 4) store_grad16(dst + e0 + k, oy[k], oy[k + 1], oy[k + 2], oy[k + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    if (N == Geo::CAP || e0 + k < N) dst[c.y_ident ? e0 + k : a.yperm[e0 + k]] = oy[k];
                }
            }
        }
        if (NW == 1) row_sync<NW>();   // (several waves: the exchanges above are this row's barriers; the next row's writes to red / xw lie behind its own)
    }
    if (a.mt.counters != nullptr) batch_mean_tail<ROWS * G>(a.mt, a.row_loss, a.B, reinterpret_cast<double*>(smem));
}

template <int G, int CPT, int ROWS, bool SQ, int NX>
static hipError_t launch_area_train(const BwdArgs& b, hipStream_t s)
{
    auto kern = sot_area_train_kernel<G, CPT, ROWS, SQ, NX>;
    constexpr FullLayout L = full_layout<G, CPT, ROWS, false, NX>();
    const size_t lds = sizeof(float) * (size_t)ROWS * (size_t)L.rowf + sizeof(double) * (size_t)ROWS * 2 * (G / kWave);
    constexpr int block = ROWS * G;
    static GridCache cache;
    const int grid_cap = cached_resident_grid(cache, kern, block, lds);
    const int64_t want = (b.f.B + ROWS - 1) / ROWS;
    const int grid = persistent_grid(want, grid_cap);
    (void)hipGetLastError();
    launch_maybe_profiled(kern, grid, block, lds, s, b);
    return hipGetLastError();
}

template <int G, int CPT, int ROWS, int NX = 0>
static hipError_t dispatch_area_train_g(const BwdArgs& b, hipStream_t s)
{
    return (b.f.flags & SOT_FLAG_SQUARE) ? launch_area_train<G, CPT, ROWS, true, NX>(b, s) : launch_area_train<G, CPT, ROWS, false, NX>(b, s);
}

template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX, bool RP = false>
static hipError_t launch_forward_full(const FwdArgs& a, hipStream_t s)
{
    auto kern = sot_forward_full_kernel<G, CPT, ROWS, PM, LIM, SQ, NX, RP>;
    constexpr FullLayout L = full_layout<G, CPT, ROWS, false, NX>();
    const size_t lds = sizeof(float) * (size_t)L.total;
    constexpr int block = ROWS * G;
    static GridCache cache;  // per instantiation, per device (sot_launch.hpp: cached_resident_grid)
    const int grid_cap = cached_resident_grid(cache, kern, block, lds);
    const int64_t want = (a.B + ROWS - 1) / ROWS;
    const int grid = persistent_grid(want, grid_cap);
    (void)hipGetLastError();
    launch_maybe_profiled(kern, grid, block, lds, s, a);
    return hipGetLastError();
}

template <int G, int CPT, int ROWS, int NX = 0>
static hipError_t dispatch_forward_full_g(int pm, const FwdArgs& a, hipStream_t s)
{
    static_assert(sizeof(float) * (size_t)full_layout<G, CPT, ROWS, false, NX>().total <= kLdsLimit, "workgroup fits one CU's LDS");
    const bool lim = a.flags & SOT_FLAG_LIMIT_Q;
    const bool sq = a.flags & SOT_FLAG_SQUARE;
    // pm: 1 -> p == 1, 2 -> p == 2, 0 -> any other p >= 1 (powf in the walk; losses.py:313 takes any p at one speed, and so does
    // the compile-time-length kernel: round 2 sent such calls to the generic kernel, 4x slower at 8192 x 2048)
    const int sel = (pm == 2 ? 4 : pm == 0 ? 8 : 0) | (lim ? 2 : 0) | (sq ? 1 : 0);
    switch (sel) {
        case 0: return launch_forward_full<G, CPT, ROWS, 1, false, false, NX>(a, s);
        case 1: return launch_forward_full<G, CPT, ROWS, 1, false, true, NX>(a, s);
        case 2: return launch_forward_full<G, CPT, ROWS, 1, true, false, NX>(a, s);
        case 3: return launch_forward_full<G, CPT, ROWS, 1, true, true, NX>(a, s);
        case 4: return launch_forward_full<G, CPT, ROWS, 2, false, false, NX>(a, s);
        case 5: return launch_forward_full<G, CPT, ROWS, 2, false, true, NX>(a, s);
        case 6: return launch_forward_full<G, CPT, ROWS, 2, true, false, NX>(a, s);
        case 7: return launch_forward_full<G, CPT, ROWS, 2, true, true, NX>(a, s);
        case 8: return launch_forward_full<G, CPT, ROWS, 0, false, false, NX>(a, s);
        case 9: return launch_forward_full<G, CPT, ROWS, 0, false, true, NX>(a, s);
        case 10: return launch_forward_full<G, CPT, ROWS, 0, true, false, NX>(a, s);
        default: return launch_forward_full<G, CPT, ROWS, 0, true, true, NX>(a, s);
    }
}

// Per-row positions with handed-over permutations on the compile-time geometries of 2048- / 1024- / 512-point rows, ONE row per workgroup (round 6).
// Preconditions (run_forward): n == m in {512, 1024, 2048}, rows and permutation rows 16-byte aligned, a.perm_in complete, SOT_FLAG_REQUIRE_SORT.
template <int G>
static hipError_t dispatch_forward_full_rowpos_g(int pm, const FwdArgs& a, hipStream_t s)
{
    const bool lim = a.flags & SOT_FLAG_LIMIT_Q;
    const bool sq = a.flags & SOT_FLAG_SQUARE;
    const int sel = (pm == 2 ? 4 : pm == 0 ? 8 : 0) | (lim ? 2 : 0) | (sq ? 1 : 0);
    switch (sel) {
        case 0: return launch_forward_full<G, 8, 1, 1, false, false, 0, true>(a, s);
        case 1: return launch_forward_full<G, 8, 1, 1, false, true, 0, true>(a, s);
        case 2: return launch_forward_full<G, 8, 1, 1, true, false, 0, true>(a, s);
        case 3: return launch_forward_full<G, 8, 1, 1, true, true, 0, true>(a, s);
        case 4: return launch_forward_full<G, 8, 1, 2, false, false, 0, true>(a, s);
        case 5: return launch_forward_full<G, 8, 1, 2, false, true, 0, true>(a, s);
        case 6: return launch_forward_full<G, 8, 1, 2, true, false, 0, true>(a, s);
        case 7: return launch_forward_full<G, 8, 1, 2, true, true, 0, true>(a, s);
        case 8: return launch_forward_full<G, 8, 1, 0, false, false, 0, true>(a, s);
        case 9: return launch_forward_full<G, 8, 1, 0, false, true, 0, true>(a, s);
        case 10: return launch_forward_full<G, 8, 1, 0, true, false, 0, true>(a, s);
        default: return launch_forward_full<G, 8, 1, 0, true, true, 0, true>(a, s);
    }
}

template <int CPT, int ROWS, int PM, bool LIM, bool SQ, int N>
static hipError_t launch_forward_half(const FwdArgs& a, hipStream_t s)
{
    auto kern = sot_forward_half_kernel<CPT, ROWS, PM, LIM, SQ, N>;
    constexpr size_t lds = sizeof(float) * (size_t)ROWS * HalfRowGeo<CPT, ROWS, PM, LIM, SQ, N>::ROWF;
    constexpr int block = ROWS * 32;
    static GridCache cache;
    const int64_t want = (a.B + ROWS - 1) / ROWS;
    (void)hipGetLastError();
    launch_maybe_profiled(kern, persistent_grid(want, cached_resident_grid(cache, kern, block, lds)), block, lds, s, a);
    return hipGetLastError();
}

template <int CPT, int ROWS, int N>
static hipError_t dispatch_forward_half(int pm, const FwdArgs& a, hipStream_t s)
{
    const bool lim = a.flags & SOT_FLAG_LIMIT_Q;
    const bool sq = a.flags & SOT_FLAG_SQUARE;
    const int sel = (pm == 2 ? 4 : pm == 0 ? 8 : 0) | (lim ? 2 : 0) | (sq ? 1 : 0);
    switch (sel) {
        case 0: return launch_forward_half<CPT, ROWS, 1, false, false, N>(a, s);
        case 1: return launch_forward_half<CPT, ROWS, 1, false, true, N>(a, s);
        case 2: return launch_forward_half<CPT, ROWS, 1, true, false, N>(a, s);
        case 3: return launch_forward_half<CPT, ROWS, 1, true, true, N>(a, s);
        case 4: return launch_forward_half<CPT, ROWS, 2, false, false, N>(a, s);
        case 5: return launch_forward_half<CPT, ROWS, 2, false, true, N>(a, s);
        case 6: return launch_forward_half<CPT, ROWS, 2, true, false, N>(a, s);
        case 7: return launch_forward_half<CPT, ROWS, 2, true, true, N>(a, s);
        case 8: return launch_forward_half<CPT, ROWS, 0, false, false, N>(a, s);
        case 9: return launch_forward_half<CPT, ROWS, 0, false, true, N>(a, s);
        case 10: return launch_forward_half<CPT, ROWS, 0, true, false, N>(a, s);
        default: return launch_forward_half<CPT, ROWS, 0, true, true, N>(a, s);
    }
}

template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX, bool WANT_X, bool SLIM = false, int MINB = 1, bool RP = false>
static hipError_t launch_backward_full_x(const BwdArgs& b, hipStream_t s)
{
    auto kern = sot_backward_full_kernel<G, CPT, ROWS, PM, LIM, SQ, NX, WANT_X, SLIM, MINB, RP>;
    constexpr FullLayout L = full_layout<G, CPT, ROWS, SLIM ? 2 : 1, NX>();
    const size_t lds = sizeof(float) * (size_t)L.total;
    constexpr int block = ROWS * G;
    static GridCache cache;  // per instantiation, per device (sot_launch.hpp: cached_resident_grid)
    const int grid_cap = cached_resident_grid(cache, kern, block, lds);
    const int64_t want = (b.f.B + ROWS - 1) / ROWS;
    const int grid = persistent_grid(want, grid_cap);
    (void)hipGetLastError();
    launch_maybe_profiled(kern, grid, block, lds, s, b);
    return hipGetLastError();
}

// WHICH: bit 0 = the both-gradient kernels, bit 1 = the y-only kernels of this layout (a geometry whose y-only calls go to
// dispatch_backward_full_y instantiates only the former)
template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX, int WHICH = 3>
static hipError_t launch_backward_full(const BwdArgs& b, hipStream_t s)
{
    // in dont_normalize mode the y side's mass term lands in the x side's gradient, which needs gx anyway
    if constexpr (WHICH & 1) { if (b.gx != nullptr) return launch_backward_full_x<G, CPT, ROWS, PM, LIM, SQ, NX, true>(b, s); }
    if constexpr (WHICH & 2) { if (b.gx == nullptr) return launch_backward_full_x<G, CPT, ROWS, PM, LIM, SQ, NX, false>(b, s); }
    return hipErrorInvalidConfiguration;
}

template <int G, int CPT, int ROWS, int NX = 0, int WHICH = 3>
static hipError_t dispatch_backward_full_g(int pm, const BwdArgs& b, hipStream_t s)
{
    static_assert(sizeof(float) * (size_t)full_layout<G, CPT, ROWS, true, NX>().total <= kLdsLimit, "workgroup fits one CU's LDS");
    const bool lim = b.f.flags & SOT_FLAG_LIMIT_Q;
    const bool sq = b.f.flags & SOT_FLAG_SQUARE;
    const int sel = (pm == 2 ? 4 : pm == 0 ? 8 : 0) | (lim ? 2 : 0) | (sq ? 1 : 0);
    switch (sel) {
        case 0: return launch_backward_full<G, CPT, ROWS, 1, false, false, NX, WHICH>(b, s);
        case 1: return launch_backward_full<G, CPT, ROWS, 1, false, true, NX, WHICH>(b, s);
        case 2: return launch_backward_full<G, CPT, ROWS, 1, true, false, NX, WHICH>(b, s);
        case 3: return launch_backward_full<G, CPT, ROWS, 1, true, true, NX, WHICH>(b, s);
        case 4: return launch_backward_full<G, CPT, ROWS, 2, false, false, NX, WHICH>(b, s);
        case 5: return launch_backward_full<G, CPT, ROWS, 2, false, true, NX, WHICH>(b, s);
        case 6: return launch_backward_full<G, CPT, ROWS, 2, true, false, NX, WHICH>(b, s);
        case 7: return launch_backward_full<G, CPT, ROWS, 2, true, true, NX, WHICH>(b, s);
        case 8: return launch_backward_full<G, CPT, ROWS, 0, false, false, NX, WHICH>(b, s);
        case 9: return launch_backward_full<G, CPT, ROWS, 0, false, true, NX, WHICH>(b, s);
        case 10: return launch_backward_full<G, CPT, ROWS, 0, true, false, NX, WHICH>(b, s);
        default: return launch_backward_full<G, CPT, ROWS, 0, true, true, NX, WHICH>(b, s);
    }
}

// the y-only kernels of one geometry alone (gx == nullptr)
template <int G, int CPT, int ROWS, int NX = 0, bool SLIM = true, int MINB = 1>
static hipError_t dispatch_backward_full_y(int pm, const BwdArgs& b, hipStream_t s)
{
    static_assert(sizeof(float) * (size_t)full_layout<G, CPT, ROWS, SLIM ? 2 : 1, NX>().total <= kLdsLimit, "workgroup fits one CU's LDS");
    const bool lim = b.f.flags & SOT_FLAG_LIMIT_Q;
    const bool sq = b.f.flags & SOT_FLAG_SQUARE;
    const int sel = (pm == 2 ? 4 : pm == 0 ? 8 : 0) | (lim ? 2 : 0) | (sq ? 1 : 0);
    switch (sel) {
        case 0: return launch_backward_full_x<G, CPT, ROWS, 1, false, false, NX, false, SLIM, MINB>(b, s);
        case 1: return launch_backward_full_x<G, CPT, ROWS, 1, false, true, NX, false, SLIM, MINB>(b, s);
        case 2: return launch_backward_full_x<G, CPT, ROWS, 1, true, false, NX, false, SLIM, MINB>(b, s);
        case 3: return launch_backward_full_x<G, CPT, ROWS, 1, true, true, NX, false, SLIM, MINB>(b, s);
        case 4: return launch_backward_full_x<G, CPT, ROWS, 2, false, false, NX, false, SLIM, MINB>(b, s);
        case 5: return launch_backward_full_x<G, CPT, ROWS, 2, false, true, NX, false, SLIM, MINB>(b, s);
        case 6: return launch_backward_full_x<G, CPT, ROWS, 2, true, false, NX, false, SLIM, MINB>(b, s);
        case 7: return launch_backward_full_x<G, CPT, ROWS, 2, true, true, NX, false, SLIM, MINB>(b, s);
        case 8: return launch_backward_full_x<G, CPT, ROWS, 0, false, false, NX, false, SLIM, MINB>(b, s);
        case 9: return launch_backward_full_x<G, CPT, ROWS, 0, false, true, NX, false, SLIM, MINB>(b, s);
        case 10: return launch_backward_full_x<G, CPT, ROWS, 0, true, false, NX, false, SLIM, MINB>(b, s);
        default: return launch_backward_full_x<G, CPT, ROWS, 0, true, true, NX, false, SLIM, MINB>(b, s);
    }
}

// Per-row positions with handed-over permutations on the 2048-point geometry (round 6; see sot_forward_full_kernel: RP).  One row per workgroup;
// gradient w.r.t. y alone: the layout without U gradient slots, and the row loss on the walk (the training form).  Gradients leave through the permutation
// (scattered 4-byte stores inside the row's 8 KB).
template <int G, int PM, bool LIM, bool SQ>
static hipError_t launch_backward_full_rowpos(const BwdArgs& b, hipStream_t s)
{
    if (b.gx != nullptr) return launch_backward_full_x<G, 8, 1, PM, LIM, SQ, 0, true, false, 1, true>(b, s);
    return launch_backward_full_x<G, 8, 1, PM, LIM, SQ, 0, false, true, 1, true>(b, s);
}
template <int G>
static hipError_t dispatch_backward_full_rowpos_g(int pm, const BwdArgs& b, hipStream_t s)
{
    const bool lim = b.f.flags & SOT_FLAG_LIMIT_Q;
    const bool sq = b.f.flags & SOT_FLAG_SQUARE;
    const int sel = (pm == 2 ? 4 : pm == 0 ? 8 : 0) | (lim ? 2 : 0) | (sq ? 1 : 0);
    switch (sel) {
        case 0: return launch_backward_full_rowpos<G, 1, false, false>(b, s);
        case 1: return launch_backward_full_rowpos<G, 1, false, true>(b, s);
        case 2: return launch_backward_full_rowpos<G, 1, true, false>(b, s);
        case 3: return launch_backward_full_rowpos<G, 1, true, true>(b, s);
        case 4: return launch_backward_full_rowpos<G, 2, false, false>(b, s);
        case 5: return launch_backward_full_rowpos<G, 2, false, true>(b, s);
        case 6: return launch_backward_full_rowpos<G, 2, true, false>(b, s);
        case 7: return launch_backward_full_rowpos<G, 2, true, true>(b, s);
        case 8: return launch_backward_full_rowpos<G, 0, false, false>(b, s);
        case 9: return launch_backward_full_rowpos<G, 0, false, true>(b, s);
        case 10: return launch_backward_full_rowpos<G, 0, true, false>(b, s);
        default: return launch_backward_full_rowpos<G, 0, true, true>(b, s);
    }
}

}  // namespace sot
