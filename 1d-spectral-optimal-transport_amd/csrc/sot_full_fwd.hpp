// sot_full_fwd.hpp -- forward kernels of the full-row family (compile-time geometries) with their launch and dispatch templates,
// namespace sot: the merge forward, the merge-free p = 1 forward (area) and their two-rows-per-wave forms.  Included by the objects
// that instantiate them: sot_full_fwd.hip (compile-time row lengths), sot_full_rt_fwd.hip (run-time row lengths) and sot_bf16.hip (16-bit
// rows).  The non-template dispatch functions live in the first two (dispatch_forward_full, dispatch_area_full, ...); the geometry tables
// of 512 ... 4096 bins, which the float32 and the 16-bit rows share, are templates over the element type here (dispatch_*_full_pow2).
// The backward side is sot_full_bwd.hpp.
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
#include "sot_full_common.hpp"

namespace sot {

// the one-wave-per-row forward kernels of 1025-bin rows (17 elements per thread): 152 / 154 VGPRs = three waves per SIMD; held to four
// (128 VGPRs, spills): 16384 x 1025 paper mode 41.5 -> 77.4 us, p = 1 28.8 -> 47.0 us -- left alone
constexpr int kFwd17MinWaves = 1;

constexpr int kFwd1025OneWaveRows = 6144;   // batches of at least this many 1025-bin rows: one wave per row in the forward kernel
constexpr int kRt1024OneWaveRows = 8192;    // the same for run-time lengths on the 1024-point geometry (16 elements per thread)

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

// RP (round 6): PER-ROW positions whose sort permutations are handed in (a.perm_in: [B, 2 N] uint16, written by sot_rowpos_sort_kernel or an earlier
// forward): every row brings its own positions -- loaded coalesced, staged in the U / V regions, gathered through the permutation into the
// position copy behind the row region -- and its weights are read through the same permutation (the psx / psy path of a permuted shared grid).
// One row per workgroup only (the position copy is the row's own), rows that fill their geometry (NX == 0).
// WT (sot_full_common.hpp: fetch_row): the element type of the weight rows in memory -- float, or uint16_t for bfloat16 rows (a.x / a.y then
// point at 16-bit elements, a.xs / a.ys count them; NX == 0 on shared positions only).  Only the two fetches see it.
template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX = 0, bool RP = false, class WT = float>
__global__ __launch_bounds__(ROWS * G, (G == 512 && NX < 0) ? kRt512MinWaves : (CPT == 17) ? kFwd17MinWaves : kFwdMinWaves) void sot_forward_full_kernel(const FwdArgs a)
{
    static_assert(std::is_same<WT, float>::value || (NX == 0 && !RP), "16-bit rows: rows that fill their geometry, shared positions");
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
        fetch_row<G, CPT, NX, WT>(weight_row<WT>(a.x, r, a.xs), weight_row<WT>(a.y, r, a.ys), t, a.n, rx, ry);
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
        full_build_cdfs<G, CPT, ROWS, false, SQ, NX, true, false, false, NoRowHook, WT>(
            a, c, rx, ry, more ? weight_row<WT>(a.x, rn, a.xs) : nullptr, more ? weight_row<WT>(a.y, rn, a.ys) : nullptr, wx, wy, Sx, Sy, cu, cv, sacc,
            HOIST_PERM ? psx : nullptr, HOIST_PERM ? psy : nullptr);
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

// The row loop of sot_area_full_kernel for the launch every reference call site makes: both permutations the identity, normalised rows,
// row losses wanted, no mean tail -- tested once per launch by the kernel, compile-time constants here (full_build_cdfs: PLAIN), so the
// loop holds neither the branches on them, nor the gathers through a.xperm / a.yperm, nor the write-through store.  Same arithmetic in
// the same order as the general body: the row losses are bit-identical (tests/test_area_fast_loop_gpu.py).
// Rows of several waves (NW > 1) run on THREE workgroup barriers instead of four: the wave sums of row k wait in red[] until the row
// group's last wave -- which has no part in the mass fold, the critical path between barriers 1 and 3 -- adds them up (red[0] + red[1] +
// ..., the order of the general body) and stores the loss behind barrier 1 of row k + 1; the workgroup's last row pays one barrier of
// its own behind the loop.  LDS hazards of one row group, row k against row k + 1 (b1 ... b4: the barriers of full_build_cdfs):
//   region        written                                      read                                       reuse ordered by
//   U / V (raw)   staging of row k, before b1(k)               fold tail + owner reads, b1(k) .. b3(k)    b3(k), b4(k): row k + 1 is staged behind them
//   part          staging of row k, before b1(k)               columns (waves 0, 1), b1(k) .. b3(k)       b3(k), b4(k)
//   colbuf        waves 0 / 1, b1(k) .. b3(k)                  the writing wave itself (wave fence)       program order of one wave
//   Sv            lane 0 of waves 0 / 1, b1(k) .. b3(k)        everyone, b3(k) .. b4(k)                   b4(k), b1(k + 1): rewritten behind b1(k + 1)
//   wtot          last lane of each wave, b3(k) .. b4(k)       everyone, behind b4(k)                     b1(k + 1), b3(k + 1): rewritten behind b3(k + 1)
//   red           lane 0 of each wave, behind b4(k)            the last wave's lane 0, behind b1(k + 1)   b3(k + 1), b4(k + 1): rewritten behind b4(k + 1)
// Every reuse has a barrier of the next row in between: nothing is double-buffered.
//
// Which geometries carry the second loop body: 2048-bin rows on 256 x 8 only, where it was measured to pay (33.2 -> 32.2 us per headline
// step, 106 -> 118 VGPRs, still four waves per SIMD).  A kernel is allocated the registers of its hungrier body, and compiled into every
// geometry the second body cost the others an occupancy step or pushed them into scratch without a measurement to show for it:
// 8192 bins (1024 x 8) 122 -> 128 VGPRs + 152 bytes of scratch, 4096 bins (512 x 8) 111 -> 134 (one workgroup per CU instead of two),
// 1025 bins on one wave (64 x 17) 152 -> 192 (two waves per SIMD instead of three), run-time lengths on 512 x 8 122 -> 143; one-wave rows
// have no workgroup barrier to lose in the first place.  Those keep the single loop.
template <int G, int CPT, int ROWS, int NX>
constexpr bool kAreaPlainLoop = (G == 256 && CPT == 8 && ROWS == 1 && NX == 0);

template <int G, int CPT, int ROWS, bool SQ, int NX, class WT = float>
__device__ __forceinline__ void area_rows_plain(const FwdArgs& a, const FullCtx& c, float (&rx)[CPT], float (&ry)[CPT], const float (&dx)[CPT],
                                                int64_t row0, int64_t row_step, unsigned long long* sacc)
{
    (void)sacc;
    constexpr int NW = FullGeo<G, CPT, ROWS, false, NX>::NW;
    const int rg = c.rg, t = c.t, lane = c.lane, wv = c.wv;
    float* const red = c.red;
    float* const row_loss = a.row_loss;
    int64_t pending = -1;   // the row whose wave sums wait in red[] (wave-uniform)
    const auto store_pending = [&] {
        if (NW > 1 && t == G - kWave && pending >= 0) {
            float tot = red[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) tot += red[w];
            row_loss[pending] = tot;
        }
    };
    if (row0 >= a.B) return;
    for (;;) {
        const int64_t row = row0 + rg;
        const bool valid = ROWS == 1 || row < a.B;
        const int64_t next0 = row0 + row_step;
        const bool more = next0 < a.B;
        const int64_t rn = min(next0 + rg, a.B - 1);
        float wx[CPT], wy[CPT], cu[CPT], cv[CPT];
        float Sx, Sy;
#ifdef SOT_STAMPS
        if (sacc != nullptr) sacc[15] = __builtin_readcyclecounter();
#endif
        full_build_cdfs<G, CPT, ROWS, false, SQ, NX, false, false, true, std::remove_const_t<decltype(store_pending)>, WT>(
            a, c, rx, ry, more ? weight_row<WT>(a.x, rn, a.xs) : nullptr, more ? weight_row<WT>(a.y, rn, a.ys) : nullptr, wx, wy, Sx, Sy, cu, cv, sacc,
            nullptr, nullptr, store_pending);
        SOT_PH(sacc, 9);   // wave totals, CDF values, next row's loads issued
        float acc = 0.0f;
        static_assert(CPT % 2 == 0, "kAreaPlainLoop: 8 elements per thread");
#pragma unroll
        for (int k = 0; k < CPT; k += 2) {   // the differences on pairs (v_pk_add_f32 with neg); the sum stays one chain in element order
            const f32x2 d = f32x2{cu[k], cu[k + 1]} - f32x2{cv[k], cv[k + 1]};
            acc = fmaf(fabsf(d.x), dx[k], acc);
            acc = fmaf(fabsf(d.y), dx[k + 1], acc);
        }
        acc = wave_sum(acc);
        if (NW == 1) {
            if (lane == 0 && valid) row_loss[row] = acc;
            row_sync<NW>();  // Sv of this row is consumed before the next row rewrites it
        } else {
            if (lane == 0) red[wv] = acc;
            pending = valid ? row : -1;
        }
#ifdef SOT_STAMPS
        SOT_PH(sacc, 10);  // area, wave sum (the store: behind barrier 1 of the next row)
        if (sacc != nullptr) sacc[0] += 1;
#endif
        if (!more) break;
        row0 = next0;
    }
    if constexpr (NW > 1) {
        row_sync<NW>();
        store_pending();
    }
}

template <int G, int CPT, int ROWS, bool SQ, int NX = 0, class WT = float>
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
        fetch_row<G, CPT, NX, WT>(weight_row<WT>(a.x, r, a.xs), weight_row<WT>(a.y, r, a.ys), t, a.n, rx, ry);
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
#else
    constexpr unsigned long long* sacc = nullptr;
#endif

    // one wave-uniform test per launch: the plain launch takes the loop compiled for it, every other one the general loop below
    constexpr bool PLAIN_LOOP = kAreaPlainLoop<G, CPT, ROWS, NX>;
    bool plain = false;
    if constexpr (PLAIN_LOOP) plain = c.x_ident && c.y_ident && !c.dn && a.row_loss != nullptr && a.mt.counters == nullptr;
    if (plain) {
        if constexpr (PLAIN_LOOP) area_rows_plain<G, CPT, ROWS, SQ, NX, WT>(a, c, rx, ry, dx, row0, row_step, sacc);
    } else {
    for (; row0 < a.B; row0 += row_step) {
        const int64_t row = row0 + rg;
        const bool valid = row < a.B;
        const bool more = row0 + row_step < a.B;
        const int64_t rn = min(row0 + row_step + rg, a.B - 1);
        float wx[CPT], wy[CPT], cu[CPT], cv[CPT];
        float Sx, Sy;
#ifdef SOT_STAMPS
        if (sacc != nullptr) sacc[15] = __builtin_readcyclecounter();
        full_build_cdfs<G, CPT, ROWS, false, SQ, NX, false, false, false, NoRowHook, WT>(
            a, c, rx, ry, more ? weight_row<WT>(a.x, rn, a.xs) : nullptr, more ? weight_row<WT>(a.y, rn, a.ys) : nullptr, wx, wy, Sx, Sy, cu, cv, sacc);
        SOT_PH(sacc, 9);   // wave totals, CDF values, next row's loads issued
#else
        full_build_cdfs<G, CPT, ROWS, false, SQ, NX, false, false, false, NoRowHook, WT>(
            a, c, rx, ry, more ? weight_row<WT>(a.x, rn, a.xs) : nullptr, more ? weight_row<WT>(a.y, rn, a.ys) : nullptr, wx, wy, Sx, Sy, cu, cv);
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
    if (a.mt.counters != nullptr) batch_mean_tail<ROWS * G>(a.mt, a.row_loss, a.B, reinterpret_cast<double*>(smem));
    }
#ifdef SOT_STAMPS
    if (sacc != nullptr) { for (int i = 0; i < 16; ++i) g_stamps[i] = sacc[i]; }
#endif
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

// WT (here and below): the element type of the weight rows in memory -- same LDS layout, block and row groups whatever it is
template <int G, int CPT, int ROWS, bool SQ, int NX, class WT = float>
static hipError_t launch_area_full(const FwdArgs& a, hipStream_t s)
{
    constexpr FullLayout L = full_layout<G, CPT, ROWS, false, NX>();
    return launch_persistent_profiled<sot_area_full_kernel<G, CPT, ROWS, SQ, NX, WT>>(a, sizeof(float) * (size_t)ROWS * (size_t)L.rowf, (a.B + ROWS - 1) / ROWS,
                                                                                   ROWS * G, s);
}

template <int G, int CPT, int ROWS, int NX = 0, class WT = float>
static hipError_t dispatch_area_full_g(const FwdArgs& a, hipStream_t s)
{
    return (a.flags & SOT_FLAG_SQUARE) ? launch_area_full<G, CPT, ROWS, true, NX, WT>(a, s) : launch_area_full<G, CPT, ROWS, false, NX, WT>(a, s);
}

// 512 / 1024 / 2048 / 4096 bins on shared positions: the geometries of the merge-free kernel for either element type (declared in sot_launch.hpp)
template <class WT>
hipError_t dispatch_area_full_pow2(const FwdArgs& a, hipStream_t s)
{
    switch (a.n) {
        case 512: return dispatch_area_full_g<64, 8, 4, 0, WT>(a, s);
        case 1024: return dispatch_area_full_g<128, 8, 2, 0, WT>(a, s);
        case 2048: return dispatch_area_full_g<256, 8, 1, 0, WT>(a, s);
        case 4096: return dispatch_area_full_g<512, 8, 1, 0, WT>(a, s);
        default: return hipErrorInvalidConfiguration;
    }
}

template <int CPT, int ROWS, bool SQ, int N>
static hipError_t launch_area_half(const FwdArgs& a, hipStream_t s)
{
    constexpr size_t lds = sizeof(float) * (size_t)ROWS * (2 * (32 * CPT + 4) + 64 + 8);
    return launch_persistent_profiled<sot_area_half_kernel<CPT, ROWS, SQ, N>>(a, lds, (a.B + ROWS - 1) / ROWS, ROWS * 32, s);
}

template <int CPT, int ROWS, int N>
static hipError_t dispatch_area_half(const FwdArgs& a, hipStream_t s)
{
    return (a.flags & SOT_FLAG_SQUARE) ? launch_area_half<CPT, ROWS, true, N>(a, s) : launch_area_half<CPT, ROWS, false, N>(a, s);
}

template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX, bool RP = false, class WT = float>
static hipError_t launch_forward_full(const FwdArgs& a, hipStream_t s)
{
    constexpr FullLayout L = full_layout<G, CPT, ROWS, false, NX>();
    return launch_persistent_profiled<sot_forward_full_kernel<G, CPT, ROWS, PM, LIM, SQ, NX, RP, WT>>(a, sizeof(float) * (size_t)L.total, (a.B + ROWS - 1) / ROWS,
                                                                                                   ROWS * G, s);
}

template <int G, int CPT, int ROWS, int NX = 0, class WT = float>
static hipError_t dispatch_forward_full_g(int pm, const FwdArgs& a, hipStream_t s)
{
    static_assert(sizeof(float) * (size_t)full_layout<G, CPT, ROWS, false, NX>().total <= kLdsLimit, "workgroup fits one CU's LDS");
    return with_mode(pm, a.flags, [&](auto md) { using M = decltype(md); return launch_forward_full<G, CPT, ROWS, M::PM, M::LIM, M::SQ, NX, false, WT>(a, s); });
}

// 512 / 1024 / 2048 / 4096 bins on shared positions: the geometries of the merge kernel for either element type (declared in sot_launch.hpp)
template <class WT>
hipError_t dispatch_forward_full_pow2(int pm, const FwdArgs& a, hipStream_t s)
{
    switch (a.n) {
        case 512: return dispatch_forward_full_g<64, 8, 4, 0, WT>(pm, a, s);
        case 1024: return dispatch_forward_full_g<128, 8, 2, 0, WT>(pm, a, s);
        case 2048: return dispatch_forward_full_g<256, 8, 1, 0, WT>(pm, a, s);
        case 4096: return dispatch_forward_full_g<512, 8, 1, 0, WT>(pm, a, s);
        default: return hipErrorInvalidConfiguration;
    }
}

// Per-row positions with handed-over permutations on the compile-time geometries of 2048- / 1024- / 512-point rows, ONE row per workgroup (round 6).
// Preconditions (run_forward): n == m in {512, 1024, 2048}, rows and permutation rows 16-byte aligned, a.perm_in complete, SOT_FLAG_REQUIRE_SORT.
template <int G>
static hipError_t dispatch_forward_full_rowpos_g(int pm, const FwdArgs& a, hipStream_t s)
{
    return with_mode(pm, a.flags, [&](auto md) { using M = decltype(md); return launch_forward_full<G, 8, 1, M::PM, M::LIM, M::SQ, 0, true>(a, s); });
}

template <int CPT, int ROWS, int PM, bool LIM, bool SQ, int N>
static hipError_t launch_forward_half(const FwdArgs& a, hipStream_t s)
{
    constexpr size_t lds = sizeof(float) * (size_t)ROWS * HalfRowGeo<CPT, ROWS, PM, LIM, SQ, N>::ROWF;
    return launch_persistent_profiled<sot_forward_half_kernel<CPT, ROWS, PM, LIM, SQ, N>>(a, lds, (a.B + ROWS - 1) / ROWS, ROWS * 32, s);
}

template <int CPT, int ROWS, int N>
static hipError_t dispatch_forward_half(int pm, const FwdArgs& a, hipStream_t s)
{
    return with_mode(pm, a.flags, [&](auto md) { using M = decltype(md); return launch_forward_half<CPT, ROWS, M::PM, M::LIM, M::SQ, N>(a, s); });
}

}  // namespace sot
