// sot_full_bwd.hpp -- backward kernels of the full-row family (compile-time geometries) with their launch and dispatch templates,
// namespace sot: the merge backward and the merge-free p = 1 training form.  Included by the objects that instantiate them:
// sot_full_bwd.hip (compile-time row lengths), sot_full_rt_bwd.hip (run-time row lengths) and sot_bf16_bwd.hip (16-bit rows and gradients).
// The non-template dispatch functions live in the first two (dispatch_backward_full, dispatch_area_train, ...); the geometry table of
// 512 ... 4096 bins, which both element types share, is a template here (dispatch_backward_full_pow2).  The forward side is sot_full_fwd.hpp.
#pragma once
#include "sot_full_common.hpp"

namespace sot {

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

// The 16-bit gradient stores of a thread that owns CPT = 8 contiguous elements of a row that fills its geometry (GT = uint16_t): dst = the
// address of the thread's first element in the gradient row (16-byte aligned: the host guarantees 16-byte aligned rows of N elements).
// Identity permutation: one 16-byte store; otherwise single 16-bit elements through the plan's permutation (perm = its entries for e0 ...).
template <int CPT>
__device__ __forceinline__ void store_grad_row_bf16(uint16_t* dst, const float (&o)[CPT], bool ident, const int* perm, int e0)
{
    static_assert(CPT == 8, "8 bfloat16 gradients = one 16-byte store");
    if (ident) {
        uint4 v;
        v.x = (uint32_t)f32_to_bf16_rne(o[0]) | ((uint32_t)f32_to_bf16_rne(o[1]) << 16);
        v.y = (uint32_t)f32_to_bf16_rne(o[2]) | ((uint32_t)f32_to_bf16_rne(o[3]) << 16);
        v.z = (uint32_t)f32_to_bf16_rne(o[4]) | ((uint32_t)f32_to_bf16_rne(o[5]) << 16);
        v.w = (uint32_t)f32_to_bf16_rne(o[6]) | ((uint32_t)f32_to_bf16_rne(o[7]) << 16);
        *reinterpret_cast<uint4*>(dst) = v;
    } else {
        uint16_t* const row = dst - e0;
#pragma unroll
        for (int k = 0; k < CPT; ++k) row[perm[k]] = f32_to_bf16_rne(o[k]);
    }
}

// Gradient rows of the one-sided spectra (129 / 257 / 513 / 1025 / 2049 bins: rows of 4 N bytes, never a multiple of 16) leave the
// kernel through LDS (round 4).  Before: every thread stored its CPT contiguous gradients one dword at a time, i.e. CPT store
// instructions per wave at a lane stride of 4 CPT bytes, each touching every 128-B line of the wave's span partially.  The L2 answered
// the partial writes with line fills and partial write-backs: 16384 x 1025 training form FETCH 1.30 x / WRITE 1.13 x the algorithmic
// bytes (profiles/r3e_b16384n1025_cutoff_rocprofv3_summary.txt).  Now a thread writes its gradients back into the
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
// WT (sot_full_common.hpp: fetch_row): the element type of the weight rows in memory -- float, or uint16_t for bfloat16 rows (a.x / a.y then
// point at 16-bit elements and the row strides count them; instantiated by sot_bf16_bwd.hip).  GT: the element type of the gradient rows
// b.gx / b.gy -- float, or uint16_t for bfloat16 gradients: ox[k] / oy[k] stay the float32 values of the float32 kernel and are rounded once,
// to nearest even, at the store (b.gx / b.gy then point at 16-bit elements, rows of N of them on 16-byte boundaries).  The y-only 16-bit kernel
// also has the FIX-UP mode of BwdArgs::rescale: every workgroup reads the scalar first and returns at once when it is exactly 1 (what
// sot_scale_inplace does); otherwise the stored element is rne(oy[k] * *rescale), one float32 multiply in front of the one rounding.
template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX = 0, bool WANT_X = true, bool SLIM = false, int MINB = 1, bool RP = false,
          class WT = float, class GT = float>
__global__ __launch_bounds__(ROWS * G, MINB) void sot_backward_full_kernel(const BwdArgs b)
{
    constexpr bool G16 = !std::is_same<GT, float>::value;
    static_assert(std::is_same<WT, float>::value || (NX == 0 && !RP), "16-bit rows: rows that fill their geometry, shared positions");
    static_assert(!G16 || (std::is_same<GT, uint16_t>::value && NX == 0 && !RP), "16-bit gradients: bfloat16, rows that fill their geometry, shared positions");
    static_assert(!RP || (ROWS == 1 && NX == 0 && CPT == 8), "per-row positions (see sot_forward_full_kernel): one row per workgroup, rows that fill the 8-element geometry");
    static_assert(!(SLIM && WANT_X), "SLIM is a y-only layout");
    constexpr int GR = SLIM ? 2 : 1;
    using Geo = FullGeo<G, CPT, ROWS, GR, NX>;
    constexpr FullLayout L = Geo::L;
    constexpr int N = Geo::N, NW = Geo::NW, E = Geo::E, GA = Geo::GA, PAD = Geo::PAD;
    constexpr bool WITH_LOSS = !WANT_X;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FwdArgs& a = b.f;
    float rescale = 1.0f;
    bool rescaled = false;   // kernel-uniform
    if constexpr (G16 && !WANT_X) {
        if (b.rescale != nullptr) {
            rescale = *b.rescale;
            if (rescale == 1.0f) return;   // the gradient in place is already the answer (every thread of every workgroup leaves: no barrier is pending)
            rescaled = true;
        }
    }
    (void)rescale; (void)rescaled;
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
        fetch_row<G, CPT, NX, WT>(weight_row<WT>(a.x, r, a.xs), weight_row<WT>(a.y, r, a.ys), t, a.n, rx, ry);
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
        full_build_cdfs<G, CPT, ROWS, GR, SQ, NX, true, true, false, NoRowHook, WT>(
            a, c, rx, ry, more ? weight_row<WT>(a.x, rn, a.xs) : nullptr, more ? weight_row<WT>(a.y, rn, a.ys) : nullptr, wx, wy, Sx, Sy, cu, cv, sacc,
            RP ? psx : nullptr, RP ? psy : nullptr);
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
            if constexpr (G16) {   // bfloat16 gradient rows: rounded at the store, 8 contiguous gradients as one 16-byte store
                if constexpr (WANT_X) {
                    if (b.gx) store_grad_row_bf16<CPT>(reinterpret_cast<uint16_t*>(b.gx) + row * (int64_t)N + e0, ox, c.x_ident, a.xperm + e0, e0);
                }
                if (b.gy) {
                    if (rescaled) {
#pragma unroll
                        for (int k = 0; k < CPT; ++k) oy[k] = oy[k] * rescale;
                    }
                    store_grad_row_bf16<CPT>(reinterpret_cast<uint16_t*>(b.gy) + row * (int64_t)N + e0, oy, c.y_ident, a.yperm + e0, e0);
                }
            }
            if (!G16 && WANT_X && b.gx && !stage_x) {
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
            if (!G16 && b.gy && !stage_y) {
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
    constexpr FullLayout L = full_layout<G, CPT, ROWS, false, NX>();
    const size_t lds = sizeof(float) * (size_t)ROWS * (size_t)L.rowf + sizeof(double) * (size_t)ROWS * 2 * (G / kWave);
    return launch_persistent_profiled<sot_area_train_kernel<G, CPT, ROWS, SQ, NX>>(b, lds, (b.f.B + ROWS - 1) / ROWS, ROWS * G, s);
}

template <int G, int CPT, int ROWS, int NX = 0>
static hipError_t dispatch_area_train_g(const BwdArgs& b, hipStream_t s)
{
    return (b.f.flags & SOT_FLAG_SQUARE) ? launch_area_train<G, CPT, ROWS, true, NX>(b, s) : launch_area_train<G, CPT, ROWS, false, NX>(b, s);
}

// WT / GT (here and below): the weight and gradient element types of sot_backward_full_kernel; same LDS layout, block and row groups whatever they are
template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX, bool WANT_X, bool SLIM = false, int MINB = 1, bool RP = false,
          class WT = float, class GT = float>
static hipError_t launch_backward_full_x(const BwdArgs& b, hipStream_t s)
{
    constexpr FullLayout L = full_layout<G, CPT, ROWS, SLIM ? 2 : 1, NX>();
    return launch_persistent_profiled<sot_backward_full_kernel<G, CPT, ROWS, PM, LIM, SQ, NX, WANT_X, SLIM, MINB, RP, WT, GT>>(
        b, sizeof(float) * (size_t)L.total, (b.f.B + ROWS - 1) / ROWS, ROWS * G, s);
}

// WHICH: bit 0 = the both-gradient kernels, bit 1 = the y-only kernels of this layout (a geometry whose y-only calls go to
// dispatch_backward_full_y instantiates only the former)
template <int G, int CPT, int ROWS, int PM, bool LIM, bool SQ, int NX, int WHICH = 3, class WT = float, class GT = float>
static hipError_t launch_backward_full(const BwdArgs& b, hipStream_t s)
{
    // in dont_normalize mode the y side's mass term lands in the x side's gradient, which needs gx anyway
    if constexpr (WHICH & 1) { if (b.gx != nullptr) return launch_backward_full_x<G, CPT, ROWS, PM, LIM, SQ, NX, true, false, 1, false, WT, GT>(b, s); }
    if constexpr (WHICH & 2) { if (b.gx == nullptr) return launch_backward_full_x<G, CPT, ROWS, PM, LIM, SQ, NX, false, false, 1, false, WT, GT>(b, s); }
    return hipErrorInvalidConfiguration;
}

template <int G, int CPT, int ROWS, int NX = 0, int WHICH = 3, class WT = float, class GT = float>
static hipError_t dispatch_backward_full_g(int pm, const BwdArgs& b, hipStream_t s)
{
    static_assert(sizeof(float) * (size_t)full_layout<G, CPT, ROWS, true, NX>().total <= kLdsLimit, "workgroup fits one CU's LDS");
    return with_mode(pm, b.f.flags, [&](auto md) { using M = decltype(md); return launch_backward_full<G, CPT, ROWS, M::PM, M::LIM, M::SQ, NX, WHICH, WT, GT>(b, s); });
}

// the y-only kernels of one geometry alone (gx == nullptr)
template <int G, int CPT, int ROWS, int NX = 0, bool SLIM = true, int MINB = 1, class WT = float, class GT = float>
static hipError_t dispatch_backward_full_y(int pm, const BwdArgs& b, hipStream_t s)
{
    static_assert(sizeof(float) * (size_t)full_layout<G, CPT, ROWS, SLIM ? 2 : 1, NX>().total <= kLdsLimit, "workgroup fits one CU's LDS");
    return with_mode(pm, b.f.flags, [&](auto md) {
        using M = decltype(md);
        return launch_backward_full_x<G, CPT, ROWS, M::PM, M::LIM, M::SQ, NX, false, SLIM, MINB, false, WT, GT>(b, s);
    });
}

// Waves per SIMD the y-only kernel of 2048-bin rows is compiled for (MINB) -- the one geometry choice that follows the element type.  16-bit
// rows: four.  Uncapped, the modes without square_dist take 129 / 130 VGPRs (float32: 125 / 126), and at three waves per SIMD only ONE of these
// 8-wave workgroups is resident on a CU instead of the two its LDS allows.  (The both-gradient kernel's 129 VGPRs under square_dist cost
// nothing: one row with U slots takes 50.9 KB, three 4-wave workgroups per CU either way.)
template <class WT>
constexpr int kBwdY2048MinB = std::is_same<WT, float>::value ? 1 : 4;

// 512 / 1024 / 2048 / 4096 bins on shared positions: the geometries of the backward for either element type of weight and gradient rows
// (declared in sot_launch.hpp).  y-only calls at 1024 and 2048 bins take the layout without U gradient slots:
// 1024: 34.8 instead of 43.3 KB per two rows = eight rows per CU instead of six: 16384 rows 78.8 -> 73.4 us, 4096 rows 27.3 -> 26.0 us (float32)
// 2048: two rows and the shared position copy take 68.7 KB: two workgroups = four rows per CU instead of three (one row with U slots +
//       positions: 50.9 KB).  Measured at 8192 x 2048, paper mode, float32: 79.7 instead of 81.5 us.
// (512: the slim layout adds a fourth workgroup per CU here too: 64.5 vs 65.0 us, nothing)
template <class WT>
hipError_t dispatch_backward_full_pow2(int pm, const BwdArgs& b, hipStream_t s)
{
    switch (b.f.n) {
        case 512: return dispatch_backward_full_g<64, 8, 4, 0, 3, WT, WT>(pm, b, s);
        case 1024:
            if (b.gx == nullptr) return dispatch_backward_full_y<128, 8, 2, 0, true, 1, WT, WT>(pm, b, s);
            return dispatch_backward_full_g<128, 8, 2, 0, 1, WT, WT>(pm, b, s);
        case 2048:
            if (b.gx == nullptr) return dispatch_backward_full_y<256, 8, 2, 0, true, kBwdY2048MinB<WT>, WT, WT>(pm, b, s);
            return dispatch_backward_full_g<256, 8, 1, 0, 1, WT, WT>(pm, b, s);
        case 4096: return dispatch_backward_full_g<512, 8, 1, 0, 3, WT, WT>(pm, b, s);
        default: return hipErrorInvalidConfiguration;
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
    return with_mode(pm, b.f.flags, [&](auto md) { using M = decltype(md); return launch_backward_full_rowpos<G, M::PM, M::LIM, M::SQ>(b, s); });
}

}  // namespace sot
