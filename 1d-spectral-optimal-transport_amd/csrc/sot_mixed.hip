// sot_mixed.hip -- MIXED SUPPORTS: one measure on a position row shared by every batch row, the other with positions of its own per
// row (losses.py:162-170 of the reference: a dense target spectrum on the STFT bin grid against a model's line spectrum of K partials
// per frame).  Forward row losses, weight gradients of both sides, position gradient of the per-row side; entry points
// sot_w1d_mixed_* (include/sot_hip.h).
//
// The kernels are the generic per-row-position pipelines of sot_rows.hpp / sot_posgrad.hip with another front end: everything behind
// "PX / PY hold the sorted supports, ix / iy the original column of each sorted element" -- ATen-ordered row masses, safe_divide,
// fp64-accumulated CDFs (build_cdfs, so U and V carry the bits every other route produces), merge-path walk, weight_grad_tail -- is
// shared code.  The front end:
//   * shared side: its SORTED positions (the position plan's, as on the all-shared route), the clamp slot behind them and the
//     walk's front padding are written to the row group's LDS ONCE PER WORKGROUP, before the row loop; nothing in a row's pipeline
//     writes that region.  The plan's permutation entries of the CPT elements a thread owns stay in registers for the whole loop.
//   * per-row side: K <= 2048 positions per row, loaded coalesced, tested for sortedness and -- only if some row of the workgroup
//     needs it -- stably sorted in LDS with an index payload (merge_sort16_kv2 with one job).  The backward kernels sort again.
// LDS layout: make_layout(n, m, G, rowpos = true, with_grad = true) of the generic kernels, i.e.  [pad|U][V][pad|PX][PY] | mass
// scratch | [pad|GU][GV]; the sort's index payload aliases the raw-weight region of the per-row side (U or V) until the weights
// arrive.  HBM per row: 4 (n + m) bytes of weights, 4 K bytes of positions, 4 bytes out -- against 8 (n + m) + 8 n_shared + 2 (n + m)
// on the materialising route (positions at 4 bytes per point on both sides, the expanded copy written and read, uint16 permutations
// written and read).
// Domain (mixed_domain): per-row side 1 ... 2048 points, and the pair fits pick_cfg(n, m, rowpos, with_grad) with room for the
// position gradient's per-thread tails (8 bytes per thread) -- one test for all three kernels.
// Deterministic (no atomics), enqueue-only, persistent grid.
#include "sot_launch.hpp"

namespace sot {

constexpr int kMixedMaxRowSide = 2048;

struct MixedGradArgs {
    FwdArgs f;                 // f.xps / f.yps: exactly one is 0 (the shared side); f.xperm / f.yperm: the shared side's plan permutation
                               // (null: identity); f.ident: ONE device flag, the shared side's "already sorted" (null with a null permutation)
    const float* grad_row; int64_t grad_row_stride; float grad_scale;
    float* gx; float* gy;      // weight gradients [B, n] / [B, m]
    float* gpos;               // position gradient of the per-row side [B, K]
};

// ---- shared side, once per workgroup: sorted positions -> LDS (with the clamp slot and, for x, the walk's front padding); is[k]: the
// original column of sorted element t CPT + k.  The first barrier of the row loop orders these stores before any read.
template <int G, int CPT>
__device__ __forceinline__ void mixed_stage_shared(const FwdArgs& a, const RowCtx<G>& c, bool xrow, int (&is)[CPT])
{
    const int ns = xrow ? c.m : c.n;
    const float* const spos = xrow ? a.ypos : a.xpos;
    const int* const sperm = xrow ? a.yperm : a.xperm;
    float* const PS = xrow ? c.PY : c.PX;
    const bool ident = sperm == nullptr || (a.ident != nullptr && a.ident[0] != 0);
    for (int e = c.t; e < ns; e += G) PS[e] = spos[e];
    if (c.t == 0) PS[ns] = spos[ns - 1];                                        // clamp of losses.py:220
    if (!xrow) for (int e = c.t; e < c.pad; e += G) c.PX[e - c.pad] = spos[0];  // pads sit at the first position (zero width)
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int e = c.t * CPT + k;
        is[k] = (!ident && e < ns) ? min(max(sperm[e], 0), ns - 1) : e;         // (clamped: a foreign plan must not become a wild index)
    }
}

// ---- per-row side, every row: positions -> LDS, stably sorted with an index payload when REQUIRE_SORT finds them unsorted; ir[k]: the
// original column of sorted element t CPT + k.  Ends with a barrier (the payload's region may be overwritten by the weights afterwards).
template <int G, int CPT>
__device__ __forceinline__ void mixed_sort_row(const RowCtx<G>& c, bool xrow, bool want_sort, const float* rp, int (&ir)[CPT])
{
    constexpr int NW = G / kWave;
    const int nr = xrow ? c.n : c.m, t = c.t;
    float* const PR = xrow ? c.PX : c.PY;
    int* const IR = reinterpret_cast<int*>(xrow ? c.U : c.V);
    const int np = sort16_npad(nr);   // one block of 16 per thread: nr <= min(2048, G CPT), so np / 16 <= G in every geometry of pick_cfg
    float v[CPT], w1[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int e = t + k * G;
        v[k] = (e < nr) ? rp[e] : INFINITY;
        w1[k] = (want_sort && e + 1 < nr) ? rp[e + 1] : INFINITY;   // right neighbour for the sortedness test
    }
    int unsorted = 0;
    if (want_sort) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t + k * G;
            if (e < np) PR[e] = v[k];
            unsorted |= (v[k] > w1[k]);
        }
        for (int e = t + CPT * G; e < np; e += G) PR[e] = INFINITY;   // padding of the sort past the slots
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = t + k * G;
            if (e < nr) PR[e] = v[k];
        }
    }
    const bool need_sort = row_any<NW>(unsorted != 0);   // also the barrier after the stores
    if (need_sort) {
        const SortJob jr{PR, IR, nr, np}, none{nullptr, nullptr, 0, 0};
        merge_sort16_kv2<1>(jr, none, t, G, [] { row_sync<NW>(); });   // job.idx is scratch on entry: the sort numbers the elements itself
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int e = t * CPT + k;
        ir[k] = (need_sort && e < nr) ? min(IR[e], nr - 1) : e;   // (clamped: a NaN position can surface a pad's index, see rowpos_prepare)
    }
    row_sync<NW>();
    if (t == 0) PR[nr] = PR[nr - 1];
    if (xrow) for (int e = t; e < c.pad; e += G) { c.PX[e - c.pad] = c.PX[0]; c.U[e - c.pad] = 0.0f; }
}

// common front of the three kernels' row loop body
#define SOT_MIXED_ROW_FRONT()                                                                                          \
    const int64_t row = row0 + rg;                                                                                     \
    const bool valid = row < a.B;                                                                                      \
    const int64_t rowc = valid ? row : a.B - 1;                                                                        \
    int ir[CPT], ix[CPT], iy[CPT];                                                                                     \
    mixed_sort_row<G, CPT>(c, xrow, want_sort, xrow ? a.xpos + rowc * a.xps : a.ypos + rowc * a.yps, ir);              \
    _Pragma("unroll") for (int k = 0; k < CPT; ++k) { ix[k] = xrow ? ir[k] : is[k]; iy[k] = xrow ? is[k] : ir[k]; }    \
    store_row<G, CPT, false>(U, n, t, rx);                                                                             \
    store_row<G, CPT, false>(V, m, t, ry);                                                                             \
    if (row0 + row_step < a.B) {                                                                                       \
        const int64_t r = min(row0 + row_step + rg, a.B - 1);                                                          \
        load_row<G, CPT, false>(a.x + r * a.xs, n, t, rx);                                                             \
        load_row<G, CPT, false>(a.y + r * a.ys, m, t, ry);                                                             \
    }                                                                                                                  \
    row_sync<NW>();                                                                                                    \
    float wx[CPT], wy[CPT];                                                                                            \
    float Sx, Sy;                                                                                                      \
    build_cdfs<G, CPT, true>(a, c, ix, iy, wx, wy, Sx, Sy)

// common head of the three kernels: context, shared side, first row's weights
#define SOT_MIXED_HEAD(WITH_GRAD)                                                                                      \
    constexpr int BLOCK = (G < 256 ? 256 : G);                                                                         \
    constexpr int RPW = BLOCK / G;                                                                                     \
    constexpr int NW = G / kWave;                                                                                      \
    extern __shared__ __attribute__((aligned(16))) float smem[];                                                       \
    RowCtx<G> c = make_ctx<G, true>(a, smem, WITH_GRAD);                                                               \
    const bool xrow = a.xps != 0;          /* which side has per-row positions */                                      \
    const bool want_sort = c.do_sort;                                                                                  \
    c.do_sort = true;                      /* the shared code gathers and scatters through ix / iy (identity where nothing was sorted) */ \
    const int rg = threadIdx.x / G;                                                                                    \
    const int n = c.n, m = c.m, t = c.t;                                                                               \
    float* const U = c.U; float* const V = c.V; float* const PX = c.PX; float* const PY = c.PY;                        \
    int is[CPT];                                                                                                       \
    mixed_stage_shared<G, CPT>(a, c, xrow, is);                                                                        \
    const int64_t row_step = (int64_t)gridDim.x * RPW;                                                                 \
    int64_t row0 = (int64_t)blockIdx.x * RPW;                                                                          \
    float rx[CPT], ry[CPT];                                                                                            \
    if (row0 < a.B) {                                                                                                  \
        const int64_t r = min(row0 + rg, a.B - 1);                                                                     \
        load_row<G, CPT, false>(a.x + r * a.xs, n, t, rx);                                                             \
        load_row<G, CPT, false>(a.y + r * a.ys, m, t, ry);                                                             \
    }

// ---------------------------------------------------------------------------------------------
// Forward: row losses.  The walk is sot_forward_kernel's "loser" form (sot_rows.hpp).
// ---------------------------------------------------------------------------------------------
template <int G, int CPT, int PM, bool LIM>
__global__ __launch_bounds__((G < 256 ? 256 : G)) void sot_mixed_forward_kernel(const FwdArgs a)
{
    SOT_MIXED_HEAD(false)
    for (; row0 < a.B; row0 += row_step) {
        SOT_MIXED_ROW_FRONT();
        float acc = 0.0f;
        __builtin_amdgcn_s_setprio(kWalkPrio);
        if (t < c.Ga) {
            const float* const Uw = U - c.pad;
            const float* const PXw = PX - c.pad;
            const int nw = n + c.pad;
            const int D0 = t * c.E;
            const uint32_t ub1 = lds_addr(Uw) - 4u;
            const int i0 = (int)((merge_path_steps32(ub1, lds_addr(V) + 4u * (uint32_t)D0 + ub1, nw, m, D0, c.topk) - ub1) >> 2);
            const int j0 = D0 - i0;
            float qprev = 0.0f;   // Q_0 := 0 (the pad of losses.py:301)
            if (i0 > 0) qprev = Uw[i0 - 1];
            if (j0 > 0) qprev = fmaxf(qprev, V[j0 - 1]);
            const uint32_t poff4 = 4u * (uint32_t)c.L.poff;
            const int voff = (int)(V - Uw);
            float w = Uw[i0], wp = PXw[i0], r = V[j0], rp = PY[j0];
            const uint32_t lb32 = lds_addr(Uw);
            uint32_t pw = lb32 + 4u * (uint32_t)i0 + 4u, pr = lb32 + 4u * (uint32_t)(voff + j0) + 4u;
#pragma unroll SOT_WALK_UNROLL
            for (int s = 0; s < c.E; ++s) {
                const bool cw = w <= r;
                const float q = cw ? w : r;
                const float cost = transport_cost<PM>(wp, rp, c.p);
                float delta = q - qprev;
                if (LIM && q > 1.0f) delta = 0.0f;
                acc = fmaf(delta, cost, acc);
                qprev = q;
                const uint32_t nx = cw ? pw : pr;
                pr = cw ? pr : pw;
                pw = nx + 4u;
                r = cw ? r : w;
                rp = cw ? rp : wp;
                w = lds_load(nx);
                wp = lds_load(nx + poff4);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        acc = wave_sum(acc);
        if (NW == 1) {
            if (t == 0 && valid) a.row_loss[row] = acc;
            row_sync<NW>();   // this row's LDS reads are done before the next row's staging
        } else {
            if (c.lane == 0) c.red[c.wv] = acc;
            row_sync<NW>();
            if (t == 0 && valid) {
                float tot = c.red[0];
                for (int w = 1; w < NW; ++w) tot += c.red[w];
                a.row_loss[row] = tot;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Weight gradients of both sides: sot_backward_kernel's walk (tie convention: stable order, U before V, lowest index first; a run of
// equal levels hands its gradient to its last member) and weight_grad_tail.
// ---------------------------------------------------------------------------------------------
template <int G, int CPT, int PM, bool LIM>
__global__ __launch_bounds__((G < 256 ? 256 : G)) void sot_mixed_backward_kernel(const MixedGradArgs b)
{
    const FwdArgs& a = b.f;
    SOT_MIXED_HEAD(true)
    for (; row0 < a.B; row0 += row_step) {
        SOT_MIXED_ROW_FRONT();
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
                qprev = __int_as_float(0x7fc00000);   // NaN: the very first level always starts a run
            } else if (fminf(ua, vb) == qprev) {       // we start inside a run: cost at its first member's ranks
                const float q0 = qprev;
                const float cst = transport_cost<PM>(PX[lower_rank(U, n, q0)], PY[lower_rank(V, m, q0)], c.p);
                dcur = (LIM && q0 > 1.0f) ? 0.0f : cst;
            }
            char* const lb = reinterpret_cast<char*>(const_cast<float*>(Uw));
            const uint32_t poff4 = 4u * (uint32_t)c.L.poff;
            const uint32_t goff4 = 4u * (uint32_t)c.L.grad;
            const int voff = (int)(V - Uw);
            uint32_t iu = (uint32_t)i0;
            uint32_t prev_off = 4u * (uint32_t)(c.pad + n);   // U[n]'s gradient slot: a scratch target for "no element yet"
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
                prev_off = 4u * (tu ? iu : (vk - iu));   // slot of the element consumed now
                iu += tu ? 1u : 0u;
                const uint32_t off = prev_off + 4u;      // the consumed side's next element
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
        row_sync<NW>();
        weight_grad_tail<G, CPT, true, false>(a, c, ix, iy, wx, wy, Sx, Sy, b.grad_row, b.grad_row_stride, b.grad_scale, b.gx, b.gy, row, rowc, valid);
        row_sync<NW>();   // GU / GV / wtot reads done before the next row reuses LDS
    }
}

// ---------------------------------------------------------------------------------------------
// Position gradient of the per-row side: sot_position_grad_kernel's scheme (sot_posgrad.hip) for ONE side.  With delta_k the width of
// merged level k and (i_k, j_k) its searchsorted ranks,  d row_loss / d xs[i] = sum_{k : i_k = i} delta_k p |xs[i_k] - ys[j_k]|^(p-1) sign(.),
// ys[j]: minus the same.  The terms of element i of the per-row side are the walk steps between the consumption of its predecessor and
// its own, a range that may span threads: the consuming thread ASSIGNS its own steps' sum to slot i, every thread leaves the sum behind
// its last consumed element as a (slot, value) tail, and after a barrier the first thread of each run of equal tail slots adds the
// run's values in thread order.  Levels past the side's last element are clamped onto it (losses.py:220).  No atomics.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float mixed_cost_slope(float d, int pm, float p)
{
    if (pm == 1) return (float)(d > 0.0f) - (float)(d < 0.0f);   // d |d| / dd, 0 at 0 (torch.abs backward)
    if (pm == 2) return 2.0f * d;
    return copysignf(p * pow_nonneg(fabsf(d), p - 1.0f), d);
}

template <int G, int CPT>
__global__ __launch_bounds__((G < 256 ? 256 : G)) void sot_mixed_position_grad_kernel(const MixedGradArgs b)
{
    const FwdArgs& a = b.f;
    SOT_MIXED_HEAD(true)
    // per-thread tails (value, slot) of the Ga walking threads: in the row's dead CDF region when it is large enough, else behind the rows
    const bool tails_in_cdfs = 2 * c.Ga <= n + m;
    const int tstride = tails_in_cdfs ? c.Ga : G;
    float* const tail_v = tails_in_cdfs ? U : smem + RPW * c.L.row_floats + rg * 2 * G;
    int* const tail_s = reinterpret_cast<int*>(tail_v + tstride);
    const int pm = (a.p == 1.0f) ? 1 : ((a.p == 2.0f) ? 2 : 0);
    const bool lim = c.lim;
    const int nr = xrow ? n : m;
    float* const GRw = xrow ? c.GU - c.pad : c.GV;      // slots of the per-row side, indexed like the walk's arrays (Uw / V)
    const int last = xrow ? n + c.pad : m;              // the "past the end" slot
    for (; row0 < a.B; row0 += row_step) {
        SOT_MIXED_ROW_FRONT();
        (void)wx; (void)wy; (void)Sx; (void)Sy;
        if (t == 0) GRw[last] = 0.0f;   // nobody consumes the sentinel: this slot only receives tails
        float tv = 0.0f;
        int ts = -1;
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
            char* const lb = reinterpret_cast<char*>(const_cast<float*>(Uw));
            const uint32_t poff4 = 4u * (uint32_t)c.L.poff;
            const uint32_t goff4 = 4u * (uint32_t)c.L.grad;
            const int voff = (int)(V - Uw);
            uint32_t iu = (uint32_t)i0;
            float acc = 0.0f;   // sum of the per-row side's run that is open at this step
            for (int s = 0; s < c.E; ++s) {
                const bool tu = ua <= vb;   // canonical stable order: U before V on ties
                const float q = tu ? ua : vb;
                float delta = q - qprev;
                if (lim && q > 1.0f) delta = 0.0f;
                acc += delta * mixed_cost_slope(xa - yb, pm, c.p);
                qprev = q;
                const uint32_t vk = (uint32_t)(voff + D0 + s);
                const uint32_t off = 4u * (tu ? iu : (vk - iu));
                if (tu == xrow) {   // an element of the per-row side is consumed: it closes its run
                    *reinterpret_cast<float*>(lb + off + goff4) = acc;
                    acc = 0.0f;
                }
                iu += tu ? 1u : 0u;
                const float nv = *reinterpret_cast<const float*>(lb + off + 4u);
                const float np = *reinterpret_cast<const float*>(lb + off + 4u + poff4);
                ua = tu ? nv : ua;
                xa = tu ? np : xa;
                vb = tu ? vb : nv;
                yb = tu ? yb : np;
            }
            tv = acc;
            ts = xrow ? (int)iu : D0 + c.E - (int)iu;   // the per-row side's head when this segment ends; `last` = past the end
        }
        row_sync<NW>();   // every walk is done: the CDFs may be overwritten by the tails
        if (t < c.Ga) { tail_v[t] = tv; tail_s[t] = ts; }
        row_sync<NW>();
        if (t < c.Ga && (t == 0 || tail_s[t - 1] != ts)) {   // first thread of a run of equal tail slots: one writer per slot
            float sum = tv;
            for (int u = t + 1; u < c.Ga && tail_s[u] == ts; ++u) sum += tail_v[u];
            GRw[ts] = sum + GRw[ts];
        }
        row_sync<NW>();
        if (t == 0) GRw[last - 1] += GRw[last];   // clamp of losses.py:220
        row_sync<NW>();
        if (valid) {
            const float gr = (b.grad_row ? b.grad_row[rowc * b.grad_row_stride] : 1.0f) * b.grad_scale;
            const float* const GR = xrow ? c.GU : c.GV;
            float* dst = b.gpos + row * (int64_t)nr;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int e = t * CPT + k;
                if (e < nr) dst[ir[k]] = xrow ? GR[e] * gr : -(GR[e] * gr);
            }
        }
        row_sync<NW>();   // slot reads done before the next row reuses LDS (build_cdfs rewrites the sentinels under the tails)
    }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
struct MixedLaunch {
    FwdArgs a;
    LaunchCfg cfg;
    size_t lds_fwd, lds_grad, lds_pos;
    int block, rpw;
    int64_t want;
    int pm;
    hipStream_t s;
};

// The domain of the three kernels, one test (host arithmetic only): the per-row side has 1 ... 2048 points and the pair has a geometry
// whose gradient layout, plus the position gradient's tails, fits one CU's LDS.
static bool mixed_domain(int n, int m, bool xrow, MixedLaunch* l)
{
    const int nr = xrow ? n : m;
    if (nr < 1 || nr > kMixedMaxRowSide) return false;
    int rpw = 1, blk = 0;
    size_t lds_grad = 0;
    LaunchCfg cfg;
    if (!pick_cfg(n, m, true, true, &cfg, &lds_grad, &blk, &rpw)) return false;
    if (cfg.CPT == 16) return false;   // (a side beyond 8192 points: its power-of-two sort image never fits the gradient layout; no kernels are built for it)
    const size_t lds_pos = lds_grad + 2 * sizeof(float) * (size_t)blk;
    if (lds_pos > kLdsLimit) return false;
    if (l != nullptr) {
        l->cfg = cfg; l->block = blk; l->lds_grad = lds_grad; l->lds_pos = lds_pos;
        l->lds_fwd = (size_t)rpw * make_layout(n, m, cfg.G, true, false).row_floats * sizeof(float);
        l->rpw = rpw;
    }
    return true;
}

static int validate_mixed(const sot_problem* pr)
{
    if (pr == nullptr) return SOT_ERR_NULL_POINTER;
    if (!(pr->p >= 1.0f)) return SOT_ERR_INVALID_P;
    if (pr->B < 0 || pr->n < 1 || pr->m < 1) return SOT_ERR_BAD_SHAPE;
    if (pr->x_row_stride < pr->n || pr->y_row_stride < pr->m) return SOT_ERR_BAD_SHAPE;
    if ((pr->xpos_row_stride == 0) == (pr->ypos_row_stride == 0)) return SOT_ERR_BAD_SHAPE;   // exactly one side is shared
    if (pr->xpos_row_stride != 0 && pr->xpos_row_stride < pr->n) return SOT_ERR_BAD_SHAPE;
    if (pr->ypos_row_stride != 0 && pr->ypos_row_stride < pr->m) return SOT_ERR_BAD_SHAPE;
    if (!mixed_domain(pr->n, pr->m, pr->xpos_row_stride != 0, nullptr)) return SOT_ERR_UNSUPPORTED_SIZE;
    if (pr->B > 0 && (!pr->x || !pr->y || !pr->xpos || !pr->ypos)) return SOT_ERR_NULL_POINTER;
    return SOT_OK;
}

// the in-call plan of the shared side: launch_prepare sorts two arrays at once, so the grid is planned as both of them
static size_t mixed_workspace_bytes(const sot_problem* pr)
{
    if (!(pr->flags & SOT_FLAG_REQUIRE_SORT) || pr->perm_is_identity != nullptr) return 0;
    const int ns = pr->xpos_row_stride != 0 ? pr->m : pr->n;
    return ws_layout(ns, ns).total;
}

// validation, geometry, the shared side's plan (the caller's, or planned here into the workspace)
static int setup_mixed(const sot_problem* pr, void* workspace, size_t workspace_bytes, void* stream, MixedLaunch* l)
{
    const int rc = validate_mixed(pr);
    if (rc != SOT_OK) return rc;
    const bool xrow = pr->xpos_row_stride != 0;
    mixed_domain(pr->n, pr->m, xrow, l);
    l->want = (pr->B + l->rpw - 1) / l->rpw;
    l->s = reinterpret_cast<hipStream_t>(stream);
    l->pm = (pr->p == 1.0f) ? 1 : ((pr->p == 2.0f) ? 2 : 0);
    FwdArgs a{};
    a.x = pr->x; a.y = pr->y; a.xpos = pr->xpos; a.ypos = pr->ypos;
    a.B = pr->B; a.n = pr->n; a.m = pr->m;
    a.xs = pr->x_row_stride; a.ys = pr->y_row_stride; a.xps = pr->xpos_row_stride; a.yps = pr->ypos_row_stride;
    a.p = pr->p; a.flags = pr->flags;
    const float* spos = xrow ? pr->ypos : pr->xpos;
    const int* sperm = nullptr;
    if (pr->flags & SOT_FLAG_REQUIRE_SORT) {
        if (pr->perm_is_identity != nullptr) {   // caller-provided plan: the shared side's positions are the sorted ones
            sperm = xrow ? pr->yperm : pr->xperm;
            if (sperm == nullptr) return SOT_ERR_NULL_POINTER;
            a.ident = pr->perm_is_identity + (xrow ? 1 : 0);
        } else if (pr->B > 0) {
            const int ns = xrow ? pr->m : pr->n;
            const WsLayout w = ws_layout(ns, ns);
            if (workspace == nullptr) return SOT_ERR_NULL_POINTER;
            if (workspace_bytes < w.total) return SOT_ERR_WORKSPACE;
            char* ws = reinterpret_cast<char*>(workspace);
            float* sx = reinterpret_cast<float*>(ws + w.sx);
            int* px = reinterpret_cast<int*>(ws + w.px);
            int* ident = reinterpret_cast<int*>(ws + w.ident);
            const int prc = launch_prepare(spos, spos, ns, ns, sx, reinterpret_cast<float*>(ws + w.sy), px, reinterpret_cast<int*>(ws + w.py), ident, l->s);
            if (prc != SOT_OK) return prc;
            spos = sx; sperm = px; a.ident = ident;
        }
    }
    if (xrow) { a.ypos = spos; a.yperm = sperm; } else { a.xpos = spos; a.xperm = sperm; }
    l->a = a;
    return SOT_OK;
}

// KIND 0: forward, 1: weight gradients, 2: position gradient
template <int KIND, int G, int CPT>
static hipError_t dispatch_mixed_g(const MixedLaunch& l, const MixedGradArgs& b)
{
    if constexpr (KIND == 2) {
        // the per-thread tails live in the row's dead CDFs when they fit there (see the kernel), else behind the rows
        const int E = merge_steps(l.a.n + l.a.m, G), Ga = (l.a.n + l.a.m + E - 1) / E;
        return launch_persistent<sot_mixed_position_grad_kernel<G, CPT>>(b, (2 * Ga <= l.a.n + l.a.m) ? l.lds_grad : l.lds_pos, l.want, l.block, l.s);
    } else {
        const bool lim = l.a.flags & SOT_FLAG_LIMIT_Q;
        const auto launch = [&](auto pmc, auto limc) {
            constexpr int PM = decltype(pmc)::value;
            constexpr bool LIM = decltype(limc)::value;
            if constexpr (KIND == 0) return launch_persistent<sot_mixed_forward_kernel<G, CPT, PM, LIM>>(l.a, l.lds_fwd, l.want, l.block, l.s);
            else return launch_persistent<sot_mixed_backward_kernel<G, CPT, PM, LIM>>(b, l.lds_grad, l.want, l.block, l.s);
        };
        return with_pm(l.pm, [&](auto pmc) { return lim ? launch(pmc, std::true_type{}) : launch(pmc, std::false_type{}); });
    }
}

template <int KIND>
static hipError_t dispatch_mixed(const MixedLaunch& l, const MixedGradArgs& b)
{
    switch (l.cfg.G) {   // (1024 x 16 is outside mixed_domain)
        case 64: return dispatch_mixed_g<KIND, 64, 8>(l, b);
        case 128: return dispatch_mixed_g<KIND, 128, 12>(l, b);
        case 256: return dispatch_mixed_g<KIND, 256, 8>(l, b);
        default: return dispatch_mixed_g<KIND, 1024, 8>(l, b);
    }
}

}  // namespace sot

extern "C" {

size_t sot_w1d_mixed_workspace_bytes(const sot_problem* prob)
{
    if (sot::validate_mixed(prob) != SOT_OK) return 0;
    return sot::mixed_workspace_bytes(prob);
}

int sot_w1d_mixed_forward(const sot_problem* prob, float* row_loss, void* workspace, size_t workspace_bytes, void* stream)
{
    if (prob != nullptr && prob->B > 0 && row_loss == nullptr) return SOT_ERR_NULL_POINTER;
    sot::MixedLaunch l;
    const int rc = sot::setup_mixed(prob, workspace, workspace_bytes, stream, &l);
    if (rc != SOT_OK) return rc;
    if (prob->B == 0) return SOT_OK;
    l.a.row_loss = row_loss;
    sot::MixedGradArgs b{};
    return sot::launch_status(sot::dispatch_mixed<0>(l, b));
}

int sot_w1d_mixed_backward(const sot_problem* prob, const float* grad_row, int64_t grad_row_stride, float grad_scale, float* grad_x,
                           float* grad_y, void* workspace, size_t workspace_bytes, void* stream)
{
    sot::MixedLaunch l;
    const int rc = sot::setup_mixed(prob, workspace, workspace_bytes, stream, &l);
    if (rc != SOT_OK) return rc;
    if (prob->B == 0 || (grad_x == nullptr && grad_y == nullptr)) return SOT_OK;
    sot::MixedGradArgs b{};
    b.f = l.a; b.grad_row = grad_row; b.grad_row_stride = grad_row_stride; b.grad_scale = grad_scale; b.gx = grad_x; b.gy = grad_y;
    return sot::launch_status(sot::dispatch_mixed<1>(l, b));
}

int sot_w1d_mixed_position_grad(const sot_problem* prob, const float* grad_row, int64_t grad_row_stride, float grad_scale,
                                float* grad_pos, void* workspace, size_t workspace_bytes, void* stream)
{
    if (prob != nullptr && prob->B > 0 && grad_pos == nullptr) return SOT_ERR_NULL_POINTER;
    sot::MixedLaunch l;
    const int rc = sot::setup_mixed(prob, workspace, workspace_bytes, stream, &l);
    if (rc != SOT_OK) return rc;
    if (prob->B == 0) return SOT_OK;
    sot::MixedGradArgs b{};
    b.f = l.a; b.grad_row = grad_row; b.grad_row_stride = grad_row_stride; b.grad_scale = grad_scale; b.gpos = grad_pos;
    return sot::launch_status(sot::dispatch_mixed<2>(l, b));
}

}  // extern "C"
