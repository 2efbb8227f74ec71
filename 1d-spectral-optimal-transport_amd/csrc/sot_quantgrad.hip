// sot_quantgrad.hip -- vector-Jacobian product of the five return_quantiles tensors.
#include "sot_launch.hpp"

namespace sot {

// ---------------------------------------------------------------------------------------------
// Vector-Jacobian product of the five return_quantiles tensors (losses.py:198-201, 286-300: sort, gather, cumsum, cat + sort,
// searchsorted, take_along_dim -- plain ATen ops that the reference leaves attached to autograd).  With U, V the CDFs of the sorted
// measures, Q = sort(cat(U, V)) and uq_k = xs[min(#{U_i < Q_k}, n - 1)], vq_k likewise, the upstream gradients gUq, gVq, gQ [B, n + m],
// gU [B, n], gV [B, m] (any may be absent) give
//   CDF entries:  GU_i = gU_i + gQ_k(i), GV_j = gV_j + gQ_k(j) with k(.) the entry's place in the stable merge (U before V, lower index
//                 first: the walk's own order), then the tail of sot_backward_kernel (weight_grad_tail) -> grad_x, grad_y;
//   positions:    g_xs[i] = sum_{k : rank_U(Q_k) = i} gUq_k, g_ys[j] likewise, undone through the sort permutation -> grad_xpos, grad_ypos.
// ONE merge walk serves both: level k of thread t is merged element D0 + s, so each upstream row is read once, straight from global
// memory.  The rank of a level is the number of U (V) entries consumed when the RUN of equal levels it belongs to began (searchsorted is
// side='left'), hence non-decreasing in k: the levels of one position are consecutive.  Each thread sums its levels by position; a
// position that begins and ends inside the thread's segment is ASSIGNED to its slot, the thread's first and last sums are left as
// (slot, value) segment ends, and after a barrier the first of each run of equal end slots adds the run up in thread order: one writer
// per slot, no atomics, deterministic.  The position slots live in the PX | PY regions (the walk does not read support positions: the
// Jacobian of a gather is independent of the gathered values), the CDF slots in GU | GV as in sot_backward_kernel.
// ---------------------------------------------------------------------------------------------
struct QuantBwdArgs {
    FwdArgs f;
    const float* gUq; const float* gVq; const float* gQ;   // [B, n + m] dense, any may be null
    const float* gU; const float* gV;                      // [B, n] / [B, m] dense, either may be null
    float* gx; float* gy; float* gxp; float* gyp;          // [B, n] / [B, m] dense, any may be null
};

// one side's running sum over the levels of the position `cur`; `slot` is the position of the level at hand
struct PosRun {
    float acc, head; int cur, head_slot; bool flushed;
    __device__ __forceinline__ void step(float* slots, int slot, float g)
    {
        if (slot != cur) {
            if (cur >= 0) {
                if (flushed) slots[cur] = acc;                       // begins and ends inside this segment: nobody else has a term
                else { head = acc; head_slot = cur; flushed = true; }
            }
            cur = slot; acc = 0.0f;
        }
        acc += g;
    }
};

template <int G, int CPT, bool ROWPOS>
__global__ __launch_bounds__((G < 256 ? 256 : G)) void sot_quantiles_backward_kernel(const QuantBwdArgs b)
{
    constexpr int BLOCK = (G < 256 ? 256 : G);
    constexpr int RPW = BLOCK / G;
    constexpr int NW = G / kWave;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FwdArgs& a = b.f;
    const RowCtx<G> c = make_ctx<G, ROWPOS>(a, smem, true);
    const int rg = threadIdx.x / G;
    const int n = c.n, m = c.m, t = c.t, K = c.K;
    float* const U = c.U; float* const V = c.V;
    float* const SX = c.PX; float* const SY = c.PY;   // position slots (the supports themselves are never read here)
    const bool do_w = b.gx != nullptr || b.gy != nullptr;
    const bool do_p = b.gxp != nullptr || b.gyp != nullptr;
    // the two segment ends (value, slot) x 2 sides of the Ga walking threads: in the row's own U | V regions when they are large enough (the
    // CDFs are dead once every thread has finished its walk), otherwise behind the row regions (run_quantiles_backward sizes the LDS)
    const int NE = 2 * c.Ga;
    const bool ends_in_cdfs = 4 * NE <= c.L.poff - c.L.padcap;   // the U | V regions as laid out (per-row positions: the sort image's size)
    float* const end_x = ends_in_cdfs ? U : smem + RPW * c.L.row_floats + rg * 8 * G;
    int* const end_i = reinterpret_cast<int*>(end_x + NE);
    float* const end_y = end_x + 2 * NE;
    int* const end_j = reinterpret_cast<int*>(end_x + 3 * NE);

    const int64_t row_step = (int64_t)gridDim.x * RPW;
    int64_t row0 = (int64_t)blockIdx.x * RPW;
    float rx[CPT], ry[CPT];
    if (row0 < a.B) {
        const int64_t r = min(row0 + rg, a.B - 1);
        load_row<G, CPT, false>(a.x + r * a.xs, n, t, rx);
        load_row<G, CPT, false>(a.y + r * a.ys, m, t, ry);
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
        store_row<G, CPT, false>(U, n, t, rx);
        store_row<G, CPT, false>(V, m, t, ry);
        if (row0 + row_step < a.B) {
            const int64_t r = min(row0 + row_step + rg, a.B - 1);
            load_row<G, CPT, false>(a.x + r * a.xs, n, t, rx);
            load_row<G, CPT, false>(a.y + r * a.ys, m, t, ry);
        }
        row_sync<NW>();
        if (do_p) {   // (behind the barrier: rowpos_prepare's last reads of PX are done; build_cdfs ends with the barrier in front of the walk)
            for (int e = t; e < n; e += G) SX[e] = 0.0f;
            for (int e = t; e < m; e += G) SY[e] = 0.0f;
        }
        float wx[CPT], wy[CPT];
        float Sx, Sy;
        build_cdfs<G, CPT, ROWPOS>(a, c, ix, iy, wx, wy, Sx, Sy);

        PosRun px{0.0f, 0.0f, -1, -1, false}, py{0.0f, 0.0f, -1, -1, false};
        if (t < c.Ga) {
            const float* const Uw = U - c.pad;
            const int nw = n + c.pad;
            const int D0 = t * c.E;
            const uint32_t ub1 = lds_addr(Uw) - 4u;
            const int i0 = (int)((merge_path_steps32(ub1, lds_addr(V) + 4u * (uint32_t)D0 + ub1, nw, m, D0, c.topk) - ub1) >> 2);
            const int j0 = D0 - i0;
            float qprev = 0.0f;
            if (i0 > 0) qprev = Uw[i0 - 1];
            if (j0 > 0) qprev = fmaxf(qprev, V[j0 - 1]);
            float ua = Uw[i0], vb = V[j0];
            int ru = 0, rv = 0;   // searchsorted ranks of the run of equal levels that is open (U: before the clamp at 0 that removes the pads)
            if (D0 == 0) {
                qprev = __int_as_float(0x7fc00000);  // NaN: the very first level always starts a run
            } else if (fminf(ua, vb) == qprev) {      // we start inside a run: the ranks of its first member
                ru = lower_rank(U, n, qprev);
                rv = lower_rank(V, m, qprev);
            }
            char* const lb = reinterpret_cast<char*>(const_cast<float*>(Uw));
            const uint32_t goff4 = 4u * (uint32_t)c.L.grad;
            const int voff = (int)(V - Uw);
            uint32_t iu = (uint32_t)i0;
            const int64_t kb = rowc * (int64_t)K - c.pad;   // level k of this row = merged element D0 + s - pad (the pads have no upstream)
            for (int s = 0; s < c.E; ++s) {
                const bool tu = ua <= vb;   // canonical stable order: U before V on ties
                const float q = tu ? ua : vb;
                const bool new_run = !(q == qprev);
                qprev = q;
                const bool real = D0 + s >= c.pad;
                const int64_t o = kb + D0 + s;
                const uint32_t vk = (uint32_t)(voff + D0 + s);
                const uint32_t off = 4u * (tu ? iu : (vk - iu));   // slot of the element consumed now
                if (do_w) *reinterpret_cast<float*>(lb + off + goff4) = (real && b.gQ) ? b.gQ[o] : 0.0f;
                if (do_p) {
                    ru = new_run ? (int)iu - c.pad : ru;
                    rv = new_run ? D0 + s - (int)iu : rv;
                    px.step(SX, min(max(ru, 0), n - 1), (real && b.gUq) ? b.gUq[o] : 0.0f);   // clamp of losses.py:220
                    py.step(SY, min(rv, m - 1), (real && b.gVq) ? b.gVq[o] : 0.0f);
                }
                iu += tu ? 1u : 0u;
                const float nv = *reinterpret_cast<const float*>(lb + off + 4u);
                ua = tu ? nv : ua;
                vb = tu ? vb : nv;
            }
        }
        row_sync<NW>();   // every walk is done: GU / GV are complete, the CDFs may be overwritten by the segment ends

        if (do_p) {
            if (t < c.Ga) {   // a segment of one position has no head of its own: an empty one on the tail's slot keeps equal slots adjacent
                end_x[2 * t] = px.flushed ? px.head : 0.0f; end_i[2 * t] = px.flushed ? px.head_slot : px.cur;
                end_x[2 * t + 1] = px.acc;                  end_i[2 * t + 1] = px.cur;
                end_y[2 * t] = py.flushed ? py.head : 0.0f; end_j[2 * t] = py.flushed ? py.head_slot : py.cur;
                end_y[2 * t + 1] = py.acc;                  end_j[2 * t + 1] = py.cur;
            }
            row_sync<NW>();
            if (t < c.Ga) {
                for (int e = 2 * t; e < 2 * t + 2; ++e) {
                    const int si = end_i[e];
                    if (e == 0 || end_i[e - 1] != si) {   // first of a run of equal slots: one writer per slot
                        float sum = end_x[e];
                        for (int u = e + 1; u < NE && end_i[u] == si; ++u) sum += end_x[u];
                        SX[si] += sum;
                    }
                    const int sj = end_j[e];
                    if (e == 0 || end_j[e - 1] != sj) {
                        float sum = end_y[e];
                        for (int u = e + 1; u < NE && end_j[u] == sj; ++u) sum += end_y[u];
                        SY[sj] += sum;
                    }
                }
            }
            row_sync<NW>();
            if (valid) {
                const bool x_perm = ROWPOS ? c.do_sort : !c.x_ident;
                const bool y_perm = ROWPOS ? c.do_sort : !c.y_ident;
                const int e0 = t * CPT;
                if (b.gxp) {
                    float* dst = b.gxp + row * (int64_t)n;
#pragma unroll
                    for (int k = 0; k < CPT; ++k) {
                        const int e = e0 + k;
                        if (e < n) dst[ROWPOS ? (x_perm ? ix[k] : e) : (x_perm ? a.xperm[e] : e)] = SX[e];
                    }
                }
                if (b.gyp) {
                    float* dst = b.gyp + row * (int64_t)m;
#pragma unroll
                    for (int k = 0; k < CPT; ++k) {
                        const int e = e0 + k;
                        if (e < m) dst[ROWPOS ? (y_perm ? iy[k] : e) : (y_perm ? a.yperm[e] : e)] = SY[e];
                    }
                }
            }
        }
        if (do_w)
            weight_grad_tail<G, CPT, ROWPOS, false, true>(a, c, ix, iy, wx, wy, Sx, Sy, nullptr, 0, 1.0f, b.gx, b.gy, row, rowc, valid,
                                                          b.gU ? b.gU + rowc * (int64_t)n : nullptr, b.gV ? b.gV + rowc * (int64_t)m : nullptr);
        if (t == 0) { U[n] = INFINITY; V[m] = INFINITY; }   // the sentinels (make_ctx sets them once) may lie under the segment ends
        row_sync<NW>();   // slot reads done before the next row reuses LDS
    }
}

template <int G, int CPT, bool ROWPOS>
static hipError_t launch_quantiles_backward(const QuantBwdArgs& b, size_t lds, int64_t want, int block, hipStream_t s)
{
    return launch_persistent<sot_quantiles_backward_kernel<G, CPT, ROWPOS>>(b, lds, want, block, s);
}

template <bool ROWPOS>
static hipError_t dispatch_quantiles_backward(const LaunchCfg& c, const QuantBwdArgs& b, size_t lds, int64_t want, int block, hipStream_t s)
{
    if (c.CPT == 16) return launch_quantiles_backward<1024, 16, ROWPOS>(b, lds, want, block, s);
    switch (c.G) {
        case 64: return launch_quantiles_backward<64, 8, ROWPOS>(b, lds, want, block, s);
        case 128: return launch_quantiles_backward<128, 12, ROWPOS>(b, lds, want, block, s);
        case 256: return launch_quantiles_backward<256, 8, ROWPOS>(b, lds, want, block, s);
        default: return launch_quantiles_backward<1024, 8, ROWPOS>(b, lds, want, block, s);
    }
}

int run_quantiles_backward(const sot_problem* pr, const float* gUq, const float* gVq, const float* gQ, const float* gU, const float* gV,
                           float* gx, float* gy, float* gxp, float* gyp, void* workspace, size_t workspace_bytes, void* stream)
{
    int rc = validate(pr);
    if (rc != SOT_OK) return rc;
    if (pr->B == 0 || (gx == nullptr && gy == nullptr && gxp == nullptr && gyp == nullptr)) return SOT_OK;
    // the LDS budget is checked BEFORE setup_launch, which may enqueue the position plan or the per-row pre-sort
    LaunchCfg cfg; size_t lds = 0; int block = 0, rpw = 1;
    if (!pick_cfg(pr->n, pr->m, pr->xpos_row_stride != 0, true, &cfg, &lds, &block, &rpw)) return SOT_ERR_UNSUPPORTED_SIZE;
    // the segment ends: behind the row regions unless the rows are long enough to hold them in their dead CDFs (see the kernel)
    const int E = merge_steps(pr->n + pr->m, cfg.G), Ga = (pr->n + pr->m + E - 1) / E;
    const RowLayout L = make_layout(pr->n, pr->m, cfg.G, pr->xpos_row_stride != 0, true);
    if (8 * Ga > L.poff - L.padcap) lds += 8 * sizeof(float) * (size_t)block;
    if (lds > kLdsLimit) return SOT_ERR_UNSUPPORTED_SIZE;
    Launch l;
    rc = setup_launch(pr, true, workspace, workspace_bytes, stream, &l);
    if (rc != SOT_OK) return rc;
    QuantBwdArgs b{};
    b.f = l.a; b.gUq = gUq; b.gVq = gVq; b.gQ = gQ; b.gU = gU; b.gV = gV; b.gx = gx; b.gy = gy; b.gxp = gxp; b.gyp = gyp;
    const hipError_t e = l.rowpos ? dispatch_quantiles_backward<true>(l.cfg, b, lds, l.want, l.block, l.s)
                                  : dispatch_quantiles_backward<false>(l.cfg, b, lds, l.want, l.block, l.s);
    return launch_status(e);
}

}  // namespace sot
