// sot_f64.hip -- the row pipeline in double precision (include/sot_hip.h: sot_w1d_*_f64, ABI 21): float64 weights and float64 positions,
// float64 row losses and gradients.  ONE generic kernel family, written in `double` from SURVEY.md A.1 / A.2 / A.4; nothing of the float32
// kernels is instantiated here (they carry the float32 emulation of ATen's summation order and packed-fp32 arithmetic, which have no double
// form).  The reference in float64 is plain ATen on double tensors; this file evaluates the same quantities with sums in a fixed order of
// its own (thread chunk, wavefront, the workgroup's four wavefronts in order), so a result depends neither on the grid nor on a row's place
// in the batch.
//
// One 256-thread workgroup per row pair, persistent over the batch.  Per row:
//   1. the two weight rows are staged into LDS with coalesced 8-byte loads (16-byte where the row starts on a 16-byte boundary), squared on the
//      way for square_dist; shared positions are staged once per workgroup, per-row positions with every row;
//   2. row masses: every thread sums its contiguous chunk, wave_sum, the four wave sums in order; the guard of utils.py:135-142 (a mass
//      <= 1e-7 becomes the float32 1e-7 widened to double); IEEE division;
//   3. inclusive scan: thread-serial over the chunk, wave_incl_scan(double) over the chunk totals, the wave offsets in order;
//   4. merge-path partition of the n + m levels (U before V on ties: the order of a stable sort of cat(U, V)); every thread walks its own
//      segment and accumulates delta_k |uq_k - vq_k|^p; levels above 1 contribute nothing under the cutoff;
//   5. wave_sum and the four wave sums in order.
// Backward: the same CDFs, then g_k = m_k d_k - m_{k+1} d_{k+1} per level, un-merged into a slot per CDF entry; suffix sums
// (thread chunk, wave_suffix_incl_scan(double), later waves in order); normalisation terms, the 2x of square_dist, the row's upstream
// gradient times grad_scale.  TIE ORDER: at exactly tied levels the kernel follows the float32 backward kernels (sot_rows.hpp:
// sot_backward_kernel, sot_full_bwd.hpp) -- searchsorted ranks are constant along a run of equal levels, so g is non-zero only at the run's
// LAST member in the stable order (U before V, lower index first), which receives d(run) - d(next run).
//
// Supports must arrive sorted (positions non-decreasing along a row): a call with SOT_FLAG_REQUIRE_SORT is refused; the Python layer sorts.
#include "sot_host.hpp"
#include "sot_device.hpp"

namespace sot {

constexpr int kF64Block = 256;
constexpr int kF64Waves = kF64Block / kWave;
constexpr int kF64Red = 40;   // doubles of reduction scratch in front of the row arrays (nine groups of kF64Waves, see F64Red)

// reduction scratch: one group of kF64Waves doubles per fixed-order sum
enum F64Red { kRedMassX = 0, kRedMassY = 4, kRedScanU = 8, kRedScanV = 12, kRedLoss = 16, kRedSufU = 20, kRedSufV = 24, kRedDotX = 28, kRedDotY = 32 };

struct F64Args {
    const double* x; const double* y; const double* xpos; const double* ypos;
    int64_t B, xs, ys, xps, yps;
    int n, m;
    double p;
    uint32_t flags;
    double* row_loss;            // forward
    const double* grad_row;      // backward: [B] (stride 1), one broadcast element (stride 0) or null = 1 for every row
    int64_t grad_row_stride;
    double grad_scale;
    double* gx; double* gy;      // dense [B, n] / [B, m], or null
};

// arrays start on 16-byte boundaries: lengths are rounded up to an even number of doubles
__host__ __device__ static inline int f64_even(int n) { return n + (n & 1); }
static inline size_t f64_lds_bytes(int n, int m, bool backward)
{
    return sizeof(double) * ((size_t)kF64Red + (size_t)(backward ? 3 : 2) * ((size_t)f64_even(n) + (size_t)f64_even(m)));
}

struct F64Row {
    double* red; double* U; double* V; double* PX; double* PY; double* GU; double* GV;
};
__device__ __forceinline__ F64Row f64_layout(double* smem, int n, int m, bool backward)
{
    const int ne = f64_even(n), me = f64_even(m);
    F64Row r;
    r.red = smem;
    r.U = smem + kF64Red;
    r.V = r.U + ne;
    r.PX = r.V + me;
    r.PY = r.PX + ne;
    r.GU = backward ? r.PY + me : nullptr;
    r.GV = backward ? r.GU + ne : nullptr;
    return r;
}

// src[0, n) -> dst[0, n) (LDS, 16-byte aligned), squared on the way when sq: coalesced, 16-byte loads where src allows
__device__ __forceinline__ void f64_stage(const double* src, int n, double* dst, bool sq, int t)
{
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        const int n2 = n >> 1;
        for (int i = t; i < n2; i += kF64Block) {
            double2 v = reinterpret_cast<const double2*>(src)[i];
            if (sq) { v.x *= v.x; v.y *= v.y; }
            reinterpret_cast<double2*>(dst)[i] = v;
        }
        if ((n & 1) && t == 0) { const double w = src[n - 1]; dst[n - 1] = sq ? w * w : w; }
    } else {
        for (int i = t; i < n; i += kF64Block) { const double w = src[i]; dst[i] = sq ? w * w : w; }
    }
}

// the four wave values of one group, in order
__device__ __forceinline__ double f64_fold(const double* red)
{
    double s = red[0];
#pragma unroll
    for (int w = 1; w < kF64Waves; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ double f64_guard(double s) { return (s <= 1e-7) ? (double)kMassEps : s; }

template <int PM>
__device__ __forceinline__ double f64_cost(double xa, double yb, double p)
{
    const double d = fabs(xa - yb);
    if (PM == 1) return d;
    if (PM == 2) return d * d;
    return pow(d, p);
}

// #{A[i] < q}, A non-decreasing of length n
__device__ __forceinline__ int f64_lower_rank(const double* A, int n, double q)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A[mid] < q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Steps 1 - 3 for one row pair: on return (a barrier has been passed) r.U / r.V hold the CDFs; Sx / Sy the row masses before the guard, dx / dy
// the divisors (1 for weights used as given).  stage_pos: the positions are staged with this row.
__device__ __forceinline__ void f64_build_cdfs(const F64Args& a, const F64Row& r, int64_t row, bool stage_pos, int t, double& Sx, double& Sy,
                                               double& dx, double& dy)
{
    const int n = a.n, m = a.m;
    const bool prenorm = a.flags & SOT_FLAG_PRENORMALIZED;
    const bool sq = !prenorm && (a.flags & SOT_FLAG_SQUARE);
    const bool dn = !prenorm && (a.flags & SOT_FLAG_DONT_NORMALIZE);
    const int lane = t & (kWave - 1), wv = t >> 6;
    f64_stage(a.x + row * a.xs, n, r.U, sq, t);
    f64_stage(a.y + row * a.ys, m, r.V, sq, t);
    if (stage_pos) {
        f64_stage(a.xpos + row * a.xps, n, r.PX, false, t);
        f64_stage(a.ypos + row * a.yps, m, r.PY, false, t);
    }
    __syncthreads();
    const int cx = (n + kF64Block - 1) / kF64Block, cy = (m + kF64Block - 1) / kF64Block;
    const int bx = min(t * cx, n), ex = min(bx + cx, n), by = min(t * cy, m), ey = min(by + cy, m);
    // row masses
    double sx = 0.0, sy = 0.0;
    for (int i = bx; i < ex; ++i) sx += r.U[i];
    for (int j = by; j < ey; ++j) sy += r.V[j];
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    if (lane == 0) { r.red[kRedMassX + wv] = sx; r.red[kRedMassY + wv] = sy; }
    __syncthreads();
    Sx = f64_fold(r.red + kRedMassX);
    Sy = f64_fold(r.red + kRedMassY);
    dx = prenorm ? 1.0 : f64_guard(Sx);
    dy = prenorm ? 1.0 : (dn ? dx : f64_guard(Sy));
    // inclusive scan of the quotients
    double ru = 0.0, rv = 0.0;
    for (int i = bx; i < ex; ++i) { ru += prenorm ? r.U[i] : r.U[i] / dx; r.U[i] = ru; }
    for (int j = by; j < ey; ++j) { rv += prenorm ? r.V[j] : r.V[j] / dy; r.V[j] = rv; }
    const double iu = wave_incl_scan(ru), iv = wave_incl_scan(rv);
    double ou = wave_shift_right1(iu), ov = wave_shift_right1(iv);   // exclusive over the lanes: lane 0 gets 0
    if (lane == kWave - 1) { r.red[kRedScanU + wv] = iu; r.red[kRedScanV + wv] = iv; }
    __syncthreads();
    double wu = 0.0, wvv = 0.0;
    for (int w = 0; w < wv; ++w) { wu += r.red[kRedScanU + w]; wvv += r.red[kRedScanV + w]; }
    ou += wu;
    ov += wvv;
    for (int i = bx; i < ex; ++i) r.U[i] += ou;
    for (int j = by; j < ey; ++j) r.V[j] += ov;
    __syncthreads();
}

// number of U entries among the first D merged levels, U before V on ties
__device__ __forceinline__ int f64_merge_path(const double* U, const double* V, int n, int m, int D)
{
    int lo = max(0, D - m), hi = min(D, n);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (U[mid] <= V[D - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <int PM>
__global__ __launch_bounds__(kF64Block) void sot_f64_forward_kernel(const F64Args a)
{
    extern __shared__ __attribute__((aligned(16))) double smem64[];
    const int n = a.n, m = a.m, K = n + m, t = threadIdx.x;
    const int lane = t & (kWave - 1), wv = t >> 6;
    const F64Row r = f64_layout(smem64, n, m, false);
    const bool lim = a.flags & SOT_FLAG_LIMIT_Q;
    const bool shared_pos = a.xps == 0;
    if (shared_pos && (int64_t)blockIdx.x < a.B) {   // (the first row's barrier covers these)
        f64_stage(a.xpos, n, r.PX, false, t);
        f64_stage(a.ypos, m, r.PY, false, t);
    }
    const int E = (K + kF64Block - 1) / kF64Block;
    for (int64_t row = blockIdx.x; row < a.B; row += gridDim.x) {
        double Sx, Sy, dx, dy;
        f64_build_cdfs(a, r, row, !shared_pos, t, Sx, Sy, dx, dy);
        double acc = 0.0;
        const int D0 = t * E, D1 = min(D0 + E, K);
        if (D0 < K) {
            int i = f64_merge_path(r.U, r.V, n, m, D0);
            int j = D0 - i;
            double qprev = 0.0;   // Q_0 := 0
            if (i > 0) qprev = r.U[i - 1];
            if (j > 0) qprev = fmax(qprev, r.V[j - 1]);
            for (int s = D0; s < D1; ++s) {
                const bool tu = (i < n) && (j >= m || r.U[i] <= r.V[j]);
                const double q = tu ? r.U[i] : r.V[j];
                const double cost = f64_cost<PM>(r.PX[min(i, n - 1)], r.PY[min(j, m - 1)], a.p);
                double delta = q - qprev;
                if (lim && q > 1.0) delta = 0.0;
                acc += delta * cost;
                qprev = q;
                i += tu ? 1 : 0;
                j += tu ? 0 : 1;
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) r.red[kRedLoss + wv] = acc;
        __syncthreads();
        if (t == 0) a.row_loss[row] = f64_fold(r.red + kRedLoss);
        __syncthreads();   // this row's LDS reads are done before the next row is staged
    }
}

// one side of the backward's tail: suffix sums of the slots G (in place), thread chunk -> wavefront -> later waves in order
__device__ __forceinline__ void f64_suffix_local(double* G, int b, int e, double& tot)
{
    double run = 0.0;
    for (int i = e - 1; i >= b; --i) { run += G[i]; G[i] = run; }
    tot = run;
}

template <int PM>
__global__ __launch_bounds__(kF64Block) void sot_f64_backward_kernel(const F64Args a)
{
    extern __shared__ __attribute__((aligned(16))) double smem64[];
    const int n = a.n, m = a.m, K = n + m, t = threadIdx.x;
    const int lane = t & (kWave - 1), wv = t >> 6;
    const F64Row r = f64_layout(smem64, n, m, true);
    const bool prenorm = a.flags & SOT_FLAG_PRENORMALIZED;
    const bool sq = !prenorm && (a.flags & SOT_FLAG_SQUARE);
    const bool dn = !prenorm && (a.flags & SOT_FLAG_DONT_NORMALIZE);
    const bool lim = a.flags & SOT_FLAG_LIMIT_Q;
    const bool shared_pos = a.xps == 0;
    const bool side_x = a.gx != nullptr;                      // suffix sums of the x side
    const bool side_y = a.gy != nullptr || (side_x && dn);    // ... of the y side (dont_normalize: its dot product enters d / d S_x)
    if (shared_pos && (int64_t)blockIdx.x < a.B) {
        f64_stage(a.xpos, n, r.PX, false, t);
        f64_stage(a.ypos, m, r.PY, false, t);
    }
    const int E = (K + kF64Block - 1) / kF64Block;
    const int cx = (n + kF64Block - 1) / kF64Block, cy = (m + kF64Block - 1) / kF64Block;
    const int bx = min(t * cx, n), ex = min(bx + cx, n), by = min(t * cy, m), ey = min(by + cy, m);
    for (int64_t row = blockIdx.x; row < a.B; row += gridDim.x) {
        double Sx, Sy, dx, dy;
        f64_build_cdfs(a, r, row, !shared_pos, t, Sx, Sy, dx, dy);
        // ---- g_k per level, un-merged: the gradient of a level is known one level later (it is non-zero only if the NEXT level starts a
        //      new run), so the slot of level k - 1 is written at level k; the segment's last level is closed by a look at level D1.
        const int D0 = t * E, D1 = min(D0 + E, K);
        if (D0 < K) {
            int i = f64_merge_path(r.U, r.V, n, m, D0);
            int j = D0 - i;
            double qprev = __longlong_as_double(0x7ff8000000000000ll);   // NaN: the very first level always starts a run
            double dcur = 0.0;                                           // m_k d_k of the current run
            if (D0 > 0) {
                qprev = 0.0;
                if (i > 0) qprev = r.U[i - 1];
                if (j > 0) qprev = fmax(qprev, r.V[j - 1]);
                const bool tu0 = (i < n) && (j >= m || r.U[i] <= r.V[j]);
                const double q0 = tu0 ? r.U[i] : r.V[j];
                if (q0 == qprev) {   // the segment starts inside a run: the cost at the ranks of the run's first member
                    const int iu = f64_lower_rank(r.U, n, q0), iv = f64_lower_rank(r.V, m, q0);
                    dcur = (lim && q0 > 1.0) ? 0.0 : f64_cost<PM>(r.PX[min(iu, n - 1)], r.PY[min(iv, m - 1)], a.p);
                }
            }
            double* pend = nullptr;
            for (int s = D0; s < D1; ++s) {
                const bool tu = (i < n) && (j >= m || r.U[i] <= r.V[j]);
                const double q = tu ? r.U[i] : r.V[j];
                const bool newrun = !(q == qprev);
                double dnew = dcur;
                if (newrun) dnew = (lim && q > 1.0) ? 0.0 : f64_cost<PM>(r.PX[min(i, n - 1)], r.PY[min(j, m - 1)], a.p);
                if (pend != nullptr) *pend = newrun ? dcur - dnew : 0.0;
                dcur = dnew;
                pend = tu ? r.GU + i : r.GV + j;
                qprev = q;
                i += tu ? 1 : 0;
                j += tu ? 0 : 1;
            }
            if (D1 == K) {
                *pend = dcur;   // m_{K+1} d_{K+1} := 0
            } else {
                const bool tu = (i < n) && (j >= m || r.U[i] <= r.V[j]);
                const double q = tu ? r.U[i] : r.V[j];
                double g = 0.0;
                if (!(q == qprev)) g = dcur - ((lim && q > 1.0) ? 0.0 : f64_cost<PM>(r.PX[min(i, n - 1)], r.PY[min(j, m - 1)], a.p));
                *pend = g;
            }
        }
        __syncthreads();
        // ---- suffix sums ga_i, gb_j
        double tx = 0.0, ty = 0.0;
        if (side_x) f64_suffix_local(r.GU, bx, ex, tx);
        if (side_y) f64_suffix_local(r.GV, by, ey, ty);
        const double sfx = wave_suffix_incl_scan(tx), sfy = wave_suffix_incl_scan(ty);
        double ox = __shfl_down(sfx, 1), oy = __shfl_down(sfy, 1);   // exclusive over the later lanes
        if (lane == kWave - 1) { ox = 0.0; oy = 0.0; }
        if (lane == 0) { r.red[kRedSufU + wv] = sfx; r.red[kRedSufV + wv] = sfy; }
        __syncthreads();
        double lx = 0.0, ly = 0.0;
        for (int w = kF64Waves - 1; w > wv; --w) { lx += r.red[kRedSufU + w]; ly += r.red[kRedSufV + w]; }
        ox += lx;
        oy += ly;
        if (side_x) for (int i = bx; i < ex; ++i) r.GU[i] += ox;
        if (side_y) for (int j = by; j < ey; ++j) r.GV[j] += oy;
        __syncthreads();
        // ---- dot products sum ga_i w_i (w: the weight as staged, squared under square_dist) for the normalisation terms
        const double* const xrow = a.x + row * a.xs;
        const double* const yrow = a.y + row * a.ys;
        double gSx = 0.0, gSy = 0.0;
        if (!prenorm) {
            double dotx = 0.0, doty = 0.0;
            if (side_x) for (int i = t; i < n; i += kF64Block) { const double w = xrow[i]; dotx += r.GU[i] * (sq ? w * w : w); }
            if (side_y) for (int j = t; j < m; j += kF64Block) { const double w = yrow[j]; doty += r.GV[j] * (sq ? w * w : w); }
            dotx = wave_sum(dotx);
            doty = wave_sum(doty);
            if (lane == 0) { r.red[kRedDotX + wv] = dotx; r.red[kRedDotY + wv] = doty; }
            __syncthreads();
            gSx = -f64_fold(r.red + kRedDotX);
            gSy = -f64_fold(r.red + kRedDotY);
            if (dn) { gSx += gSy; gSy = 0.0; }
            gSx = (Sx > 1e-7) ? gSx / (dx * dx) : 0.0;
            gSy = (Sy > 1e-7) ? gSy / (dy * dy) : 0.0;
        }
        const double gr = (a.grad_row ? a.grad_row[row * a.grad_row_stride] : 1.0) * a.grad_scale;
        if (a.gx) {
            double* const dst = a.gx + row * (int64_t)n;
            for (int i = t; i < n; i += kF64Block) {
                double g = r.GU[i] / dx + gSx;
                if (sq) g *= 2.0 * xrow[i];
                dst[i] = g * gr;
            }
        }
        if (a.gy) {
            double* const dst = a.gy + row * (int64_t)m;
            for (int j = t; j < m; j += kF64Block) {
                double g = r.GV[j] / dy + gSy;
                if (sq) g *= 2.0 * yrow[j];
                dst[j] = g * gr;
            }
        }
        __syncthreads();   // this row's LDS reads are done before the next row is staged
    }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
static inline int f64_validate(const sot_problem_f64* pr)
{
    if (pr == nullptr) return SOT_ERR_NULL_POINTER;
    if (!(pr->p >= 1.0)) return SOT_ERR_INVALID_P;
    if (pr->B < 0 || pr->n < 1 || pr->m < 1) return SOT_ERR_BAD_SHAPE;
    if (pr->x_row_stride < pr->n || pr->y_row_stride < pr->m) return SOT_ERR_BAD_SHAPE;
    if (pr->xpos_row_stride != 0 && pr->xpos_row_stride < pr->n) return SOT_ERR_BAD_SHAPE;
    if (pr->ypos_row_stride != 0 && pr->ypos_row_stride < pr->m) return SOT_ERR_BAD_SHAPE;
    if ((pr->xpos_row_stride == 0) != (pr->ypos_row_stride == 0)) return SOT_ERR_BAD_SHAPE;
    if (pr->flags & SOT_FLAG_REQUIRE_SORT) return SOT_ERR_BAD_SHAPE;   // supports arrive sorted
    if ((int64_t)pr->n + (int64_t)pr->m > (1 << 20) || f64_lds_bytes(pr->n, pr->m, false) > kLdsLimit) return SOT_ERR_UNSUPPORTED_SIZE;
    return SOT_OK;
}

static inline int f64_check_call(const sot_problem_f64* pr, bool backward, const void* workspace, size_t workspace_bytes)
{
    const int rc = f64_validate(pr);
    if (rc != SOT_OK) return rc;
    if (backward && f64_lds_bytes(pr->n, pr->m, true) > kLdsLimit) return SOT_ERR_UNSUPPORTED_SIZE;
    if (workspace_bytes < sot_w1d_f64_workspace_bytes(pr)) return SOT_ERR_WORKSPACE;
    if (workspace == nullptr && workspace_bytes > 0) return SOT_ERR_NULL_POINTER;
    if (pr->B > 0 && (!pr->x || !pr->y || !pr->xpos || !pr->ypos)) return SOT_ERR_NULL_POINTER;
    return SOT_OK;
}

static inline F64Args f64_args(const sot_problem_f64* pr)
{
    F64Args a{};
    a.x = pr->x; a.y = pr->y; a.xpos = pr->xpos; a.ypos = pr->ypos;
    a.B = pr->B; a.n = pr->n; a.m = pr->m;
    a.xs = pr->x_row_stride; a.ys = pr->y_row_stride; a.xps = pr->xpos_row_stride; a.yps = pr->ypos_row_stride;
    a.p = pr->p; a.flags = pr->flags;
    return a;
}

static inline int f64_pm(double p) { return p == 1.0 ? 1 : (p == 2.0 ? 2 : 0); }

}  // namespace sot

using namespace sot;

extern "C" {

size_t sot_w1d_f64_workspace_bytes(const sot_problem_f64* prob)
{
    (void)prob;
    return 0;   // a row pair's whole working set lives in LDS
}

int sot_w1d_f64_supported(const sot_problem_f64* prob, int backward)
{
    if (f64_validate(prob) != SOT_OK) return 0;
    return f64_lds_bytes(prob->n, prob->m, backward != 0) <= kLdsLimit ? 1 : 0;
}

int sot_w1d_forward_f64(const sot_problem_f64* prob, double* row_loss, void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = f64_check_call(prob, false, workspace, workspace_bytes);
    if (rc != SOT_OK) return rc;
    if (prob->B == 0) return SOT_OK;
    if (row_loss == nullptr) return SOT_ERR_NULL_POINTER;
    F64Args a = f64_args(prob);
    a.row_loss = row_loss;
    const size_t lds = f64_lds_bytes(a.n, a.m, false);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    switch (f64_pm(a.p)) {
        case 1: e = launch_persistent<sot_f64_forward_kernel<1>>(a, lds, a.B, kF64Block, s); break;
        case 2: e = launch_persistent<sot_f64_forward_kernel<2>>(a, lds, a.B, kF64Block, s); break;
        default: e = launch_persistent<sot_f64_forward_kernel<0>>(a, lds, a.B, kF64Block, s); break;
    }
    return launch_status(e);
}

int sot_w1d_backward_f64(const sot_problem_f64* prob, const double* grad_row, int64_t grad_row_stride, double grad_scale, double* grad_x,
                         double* grad_y, void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = f64_check_call(prob, true, workspace, workspace_bytes);
    if (rc != SOT_OK) return rc;
    if (grad_row_stride != 0 && grad_row_stride != 1) return SOT_ERR_BAD_SHAPE;
    if (prob->B == 0 || (grad_x == nullptr && grad_y == nullptr)) return SOT_OK;
    F64Args a = f64_args(prob);
    a.grad_row = grad_row; a.grad_row_stride = grad_row_stride; a.grad_scale = grad_scale;
    a.gx = grad_x; a.gy = grad_y;
    const size_t lds = f64_lds_bytes(a.n, a.m, true);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    switch (f64_pm(a.p)) {
        case 1: e = launch_persistent<sot_f64_backward_kernel<1>>(a, lds, a.B, kF64Block, s); break;
        case 2: e = launch_persistent<sot_f64_backward_kernel<2>>(a, lds, a.B, kF64Block, s); break;
        default: e = launch_persistent<sot_f64_backward_kernel<0>>(a, lds, a.B, kF64Block, s); break;
    }
    return launch_status(e);
}

}  // extern "C"
