// sot_launch.hpp -- host side shared by the row-kernel objects, on top of the library's launch layer (sot_host.hpp): launch configuration
// (pick_cfg), argument validation, workspace layout, kernel-attached timing and the profiled launch of a persistent kernel, the switch from
// the run-time cost / cutoff / square_dist mode to template arguments (with_mode), and the declarations of what one object calls in another.
#pragma once
#include "sot_host.hpp"
#include "sot_rows.hpp"
#include <functional>

namespace sot {

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
struct LaunchCfg { int G, CPT; };

// Row-group geometries: (threads per row, contiguous elements per thread).  G*CPT >= max(n, m).
// (128,12) serves the paper's row lengths just above 1024 (n_fft 2048 -> 1025 bins): two rows per workgroup.
static inline bool pick_cfg(int n, int m, bool rowpos, bool with_grad, LaunchCfg* cfg, size_t* lds_bytes, int* block, int* rpw)
{
    const int N = n > m ? n : m;
    static const LaunchCfg table[] = {{64, 8}, {128, 12}, {256, 8}, {1024, 8}, {1024, 16}};
    for (int ci = 0; ci < 5; ++ci) {
        const LaunchCfg& c = table[ci];
        if ((int64_t)c.G * c.CPT < N) continue;
        const int blk = c.G < 256 ? 256 : c.G;
        const int r = blk / c.G;
        const RowLayout L = make_layout(n, m, c.G, rowpos, with_grad);
        const size_t bytes = (size_t)r * L.row_floats * sizeof(float);
        if (bytes > kLdsLimit) continue;
        *cfg = c; *lds_bytes = bytes; *block = blk; *rpw = r;
        return true;
    }
    return false;
}

static inline int validate(const sot_problem* pr)
{
    if (pr == nullptr) return SOT_ERR_NULL_POINTER;
    if (!(pr->p >= 1.0f)) return SOT_ERR_INVALID_P;
    if (pr->B < 0 || pr->n < 1 || pr->m < 1) return SOT_ERR_BAD_SHAPE;
    if (pr->x_row_stride < pr->n || pr->y_row_stride < pr->m) return SOT_ERR_BAD_SHAPE;
    if (pr->xpos_row_stride != 0 && pr->xpos_row_stride < pr->n) return SOT_ERR_BAD_SHAPE;
    if (pr->ypos_row_stride != 0 && pr->ypos_row_stride < pr->m) return SOT_ERR_BAD_SHAPE;
    if ((pr->xpos_row_stride == 0) != (pr->ypos_row_stride == 0)) return SOT_ERR_BAD_SHAPE;
    if (pr->B > 0 && (!pr->x || !pr->y || !pr->xpos || !pr->ypos)) return SOT_ERR_NULL_POINTER;
    return SOT_OK;
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the batch mean out of the row kernel's last workgroup (sot_w1d_loss, sot_w1d_loss_and_grad): the one place a MeanTail is filled
static inline MeanTail make_tail(uint32_t* counters, double denom, int apply_hinge, float hinge, float* mean_out, double* sum_out)
{
    MeanTail mt{};
    mt.counters = counters; mt.denom = denom; mt.apply_hinge = apply_hinge; mt.hinge = hinge; mt.mean_out = mean_out; mt.sum_out = sum_out;
    return mt;
}

struct WsLayout { size_t sx, sy, px, py, ident, total; };
// the permutation image of a per-row-position call (setup_launch: the pre-sort kernel's output when the caller passes no row_perm_out)
static inline size_t rowpos_perm_bytes(int64_t B, int n, int m) { return align_up((size_t)B * ((size_t)n + (size_t)m) * sizeof(uint16_t), 256); }
// The pre-sort kernel's domain: per-row positions that a call has to sort itself (no row_perm_in), rows of 2 ... 2048 points, kernels with the
// length at compile time allowed.  ONE predicate for setup_launch, which runs the pre-sort, and for sot_workspace_bytes, which reports room for
// its image only where it can run (mirrored in the binding's _native._needs_workspace).
static inline bool rowpos_presort_runs(const sot_problem* pr)
{
    return pr->xpos_row_stride != 0 && (pr->flags & SOT_FLAG_REQUIRE_SORT) && pr->row_perm_in == nullptr && pr->B > 0 && pr->n >= 2 && pr->m >= 2 &&
           pr->n <= 2048 && pr->m <= 2048 && !(pr->flags & SOT_FLAG_NO_SPECIALIZE);
}

static inline WsLayout ws_layout(int n, int m)
{
    WsLayout w;
    size_t o = 0;
    w.sx = o; o = align_up(o + sizeof(float) * (size_t)n, 256);
    w.sy = o; o = align_up(o + sizeof(float) * (size_t)m, 256);
    w.px = o; o = align_up(o + sizeof(int) * (size_t)n, 256);
    w.py = o; o = align_up(o + sizeof(int) * (size_t)m, 256);
    w.ident = o; o = align_up(o + 2 * sizeof(int), 256);
    w.total = o;
    return w;
}

// ---- kernel-attached timing (sot_profile_next_launch, include/sot_hip.h): when armed by the calling thread, the next launch of
// a full-row kernel goes through hipExtLaunchKernelGGL with a start / stop event pair of the library's ring, i.e. the events
// bracket the dispatch itself (what rocprofv3's kernel trace measures) instead of stream time around it.
bool profile_take(hipEvent_t* start, hipEvent_t* stop);

template <typename Kernel, typename Args>
static inline void launch_maybe_profiled(Kernel kern, int grid, int block, size_t lds, hipStream_t s, const Args& a)
{
    hipEvent_t e0, e1;
    if (profile_take(&e0, &e1)) hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), (uint32_t)lds, s, e0, e1, 0, a);
    else hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s, a);
}

// launch_persistent (sot_host.hpp) for the full-row kernels: the launch goes through launch_maybe_profiled, i.e. it consumes an armed
// sot_profile_next_launch.
// A workgroup's second and later rows are tested in tests/test_row_loop_gpu.py, on batches that force them; a new row kernel adds a line to its CASES.
// What a call may write and read (outputs, workspace, row gaps) is tested in tests/test_memory_contract_gpu.py; a new row kernel or entry point
// adds a line to that file's CASES too.
template <auto Kern, class Args>
static inline hipError_t launch_persistent_profiled(const Args& args, size_t lds, int64_t want, int block, hipStream_t s)
{
    static GridCache cache;
    const int grid = persistent_grid(want, cached_resident_grid(cache, Kern, block, lds));
    (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
    launch_maybe_profiled(Kern, grid, block, lds, s, args);
    return hipGetLastError();
}

// ---- run-time mode -> compile-time template arguments.  pm: 1 -> p == 1, 2 -> p == 2, 0 -> any other p >= 1 (powf in the walk;
// losses.py:313 takes any p at one speed, and so do the full-row kernels: round 2 sent such calls to the generic kernel, 4x slower at
// 8192 x 2048).  with_pm(pm, f) calls f(std::integral_constant<int, PM>{}); with_mode(pm, flags, f) calls f(Mode<PM, LIM, SQ>{}) with
// the quantile cutoff (SOT_FLAG_LIMIT_Q) and square_dist (SOT_FLAG_SQUARE) of `flags`: f is instantiated for all 3 / all 12 modes.
template <int PM_, bool LIM_, bool SQ_>
struct Mode { static constexpr int PM = PM_; static constexpr bool LIM = LIM_, SQ = SQ_; };

template <class F>
static inline hipError_t with_pm(int pm, F&& f)
{
    switch (pm) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 0>{});
    }
}

template <class F>
static inline hipError_t with_mode(int pm, uint32_t flags, F&& f)
{
    const bool lim = flags & SOT_FLAG_LIMIT_Q, sq = flags & SOT_FLAG_SQUARE;
    return with_pm(pm, [&](auto pmc) {
        constexpr int PM = decltype(pmc)::value;
        switch ((lim ? 2 : 0) | (sq ? 1 : 0)) {
            case 0: return f(Mode<PM, false, false>{});
            case 1: return f(Mode<PM, false, true>{});
            case 2: return f(Mode<PM, true, false>{});
            default: return f(Mode<PM, true, true>{});
        }
    });
}

// ---- cross-object host interface (the objects are linked into one shared library; each function names its defining file) ----
struct Launch {
    FwdArgs a;
    LaunchCfg cfg;
    size_t lds;
    int block;
    int64_t want;  // row groups' worth of workgroups
    bool rowpos, vec;
    int pm;        // cost specialisation: 1 -> p == 1, 2 -> p == 2, 0 -> general
    hipStream_t s;
};

// sot_fwd_shared.hip (ROWPOS = false), sot_fwd_rowpos.hip (true); sot_bwd_shared.hip, sot_bwd_rowpos.hip
template <bool ROWPOS>
hipError_t dispatch_forward(const LaunchCfg& c, bool quant, int pm, bool vec, const FwdArgs& a, size_t lds, int64_t want, int block,
                            hipStream_t s);
template <bool ROWPOS>
hipError_t dispatch_backward(const LaunchCfg& c, int pm, bool vec, const BwdArgs& b, size_t lds, int64_t want, int block,
                             hipStream_t s);
// sot_full_fwd.hip
hipError_t dispatch_forward_full(int pm, const FwdArgs& a, hipStream_t s);
hipError_t dispatch_forward_full_rowpos(int pm, const FwdArgs& a, hipStream_t s);   // per-row positions through handed-over permutations, 2048-point rows (round 6)
hipError_t dispatch_area_full(const FwdArgs& a, hipStream_t s);
bool forward_full_supports(int n, bool aligned16);
bool backward_full_supports(int n, bool aligned16);
int full_rt_capacity(int n);   // capacity of the compile-time geometry that takes a run-time row length n (0: none)
// sot_full_bwd.hip
hipError_t dispatch_backward_full(int pm, const BwdArgs& b, hipStream_t s);
hipError_t dispatch_backward_full_rowpos(int pm, const BwdArgs& b, hipStream_t s);   // per-row positions through handed-over permutations, 2048-point rows (round 6)
hipError_t dispatch_area_train(const BwdArgs& b, hipStream_t s);
bool area_train_supports(int n);
// The geometry tables of 512 / 1024 / 2048 / 4096 bins on shared positions, ONE per route family for every element type WT of the weight rows
// (the backward's gradient rows have the same type).  Defined in sot_full_fwd.hpp / sot_full_bwd.hpp; the three float32 switches above fall
// through to <float>, sot_bf16.hip (area, forward) and sot_bf16_bwd.hip (backward) instantiate <uint16_t>: a kernel is compiled into the
// object that instantiates its table.
template <class WT> hipError_t dispatch_area_full_pow2(const FwdArgs& a, hipStream_t s);
template <class WT> hipError_t dispatch_forward_full_pow2(int pm, const FwdArgs& a, hipStream_t s);
template <class WT> hipError_t dispatch_backward_full_pow2(int pm, const BwdArgs& b, hipStream_t s);
// sot_full_rt_fwd.hip, sot_full_rt_bwd.hip
hipError_t dispatch_forward_full_rt(int pm, const FwdArgs& a, hipStream_t s);
hipError_t dispatch_area_full_rt(const FwdArgs& a, hipStream_t s);
hipError_t dispatch_backward_full_rt(int pm, const BwdArgs& b, hipStream_t s);
// sot_hip.hip.  Elem: the element type of the weight rows pr->x / pr->y in memory (and, for the backward, of the gradient rows gx / gy, which
// then point at 16-bit elements).  A bf16 problem reaches the two routers only where bf16_native(pr, with the backward's buffers) holds; they
// pick the 16-bit instantiation of the route the float32 call takes.  rescale: the fix-up mode of the 16-bit y-only kernel (BwdArgs::rescale).
enum class Elem { f32, bf16 };
int launch_prepare(const float* xpos, const float* ypos, int n, int m, float* sx, float* sy, int* px, int* py, int* ident,
                   hipStream_t s, bool unit = false);
int setup_launch(const sot_problem* pr, bool with_grad, void* workspace, size_t workspace_bytes, void* stream, Launch* out);
int run_forward(const sot_problem* pr, float* row_loss, float* uq, float* vq, float* Q, float* U, float* V, bool quant,
                void* workspace, size_t workspace_bytes, void* stream, const MeanTail* mean_tail = nullptr, Elem wt = Elem::f32);
int run_backward(const sot_problem* pr, const float* grad_row, int64_t grad_row_stride, float grad_scale, float* gx, float* gy,
                 void* workspace, size_t workspace_bytes, void* stream, float* row_loss_out = nullptr, bool* fused = nullptr,
                 const MeanTail* mean_tail = nullptr, Elem wt = Elem::f32, const float* rescale = nullptr);
// the bodies of sot_w1d_forward / _loss / _backward / _loss_and_grad and of their _bf16 twins (gx, gy: rows of wt; rescale: bf16 only)
int forward_call(Elem wt, const sot_problem* prob, float* row_loss, void* workspace, size_t workspace_bytes, void* stream);
int loss_call(Elem wt, const sot_problem* prob, float* row_loss, double denom, int apply_hinge, float hinge_threshold, float* mean_out, double* sum_out,
              uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream);
int backward_call(Elem wt, const sot_problem* prob, const float* grad_row, int64_t grad_row_stride, float grad_scale, void* grad_x, void* grad_y,
                  const float* rescale, void* workspace, size_t workspace_bytes, void* stream);
int loss_and_grad_call(Elem wt, const sot_problem* prob, float* row_loss, double denom, float* mean_out, double* sum_out, float grad_scale, void* grad_y,
                       uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream);
// sot_bf16.hip (bfloat16 rows): the row conversions, the native routes' condition, the workspace of a typed call, and the typed call itself:
// `call` on the 16-bit rows where the native kernels take them, else on float32 images in the workspace (widen, the float32 call, narrow).
int launch_rows_bf16_to_f32(const uint16_t* src, int64_t B, int n, int64_t ss, float* dst, int64_t ds, hipStream_t s);
int launch_rows_f32_to_bf16(const float* src, int64_t B, int n, int64_t ss, uint16_t* dst, int64_t ds, hipStream_t s);
bool bf16_native(const sot_problem* pr, bool backward);
size_t bf16_workspace_bytes(const sot_problem* pr, bool backward, bool want_x, bool want_y);
using RowsCall = std::function<int(Elem wt, const sot_problem* pr, float* gx, float* gy, const float* rescale, void* workspace, size_t workspace_bytes)>;
int bf16_rows_call(const sot_problem* pr, bool backward, uint16_t* gx, uint16_t* gy, const float* rescale, void* workspace, size_t workspace_bytes,
                   void* stream, const RowsCall& call);
// sot_csr.hip
int run_forward_csr(const float* xw, const float* xp, const int64_t* xoff, int64_t x_nnz, const float* yw, const float* yp,
                    const int64_t* yoff, int64_t y_nnz, int64_t B, int max_n, int max_m, float p, uint32_t flags, float* row_loss,
                    void* stream);
// sot_posgrad.hip
int run_position_grad(const sot_problem* pr, const float* grad_row, int64_t grad_row_stride, float grad_scale, float* gxp, float* gyp,
                      void* workspace, size_t workspace_bytes, void* stream);
int run_column_sum(const float* rows, int64_t B, int n, int64_t stride, float* out, void* stream);
// sot_quantgrad.hip
int run_quantiles_backward(const sot_problem* pr, const float* gUq, const float* gVq, const float* gQ, const float* gU, const float* gV,
                           float* gx, float* gy, float* gxp, float* gyp, void* workspace, size_t workspace_bytes, void* stream);

}  // namespace sot
