// sot_bf16.hip -- bfloat16 weight rows (ABI 19 / 20): the two row-conversion kernels (bf16 -> f32, f32 -> bf16 with round to nearest even) and
// their entry points, the instantiations of the full-row forward kernels that read 16-bit rows directly (sot_full_fwd.hpp: the shared geometry
// tables with WT = uint16_t), the native routes' condition, and the typed call (bf16_rows_call) through which all four typed entry points
// run the bodies of their float32 twins (sot_hip.hip); sot_w1d_forward_bf16 / sot_w1d_loss_bf16 are here, the two of the backward in
// sot_bf16_bwd.hip.  Routing is not: run_forward / run_backward (sot_hip.hip) route both element types.
// A bfloat16 is the upper half of a float32, so widening is exact and "upcast, then the float32 arithmetic" defines every result: the
// native kernels widen in the register behind the load, every other problem is widened into the workspace and takes the float32 call as it is.
#include "sot_full_fwd.hpp"

namespace sot {

// ---------------------------------------------------------------------------------------------
// Row conversion.  A workgroup of 256 threads walks groups of `rpg` rows (as many short rows as its threads cover in one pass); a thread
// owns chunks of CH consecutive elements: CH = 8 -- one 16-byte access on the 16-bit side, two on the 32-bit side -- where both pointers,
// both strides and the length allow, CH = 1 (element-wise: rows that start 2 bytes off a boundary, odd lengths) otherwise.
// (f32_to_bf16_rne: sot_full_common.hpp)
// ---------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(256) void sot_rows_bf16_to_f32_kernel(const uint16_t* __restrict__ src, int64_t B, int n, int64_t ss,
                                                                   float* __restrict__ dst, int64_t ds, int cpr, int rpg)
{
    const int64_t groups = (B + rpg - 1) / rpg;
    const int units = rpg * cpr;   // <= 256 when rpg > 1; cpr when one row takes several passes
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        for (int i = threadIdx.x; i < units; i += 256) {
            const int lr = i / cpr, c = i - lr * cpr;
            const int64_t row = g * rpg + lr;
            if (row >= B) continue;
            const uint16_t* const s = src + row * ss + (int64_t)c * CH;
            float* const d = dst + row * ds + (int64_t)c * CH;
            if constexpr (CH == 8) {   // (c < n / 8: whole chunks inside the row)
                const uint4 v = *reinterpret_cast<const uint4*>(s);
                reinterpret_cast<float4*>(d)[0] = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u),
                                                              __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xFFFF0000u));
                reinterpret_cast<float4*>(d)[1] = make_float4(__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xFFFF0000u),
                                                              __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xFFFF0000u));
            } else {
                d[0] = __uint_as_float((uint32_t)s[0] << 16);
            }
        }
    }
}

template <int CH>
__global__ __launch_bounds__(256) void sot_rows_f32_to_bf16_kernel(const float* __restrict__ src, int64_t B, int n, int64_t ss,
                                                                   uint16_t* __restrict__ dst, int64_t ds, int cpr, int rpg)
{
    const int64_t groups = (B + rpg - 1) / rpg;
    const int units = rpg * cpr;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        for (int i = threadIdx.x; i < units; i += 256) {
            const int lr = i / cpr, c = i - lr * cpr;
            const int64_t row = g * rpg + lr;
            if (row >= B) continue;
            const float* const s = src + row * ss + (int64_t)c * CH;
            uint16_t* const d = dst + row * ds + (int64_t)c * CH;
            if constexpr (CH == 8) {
                const float4 a = reinterpret_cast<const float4*>(s)[0], b = reinterpret_cast<const float4*>(s)[1];
                uint4 v;
                v.x = (uint32_t)f32_to_bf16_rne(a.x) | ((uint32_t)f32_to_bf16_rne(a.y) << 16);
                v.y = (uint32_t)f32_to_bf16_rne(a.z) | ((uint32_t)f32_to_bf16_rne(a.w) << 16);
                v.z = (uint32_t)f32_to_bf16_rne(b.x) | ((uint32_t)f32_to_bf16_rne(b.y) << 16);
                v.w = (uint32_t)f32_to_bf16_rne(b.z) | ((uint32_t)f32_to_bf16_rne(b.w) << 16);
                *reinterpret_cast<uint4*>(d) = v;
            } else {
                d[0] = f32_to_bf16_rne(s[0]);
            }
        }
    }
}

// chunks per row and rows per group of the conversion kernels, and their grid (eight 256-thread workgroups fill a CU's wave slots)
struct ConvGeo { int cpr, rpg, grid; };
static inline ConvGeo conv_geo(int64_t B, int n, int ch)
{
    ConvGeo g;
    g.cpr = (n + ch - 1) / ch;
    g.rpg = g.cpr >= 256 ? 1 : 256 / g.cpr;
    g.grid = capped_grid((B + g.rpg - 1) / g.rpg, 8);
    return g;
}

static int check_rows(const void* src, int64_t B, int32_t n, int64_t ss, const void* dst, int64_t ds)
{
    if (B < 0 || n < 1 || ss < n || ds < n) return SOT_ERR_BAD_SHAPE;
    if (B > 0 && (src == nullptr || dst == nullptr)) return SOT_ERR_NULL_POINTER;
    return SOT_OK;
}

int launch_rows_bf16_to_f32(const uint16_t* src, int64_t B, int n, int64_t ss, float* dst, int64_t ds, hipStream_t s)
{
    if (B == 0) return SOT_OK;
    const bool vec = (n & 7) == 0 && (ss & 7) == 0 && (ds & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    const ConvGeo g = conv_geo(B, n, vec ? 8 : 1);
    (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
    if (vec) hipLaunchKernelGGL(sot_rows_bf16_to_f32_kernel<8>, dim3(g.grid), dim3(256), 0, s, src, B, n, ss, dst, ds, g.cpr, g.rpg);
    else hipLaunchKernelGGL(sot_rows_bf16_to_f32_kernel<1>, dim3(g.grid), dim3(256), 0, s, src, B, n, ss, dst, ds, g.cpr, g.rpg);
    return launch_status();
}

int launch_rows_f32_to_bf16(const float* src, int64_t B, int n, int64_t ss, uint16_t* dst, int64_t ds, hipStream_t s)
{
    if (B == 0) return SOT_OK;
    const bool vec = (n & 7) == 0 && (ss & 3) == 0 && (ds & 7) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    const ConvGeo g = conv_geo(B, n, vec ? 8 : 1);
    (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
    if (vec) hipLaunchKernelGGL(sot_rows_f32_to_bf16_kernel<8>, dim3(g.grid), dim3(256), 0, s, src, B, n, ss, dst, ds, g.cpr, g.rpg);
    else hipLaunchKernelGGL(sot_rows_f32_to_bf16_kernel<1>, dim3(g.grid), dim3(256), 0, s, src, B, n, ss, dst, ds, g.cpr, g.rpg);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------
// Native 16-bit rows: the merge-free and the merge kernels of the shared geometry tables (sot_full_fwd.hpp) are compiled into this object
// ---------------------------------------------------------------------------------------------
template hipError_t dispatch_area_full_pow2<uint16_t>(const FwdArgs& a, hipStream_t s);
template hipError_t dispatch_forward_full_pow2<uint16_t>(int pm, const FwdArgs& a, hipStream_t s);

// The native routes' condition on the PROBLEM (host side; sot_w1d_bf16_native and the two workspace functions report by it): shared positions,
// n == m in the set of the tables above, kernels with the length at compile time allowed, weights normalised by the call, rows of x and y on
// 16-byte boundaries (pointer 16-byte aligned, row strides multiples of 8 elements).  backward: not the opt-in merge-free training form either,
// which has no 16-bit instantiation (the forward ignores that flag, as the float32 forward does).  A call adds the condition on its buffers:
// gradient rows on 16-byte boundaries (bf16_rows_call).
bool bf16_native(const sot_problem* pr, bool backward)
{
    return pr->xpos_row_stride == 0 && pr->ypos_row_stride == 0 && pr->n == pr->m &&
           (pr->n == 512 || pr->n == 1024 || pr->n == 2048 || pr->n == 4096) &&
           !(pr->flags & (SOT_FLAG_PRENORMALIZED | SOT_FLAG_NO_SPECIALIZE)) && !(backward && (pr->flags & SOT_FLAG_TIE_FREE_GRADIENT)) &&
           ((reinterpret_cast<uintptr_t>(pr->x) | reinterpret_cast<uintptr_t>(pr->y)) & 15) == 0 && (pr->x_row_stride & 7) == 0 && (pr->y_row_stride & 7) == 0;
}

// the float32 images of a widened call at the front of the workspace:
// [x, dense | y, dense | grad_x, dense (if asked for) | grad_y, dense (if asked for) | the float32 call's own workspace]
struct WidenLayout { size_t xf, yf, gxf, gyf, inner, total; };
static inline WidenLayout widen_layout(const sot_problem* pr, bool want_x, bool want_y)
{
    WidenLayout w;
    const size_t B = pr->B > 0 ? (size_t)pr->B : 0;
    const size_t xb = align_up(B * (size_t)pr->n * sizeof(float), 256), yb = align_up(B * (size_t)pr->m * sizeof(float), 256);
    w.xf = 16;   // room to move the first image up to a 16-byte boundary, whatever the workspace's own alignment
    w.yf = w.xf + xb;
    w.gxf = w.yf + yb;
    w.gyf = w.gxf + (want_x ? xb : 0);
    w.inner = w.gyf + (want_y ? yb : 0);
    w.total = w.inner + sot_workspace_bytes(pr);
    return w;
}

size_t bf16_workspace_bytes(const sot_problem* pr, bool backward, bool want_x, bool want_y)
{
    if (pr == nullptr || pr->n < 1 || pr->m < 1) return 0;
    return bf16_native(pr, backward) ? sot_workspace_bytes(pr) : widen_layout(pr, want_x, want_y).total;
}

// A call on bfloat16 rows x, y (backward: with bfloat16 gradient rows gx, gy).  Native problems: `call` on the rows as they are.  Every other
// problem: widen, the float32 call as it is, narrow -- one rounding to nearest even of the float32 gradient, the fix-up multiply in front of it.
// Every refusal is decided before anything is enqueued.
int bf16_rows_call(const sot_problem* pr, bool backward, uint16_t* gx, uint16_t* gy, const float* rescale, void* workspace, size_t workspace_bytes,
                   void* stream, const RowsCall& call)
{
    int rc = validate(pr);
    if (rc != SOT_OK) return rc;
    if (rescale != nullptr && gx != nullptr) return SOT_ERR_BAD_SHAPE;   // the fix-up mode belongs to the y-only call
    if (bf16_native(pr, backward) && ((reinterpret_cast<uintptr_t>(gx) | reinterpret_cast<uintptr_t>(gy)) & 15) == 0)
        return call(Elem::bf16, pr, reinterpret_cast<float*>(gx), reinterpret_cast<float*>(gy), rescale, workspace, workspace_bytes);
    {
        LaunchCfg cfg; size_t lds; int block, rpw;
        if (!pick_cfg(pr->n, pr->m, pr->xpos_row_stride != 0, backward, &cfg, &lds, &block, &rpw)) return SOT_ERR_UNSUPPORTED_SIZE;
    }
    if (pr->B == 0 || (backward && gx == nullptr && gy == nullptr))   // nothing follows x or y: the float32 call's own answer
        return call(Elem::f32, pr, nullptr, nullptr, nullptr, workspace, workspace_bytes);
    const WidenLayout w = widen_layout(pr, gx != nullptr, gy != nullptr);
    if (workspace == nullptr) return SOT_ERR_NULL_POINTER;
    if (workspace_bytes < w.total) return SOT_ERR_WORKSPACE;
    char* const base = reinterpret_cast<char*>(workspace);
    const size_t lead = (size_t)((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15);   // <= 15 < w.xf
    const auto image = [&](size_t off) { return reinterpret_cast<float*>(base + lead + (off - w.xf)); };
    float* const xf = image(w.xf); float* const yf = image(w.yf);
    float* const gxf = gx != nullptr ? image(w.gxf) : nullptr; float* const gyf = gy != nullptr ? image(w.gyf) : nullptr;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = launch_rows_bf16_to_f32(reinterpret_cast<const uint16_t*>(pr->x), pr->B, pr->n, pr->x_row_stride, xf, pr->n, s);
    if (rc != SOT_OK) return rc;
    rc = launch_rows_bf16_to_f32(reinterpret_cast<const uint16_t*>(pr->y), pr->B, pr->m, pr->y_row_stride, yf, pr->m, s);
    if (rc != SOT_OK) return rc;
    sot_problem wide = *pr;
    wide.x = xf; wide.y = yf; wide.x_row_stride = pr->n; wide.y_row_stride = pr->m;
    rc = call(Elem::f32, &wide, gxf, gyf, nullptr, image(w.inner), w.total - w.inner);
    if (rc == SOT_OK && gxf != nullptr) rc = launch_rows_f32_to_bf16(gxf, pr->B, pr->n, pr->n, gx, pr->n, s);
    if (rc == SOT_OK && gyf != nullptr && rescale != nullptr)   // float32 multiply in front of the one rounding (a no-op kernel when the scalar is exactly 1)
        rc = sot_scale_inplace(gyf, pr->B * (int64_t)pr->m, rescale, stream);
    if (rc == SOT_OK && gyf != nullptr) rc = launch_rows_f32_to_bf16(gyf, pr->B, pr->m, pr->m, gy, pr->m, s);
    return rc;
}

}  // namespace sot

extern "C" {

int sot_rows_bf16_to_f32(const uint16_t* src, int64_t B, int32_t n, int64_t src_row_stride, float* dst, int64_t dst_row_stride, void* stream)
{
    const int rc = sot::check_rows(src, B, n, src_row_stride, dst, dst_row_stride);
    if (rc != SOT_OK) return rc;
    return sot::launch_rows_bf16_to_f32(src, B, (int)n, src_row_stride, dst, dst_row_stride, reinterpret_cast<hipStream_t>(stream));
}

int sot_rows_f32_to_bf16(const float* src, int64_t B, int32_t n, int64_t src_row_stride, uint16_t* dst, int64_t dst_row_stride, void* stream)
{
    const int rc = sot::check_rows(src, B, n, src_row_stride, dst, dst_row_stride);
    if (rc != SOT_OK) return rc;
    return sot::launch_rows_f32_to_bf16(src, B, (int)n, src_row_stride, dst, dst_row_stride, reinterpret_cast<hipStream_t>(stream));
}

size_t sot_w1d_bf16_workspace_bytes(const sot_problem* prob) { return sot::bf16_workspace_bytes(prob, false, false, false); }

int sot_w1d_forward_bf16(const sot_problem* prob, float* row_loss, void* workspace, size_t workspace_bytes, void* stream)
{
    return sot::forward_call(sot::Elem::bf16, prob, row_loss, workspace, workspace_bytes, stream);
}

int sot_w1d_loss_bf16(const sot_problem* prob, float* row_loss, double denom, int apply_hinge, float hinge_threshold, float* mean_out,
                      double* sum_out, uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream)
{
    return sot::loss_call(sot::Elem::bf16, prob, row_loss, denom, apply_hinge, hinge_threshold, mean_out, sum_out, completion_counters, workspace,
                          workspace_bytes, stream);
}

}  // extern "C"
