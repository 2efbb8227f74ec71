// sot_bf16_bwd.hip -- bfloat16 training (ABI 20): the instantiations of the full-row backward kernel that read 16-bit weight rows and store
// 16-bit gradients (sot_full_bwd.hpp: sot_backward_full_kernel with WT = GT = uint16_t -- the both-gradient backward and the y-only training
// form, which accumulates the row loss on its walk), and the typed entry points sot_w1d_backward_bf16 / sot_w1d_loss_and_grad_bf16 with their
// workspace arithmetic.  The result is defined bit for bit: widen exactly, the float32 arithmetic, ONE rounding to nearest even of the float32
// gradient -- on the native route at the store of the kernel, on every other problem by widening into the workspace, the float32 call as it is
// and the row-conversion kernel of sot_bf16.hip.
#include "sot_full_bwd.hpp"

namespace sot {

// ---------------------------------------------------------------------------------------------
// Native 16-bit rows and gradients: the geometries that a row fills, on shared positions (the NX == 0 set without 8192 bins), with the
// geometry choices of dispatch_backward_full (sot_full_bwd.hip): the y-only layouts without U gradient slots at 1024 and 2048 bins.
// ---------------------------------------------------------------------------------------------
static hipError_t dispatch_backward_full_bf16(int pm, const BwdArgs& b, hipStream_t s)
{
    using H = uint16_t;
    switch (b.f.n) {
        case 512: return dispatch_backward_full_g<64, 8, 4, 0, 3, H, H>(pm, b, s);
        case 1024:
            if (b.gx == nullptr) return dispatch_backward_full_y<128, 8, 2, 0, true, 1, H, H>(pm, b, s);
            return dispatch_backward_full_g<128, 8, 2, 0, 1, H, H>(pm, b, s);
        case 2048:
            // y-only: compiled for four waves per SIMD.  Uncapped, the modes without square_dist take 129 / 130 VGPRs (float32: 125 / 126), and at
            // three waves per SIMD only ONE of these 8-wave workgroups is resident on a CU instead of the two its LDS allows.  (The both-gradient
            // kernel's 129 VGPRs under square_dist cost nothing: one row with U slots takes 50.9 KB, three 4-wave workgroups per CU either way.)
            if (b.gx == nullptr) return dispatch_backward_full_y<256, 8, 2, 0, true, 4, H, H>(pm, b, s);
            return dispatch_backward_full_g<256, 8, 1, 0, 1, H, H>(pm, b, s);
        case 4096: return dispatch_backward_full_g<512, 8, 1, 0, 3, H, H>(pm, b, s);
        default: return hipErrorInvalidConfiguration;
    }
}

// The native route's condition on the PROBLEM (sot_w1d_bf16_native and the workspace function report by it): the typed forward's
// (bf16_native, sot_bf16.hip) without the opt-in merge-free training form, which has no 16-bit instantiation.  The call adds the condition
// on its buffers: gradient rows on 16-byte boundaries.
static inline bool bf16_backward_native(const sot_problem* pr)
{
    return bf16_native(pr) && !(pr->flags & SOT_FLAG_TIE_FREE_GRADIENT);
}

// the float32 images of a widened call at the front of the workspace:
// [x, dense | y, dense | grad_x, dense (if asked for) | grad_y, dense (if asked for) | the float32 call's own workspace]
struct BwdWidenLayout { size_t xf, yf, gxf, gyf, inner, total; };
static inline BwdWidenLayout bwd_widen_layout(const sot_problem* pr, bool want_x, bool want_y)
{
    BwdWidenLayout w;
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

// row_loss_out (the training form): the row losses always come back -- from the y-only kernel's walk where one exists, from the forward
// kernel behind the backward otherwise (what sot_w1d_loss_and_grad does).
static int run_backward_bf16(const sot_problem* pr, const float* grad_row, int64_t grad_row_stride, float grad_scale, uint16_t* gx, uint16_t* gy,
                             const float* rescale, void* workspace, size_t workspace_bytes, void* stream, float* row_loss_out, const MeanTail* mean_tail)
{
    int rc = validate(pr);
    if (rc != SOT_OK) return rc;
    if (rescale != nullptr && gx != nullptr) return SOT_ERR_BAD_SHAPE;   // the fix-up mode belongs to the y-only call
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(gx) | reinterpret_cast<uintptr_t>(gy)) & 15) == 0;
    if (bf16_backward_native(pr) && aligned16) {
        Launch l;
        rc = setup_launch(pr, true, workspace, workspace_bytes, stream, &l);   // positions, plan, flags: nothing in it follows x or y
        if (rc != SOT_OK) return rc;
        if (pr->B == 0 || (gx == nullptr && gy == nullptr)) return SOT_OK;
        BwdArgs b{};
        b.f = l.a; b.grad_row = grad_row; b.grad_row_stride = grad_row_stride; b.grad_scale = grad_scale;
        b.gx = reinterpret_cast<float*>(gx); b.gy = reinterpret_cast<float*>(gy); b.rescale = rescale;
        if (gx == nullptr && row_loss_out != nullptr) {   // the y-only kernel accumulates the loss on its walk
            b.f.row_loss = row_loss_out;
            if (mean_tail != nullptr) b.f.mt = *mean_tail;
        }
        return launch_status(dispatch_backward_full_bf16(l.pm, b, l.s));
    }
    // every other problem: widen, the float32 call as it is, narrow.  Refusals are decided before the conversions are enqueued.
    {
        LaunchCfg cfg; size_t lds; int block, rpw;
        if (!pick_cfg(pr->n, pr->m, pr->xpos_row_stride != 0, true, &cfg, &lds, &block, &rpw)) return SOT_ERR_UNSUPPORTED_SIZE;
    }
    if (pr->B == 0 || (gx == nullptr && gy == nullptr))   // nothing follows x or y: the float32 call's own answer
        return run_backward(pr, grad_row, grad_row_stride, grad_scale, nullptr, nullptr, workspace, workspace_bytes, stream);
    const BwdWidenLayout w = bwd_widen_layout(pr, gx != nullptr, gy != nullptr);
    if (workspace == nullptr) return SOT_ERR_NULL_POINTER;
    if (workspace_bytes < w.total) return SOT_ERR_WORKSPACE;
    char* const base = reinterpret_cast<char*>(workspace);
    const size_t lead = (size_t)((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15);   // <= 15 < w.xf
    const auto image = [&](size_t off) { return reinterpret_cast<float*>(base + lead + (off - w.xf)); };
    float* const xf = image(w.xf); float* const yf = image(w.yf);
    float* const gxf = gx != nullptr ? image(w.gxf) : nullptr; float* const gyf = gy != nullptr ? image(w.gyf) : nullptr;
    void* const inner = image(w.inner);
    const size_t inner_bytes = w.total - w.inner;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = launch_rows_bf16_to_f32(reinterpret_cast<const uint16_t*>(pr->x), pr->B, pr->n, pr->x_row_stride, xf, pr->n, s);
    if (rc != SOT_OK) return rc;
    rc = launch_rows_bf16_to_f32(reinterpret_cast<const uint16_t*>(pr->y), pr->B, pr->m, pr->y_row_stride, yf, pr->m, s);
    if (rc != SOT_OK) return rc;
    sot_problem wide = *pr;
    wide.x = xf; wide.y = yf; wide.x_row_stride = pr->n; wide.y_row_stride = pr->m;
    bool fused = false;
    rc = run_backward(&wide, grad_row, grad_row_stride, grad_scale, gxf, gyf, inner, inner_bytes, stream, row_loss_out, &fused, mean_tail);
    if (rc != SOT_OK) return rc;
    if (row_loss_out != nullptr && !fused) {
        rc = run_forward(&wide, row_loss_out, nullptr, nullptr, nullptr, nullptr, nullptr, false, inner, inner_bytes, stream, mean_tail);
        if (rc != SOT_OK) return rc;
    }
    if (gxf != nullptr) {
        rc = launch_rows_f32_to_bf16(gxf, pr->B, pr->n, pr->n, gx, pr->n, s);
        if (rc != SOT_OK) return rc;
    }
    if (gyf != nullptr) {
        if (rescale != nullptr) {   // float32 multiply in front of the one rounding (a no-op kernel when the scalar is exactly 1)
            rc = sot_scale_inplace(gyf, pr->B * (int64_t)pr->m, rescale, stream);
            if (rc != SOT_OK) return rc;
        }
        rc = launch_rows_f32_to_bf16(gyf, pr->B, pr->m, pr->m, gy, pr->m, s);
    }
    return rc;
}

}  // namespace sot

extern "C" {

int sot_w1d_bf16_native(const sot_problem* prob)
{
    if (prob == nullptr || prob->n < 1 || prob->m < 1) return 0;
    return sot::bf16_backward_native(prob) ? 1 : 0;
}

size_t sot_w1d_bf16_backward_workspace_bytes(const sot_problem* prob, int want_grad_x, int want_grad_y)
{
    if (prob == nullptr || prob->n < 1 || prob->m < 1) return 0;
    return sot::bf16_backward_native(prob) ? sot_workspace_bytes(prob) : sot::bwd_widen_layout(prob, want_grad_x != 0, want_grad_y != 0).total;
}

int sot_w1d_backward_bf16(const sot_problem* prob, const float* grad_row, int64_t grad_row_stride, float grad_scale, uint16_t* grad_x,
                          uint16_t* grad_y, const float* rescale, void* workspace, size_t workspace_bytes, void* stream)
{
    if (grad_row_stride != 0 && grad_row_stride != 1) return SOT_ERR_BAD_SHAPE;
    return sot::run_backward_bf16(prob, grad_row, grad_row_stride, grad_scale, grad_x, grad_y, rescale, workspace, workspace_bytes, stream, nullptr, nullptr);
}

int sot_w1d_loss_and_grad_bf16(const sot_problem* prob, float* row_loss, double denom, float* mean_out, double* sum_out, float grad_scale,
                               uint16_t* grad_y, uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream)
{
    if (prob == nullptr) return SOT_ERR_NULL_POINTER;
    if (prob->B == 0) return SOT_ERR_BAD_SHAPE;  // the mean of zero rows is undefined
    if (row_loss == nullptr || grad_y == nullptr || (mean_out == nullptr && sum_out == nullptr)) return SOT_ERR_NULL_POINTER;
    sot::MeanTail mt{};
    mt.counters = completion_counters; mt.denom = denom; mt.apply_hinge = 0; mt.hinge = 0.0f; mt.mean_out = mean_out; mt.sum_out = sum_out;
    const sot::MeanTail* tail = completion_counters ? &mt : nullptr;
    const int rc = sot::run_backward_bf16(prob, nullptr, 0, grad_scale, nullptr, grad_y, nullptr, workspace, workspace_bytes, stream, row_loss, tail);
    if (rc != SOT_OK || tail != nullptr) return rc;   // (with a tail the kernel that wrote the row losses reduced them)
    return sot_w1d_reduce_mean(row_loss, prob->B, denom, 0, 0.0f, mean_out, sum_out, stream);
}

}  // extern "C"
