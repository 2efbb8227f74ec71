// sot_bf16_bwd.hip -- bfloat16 training (ABI 20): the instantiations of the full-row backward kernel that read 16-bit weight rows and store
// 16-bit gradients (sot_full_bwd.hpp: the shared geometry table with WT = GT = uint16_t -- the both-gradient backward and the y-only training
// form, which accumulates the row loss on its walk), and the typed entry points sot_w1d_backward_bf16 / sot_w1d_loss_and_grad_bf16: the
// bodies of their float32 twins (sot_hip.hip) through the typed call of sot_bf16.hip.  The result is defined bit for bit: widen exactly, the
// float32 arithmetic, ONE rounding to nearest even of the float32 gradient -- on the native route at the store of the kernel, on every
// other problem by bf16_rows_call.
#include "sot_full_bwd.hpp"

namespace sot {
template hipError_t dispatch_backward_full_pow2<uint16_t>(int pm, const BwdArgs& b, hipStream_t s);
}  // namespace sot

extern "C" {

int sot_w1d_bf16_native(const sot_problem* prob)
{
    if (prob == nullptr || prob->n < 1 || prob->m < 1) return 0;
    return sot::bf16_native(prob, true) ? 1 : 0;
}

size_t sot_w1d_bf16_backward_workspace_bytes(const sot_problem* prob, int want_grad_x, int want_grad_y)
{
    return sot::bf16_workspace_bytes(prob, true, want_grad_x != 0, want_grad_y != 0);
}

int sot_w1d_backward_bf16(const sot_problem* prob, const float* grad_row, int64_t grad_row_stride, float grad_scale, uint16_t* grad_x,
                          uint16_t* grad_y, const float* rescale, void* workspace, size_t workspace_bytes, void* stream)
{
    return sot::backward_call(sot::Elem::bf16, prob, grad_row, grad_row_stride, grad_scale, grad_x, grad_y, rescale, workspace, workspace_bytes, stream);
}

int sot_w1d_loss_and_grad_bf16(const sot_problem* prob, float* row_loss, double denom, float* mean_out, double* sum_out, float grad_scale,
                               uint16_t* grad_y, uint32_t* completion_counters, void* workspace, size_t workspace_bytes, void* stream)
{
    return sot::loss_and_grad_call(sot::Elem::bf16, prob, row_loss, denom, mean_out, sum_out, grad_scale, grad_y, completion_counters, workspace,
                                   workspace_bytes, stream);
}

}  // extern "C"
