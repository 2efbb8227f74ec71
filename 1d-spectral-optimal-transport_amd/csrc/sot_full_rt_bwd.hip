// sot_full_rt_bwd.hip -- full-row backward kernels for run-time row lengths (full_rt_capacity);
// the kernel and launch templates are in sot_full_bwd.hpp.
#include "sot_full_bwd.hpp"

namespace sot {

// y-only (training) kernels in the layout without U gradient slots, as the compile-time kernels of 1024 / 2048 points, capped at 128
// VGPRs (MINB 4) so that the smaller region does buy another resident workgroup.  Interleaved A/B against the full layout (bit-identical
// results): 1024-point geometry 16384 x 1000 paper mode 106.1 -> 96.6 us -- adopted; 2048-point geometry 8192 x 2000 paper mode
// 109.1 -> 111.6 us -- the spills cost what the fourth row buys; stays in the full layout.
// run-time row lengths (see full_rt_capacity): both-gradient and y-only (training form: also the row losses) kernels
hipError_t dispatch_backward_full_rt(int pm, const BwdArgs& b, hipStream_t s)
{
    switch (full_rt_capacity(b.f.n)) {
        case 256: return dispatch_backward_full_g<64, 4, 4, -1>(pm, b, s);
        case 512: return dispatch_backward_full_g<64, 8, 4, -1>(pm, b, s);
        case 1024:
            if (b.gx == nullptr) return dispatch_backward_full_y<128, 8, 2, -1, true, 4>(pm, b, s);
            return dispatch_backward_full_g<128, 8, 2, -1, 1>(pm, b, s);
        case 1536: return dispatch_backward_full_g<192, 8, 1, -1>(pm, b, s);
        case 2048: return dispatch_backward_full_g<256, 8, 1, -1>(pm, b, s);
        case 3072: return dispatch_backward_full_g<384, 8, 1, -1>(pm, b, s);
        case 4096: return dispatch_backward_full_g<512, 8, 1, -1>(pm, b, s);
        default: return hipErrorInvalidConfiguration;
    }
}

}  // namespace sot
