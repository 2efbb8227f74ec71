// sot_full_bwd.hip -- full-row backward kernels for compile-time row lengths, and the merge-free training form;
// the kernel and launch templates are in sot_full_bwd.hpp.
#include "sot_full_bwd.hpp"

namespace sot {

// Preconditions: those of dispatch_backward_full with gx == nullptr, plus p == 1, no quantile cutoff, SOT_FLAG_SAME_GRID.
hipError_t dispatch_area_train(const BwdArgs& b, hipStream_t s)
{
    switch (b.f.n) {
        case 512: return dispatch_area_train_g<64, 8, 4>(b, s);
        case 1024: return dispatch_area_train_g<128, 8, 2>(b, s);
        case 2048: return dispatch_area_train_g<256, 8, 1>(b, s);
        case 4096: return dispatch_area_train_g<512, 8, 1>(b, s);
        case 129: return dispatch_area_train_g<64, 3, 4, 129>(b, s);
        case 257: return dispatch_area_train_g<64, 5, 4, 257>(b, s);
        case 513: return dispatch_area_train_g<64, 9, 4, 513>(b, s);
        case 1025: return dispatch_area_train_g<128, 9, 2, 1025>(b, s);   // (one wave per row, 64 x 17 as the forward: 208 VGPRs, 96 us at 16384 rows)
        case 2049: return dispatch_area_train_g<256, 9, 1, 2049>(b, s);
        default: return hipErrorInvalidConfiguration;
    }
}
bool area_train_supports(int n) { return n == 512 || n == 1024 || n == 2048 || n == 4096 || n == 129 || n == 257 || n == 513 || n == 1025 || n == 2049; }

hipError_t dispatch_backward_full(int pm, const BwdArgs& b, hipStream_t s)
{
    switch (b.f.n) {
        case 129: return dispatch_backward_full_g<64, 3, 4, 129>(pm, b, s);
        case 2049:   // y-only: 47.7 instead of 57 KB per row = three rows per CU instead of two: 8192 rows 119.2 -> 95.5 us
            if (b.gx == nullptr) return dispatch_backward_full_y<256, 9, 1, 2049, true, 1>(pm, b, s);
            return dispatch_backward_full_g<256, 9, 1, 2049, 1>(pm, b, s);
        case 257:
            return dispatch_backward_full_g<64, 5, 4, 257>(pm, b, s);
        case 513:
            // y-only: the layout without U gradient slots (35.5 KB per four rows): 8192 rows 26.6 -> 25.0 us, 32768 rows 75.8 -> 74.5 us
            if (b.gx == nullptr) return dispatch_backward_full_y<64, 9, 4, 513, true, 4>(pm, b, s);
            return dispatch_backward_full_g<64, 9, 4, 513, 1>(pm, b, s);
        case 1025:
            // y-only (training) kernel: the layout without U gradient slots (39 KB per two rows) compiled for four workgroups per CU
            // (128 VGPRs, 9 dwords spilled) holds eight rows per CU instead of six: 4096 rows 30.8 -> 29.1 us, 16384 rows 88.9 -> 85.6 us
            if (b.gx == nullptr) return dispatch_backward_full_y<128, 9, 2, 1025, true, 4>(pm, b, s);
            return dispatch_backward_full_g<128, 9, 2, 1025, 1>(pm, b, s);
        default: return dispatch_backward_full_pow2<float>(pm, b, s);   // 512 ... 4096 bins: the table shared with the 16-bit rows (sot_full_bwd.hpp)
    }
}

hipError_t dispatch_backward_full_rowpos(int pm, const BwdArgs& b, hipStream_t s)
{
    switch (b.f.n) {
        case 2048: return dispatch_backward_full_rowpos_g<256>(pm, b, s);
        case 512: return dispatch_backward_full_rowpos_g<64>(pm, b, s);
        // (1024-point rows stay on the generic kernel: its 128 x 12 partition of the fp64 sums rounds a handful of near-zero gradient entries another
        // way than 128 x 8 would -- <= 9e-8 of the row's scale on clustered / degenerate rows, tools/r6/fuzz_rowpos.py -- and every per-row route giving
        // the same bits is worth more than that shape's backward time; 2048 and 512 share the generic kernel's partition)
        default: return hipErrorInvalidConfiguration;
    }
}

}  // namespace sot
