// sot_full_rt_fwd.hip -- full-row forward kernels for run-time row lengths (full_rt_capacity);
// the kernel and launch templates are in sot_full_fwd.hpp.
#include "sot_full_fwd.hpp"

namespace sot {

hipError_t dispatch_forward_full_rt(int pm, const FwdArgs& a, hipStream_t s)
{
    switch (full_rt_capacity(a.n)) {
        case 256: return dispatch_forward_full_g<64, 4, 4, -1>(pm, a, s);
        case 512: return dispatch_forward_full_g<64, 8, 4, -1>(pm, a, s);
        case 1024:   // large batches: one wave per row (16384 x 1000 paper mode 54.9 -> 50.6 us, 8192 rows 30.4 -> 29.9, 4096 rows 17.5 -> 19.2)
            if (a.B >= kRt1024OneWaveRows) return dispatch_forward_full_g<64, 16, 4, -1>(pm, a, s);
            return dispatch_forward_full_g<128, 8, 2, -1>(pm, a, s);
        case 1536: return dispatch_forward_full_g<192, 8, 1, -1>(pm, a, s);
        case 2048:   // (two waves per row, 16 elements per thread: 53.6 vs 53.9 us at 8192 x 2000 -- nothing; one row per workgroup 64.3 us)
            return dispatch_forward_full_g<256, 8, 1, -1>(pm, a, s);
        case 3072: return dispatch_forward_full_g<384, 8, 1, -1>(pm, a, s);
        case 4096: return dispatch_forward_full_g<512, 8, 1, -1>(pm, a, s);
        case 8192: return dispatch_forward_full_g<1024, 8, 1, -1>(pm, a, s);
        default: return hipErrorInvalidConfiguration;
    }
}

hipError_t dispatch_area_full_rt(const FwdArgs& a, hipStream_t s)
{
    switch (full_rt_capacity(a.n)) {
        case 256: return dispatch_area_full_g<64, 4, 4, -1>(a, s);
        case 512: return dispatch_area_full_g<64, 8, 4, -1>(a, s);
        // 1024-point geometry: one wave per row (16 elements per thread) -- 16384 x 1000 48.2 -> 40.4 us, 8192 rows 27.6 -> 23.3, 4096 rows
        // 17.0 -> 15.3, 2048 / 1024 rows as before; the 2048-point geometry with two waves per row instead of four: 46.6 -> 52.8 us, stays
        case 1024: return dispatch_area_full_g<64, 16, 4, -1>(a, s);
        case 1536: return dispatch_area_full_g<192, 8, 1, -1>(a, s);
        case 2048: return dispatch_area_full_g<256, 8, 1, -1>(a, s);   // (two waves per row, one row per 128-thread workgroup: 53.6 us)
        case 3072: return dispatch_area_full_g<384, 8, 1, -1>(a, s);
        case 4096: return dispatch_area_full_g<512, 8, 1, -1>(a, s);
        case 8192: return dispatch_area_full_g<1024, 8, 1, -1>(a, s);
        default: return hipErrorInvalidConfiguration;
    }
}

}  // namespace sot
