// sot_dispatch.hpp -- run-time -> compile-time dispatch of the generic row kernels (sot_rows.hpp): the launch templates and the switches over geometry, p, cutoff and load width.  The objects that include it hold nothing
// but explicit instantiations: sot_fwd_shared.hip, sot_fwd_shared_cutoff.hip, sot_fwd_rowpos.hip, sot_bwd_shared.hip, sot_bwd_rowpos.hip.
#pragma once
#include "sot_launch.hpp"

namespace sot {

template <int G, int CPT, bool ROWPOS, bool QUANT, int PM, bool LIM, bool VEC, int SQM = 2>
static hipError_t launch_forward(const FwdArgs& a, size_t lds, int64_t want, int block, hipStream_t s)
{
    return launch_persistent<sot_forward_kernel<G, CPT, ROWPOS, QUANT, PM, LIM, VEC, false, SQM>>(a, lds, want, block, s);
}

template <int G, int CPT, bool ROWPOS, bool LIM, bool VEC>
static hipError_t dispatch_forward_pm(int pm, const FwdArgs& a, size_t lds, int64_t want, int block, hipStream_t s)
{
    // p = 1 and p = 2 get square_dist at compile time as well (one multiply + select per element less); any other p
    // goes through the generic variant (powf, runtime flag)
    const bool sq = (a.flags & SOT_FLAG_SQUARE) && !(a.flags & SOT_FLAG_PRENORMALIZED);
    switch (pm) {
        case 1: return sq ? launch_forward<G, CPT, ROWPOS, false, 1, LIM, VEC, 1>(a, lds, want, block, s)
                          : launch_forward<G, CPT, ROWPOS, false, 1, LIM, VEC, 0>(a, lds, want, block, s);
        case 2: return sq ? launch_forward<G, CPT, ROWPOS, false, 2, LIM, VEC, 1>(a, lds, want, block, s)
                          : launch_forward<G, CPT, ROWPOS, false, 2, LIM, VEC, 0>(a, lds, want, block, s);
        default: return launch_forward<G, CPT, ROWPOS, false, 0, LIM, VEC, 2>(a, lds, want, block, s);
    }
}

template <int G, int CPT, bool LIM>
hipError_t forward_shared(int pm, bool vec, const FwdArgs& a, size_t lds, int64_t want, int block, hipStream_t s)
{
    return vec ? dispatch_forward_pm<G, CPT, false, LIM, true>(pm, a, lds, want, block, s)
               : dispatch_forward_pm<G, CPT, false, LIM, false>(pm, a, lds, want, block, s);
}
// shared positions: the cutoff (LIM) and no-cutoff families are compiled in objects of their own (sot_fwd_shared_cutoff.hip,
// sot_fwd_shared.hip), each with one explicit instantiation SOT_FWD_SHARED_ALL(, LIMV); every other object sees external symbols
#define SOT_FWD_SHARED_ALL(PREFIX, LIMV)                                                                              \
    PREFIX template hipError_t forward_shared<64, 8, LIMV>(int, bool, const FwdArgs&, size_t, int64_t, int, hipStream_t);   \
    PREFIX template hipError_t forward_shared<128, 12, LIMV>(int, bool, const FwdArgs&, size_t, int64_t, int, hipStream_t); \
    PREFIX template hipError_t forward_shared<256, 8, LIMV>(int, bool, const FwdArgs&, size_t, int64_t, int, hipStream_t);  \
    PREFIX template hipError_t forward_shared<1024, 8, LIMV>(int, bool, const FwdArgs&, size_t, int64_t, int, hipStream_t); \
    PREFIX template hipError_t forward_shared<1024, 16, LIMV>(int, bool, const FwdArgs&, size_t, int64_t, int, hipStream_t);
SOT_FWD_SHARED_ALL(extern, false)
SOT_FWD_SHARED_ALL(extern, true)

template <int G, int CPT, bool ROWPOS>
static hipError_t dispatch_forward_g(bool quant, int pm, bool vec, const FwdArgs& a, size_t lds, int64_t want, int block, hipStream_t s)
{
    const bool lim = a.flags & SOT_FLAG_LIMIT_Q;
    if (quant)  // rare path: one generic build per cutoff flavour
        return lim ? launch_forward<G, CPT, ROWPOS, true, 0, true, false>(a, lds, want, block, s)
                   : launch_forward<G, CPT, ROWPOS, true, 0, false, false>(a, lds, want, block, s);
    if constexpr (ROWPOS) {
        return lim ? dispatch_forward_pm<G, CPT, ROWPOS, true, false>(pm, a, lds, want, block, s)
                   : dispatch_forward_pm<G, CPT, ROWPOS, false, false>(pm, a, lds, want, block, s);
    } else {
        if (lim) return forward_shared<G, CPT, true>(pm, vec, a, lds, want, block, s);
        return forward_shared<G, CPT, false>(pm, vec, a, lds, want, block, s);
    }
}

template <bool ROWPOS>
hipError_t dispatch_forward(const LaunchCfg& c, bool quant, int pm, bool vec, const FwdArgs& a, size_t lds, int64_t want, int block,
                            hipStream_t s)
{
    if (c.CPT == 16) return dispatch_forward_g<1024, 16, ROWPOS>(quant, pm, vec, a, lds, want, block, s);
    switch (c.G) {
        case 64: return dispatch_forward_g<64, 8, ROWPOS>(quant, pm, vec, a, lds, want, block, s);
        case 128: return dispatch_forward_g<128, 12, ROWPOS>(quant, pm, vec, a, lds, want, block, s);
        case 256: return dispatch_forward_g<256, 8, ROWPOS>(quant, pm, vec, a, lds, want, block, s);
        default: return dispatch_forward_g<1024, 8, ROWPOS>(quant, pm, vec, a, lds, want, block, s);
    }
}

template <int G, int CPT, bool ROWPOS, int PM, bool LIM, bool VEC>
static hipError_t launch_backward(const BwdArgs& b, size_t lds, int64_t want, int block, hipStream_t s)
{
    return launch_persistent<sot_backward_kernel<G, CPT, ROWPOS, PM, LIM, VEC>>(b, lds, want, block, s);
}

template <int G, int CPT, bool ROWPOS, bool LIM, bool VEC>
static hipError_t dispatch_backward_pm(int pm, const BwdArgs& b, size_t lds, int64_t want, int block, hipStream_t s)
{
    switch (pm) {
        case 1: return launch_backward<G, CPT, ROWPOS, 1, LIM, VEC>(b, lds, want, block, s);
        case 2: return launch_backward<G, CPT, ROWPOS, 2, LIM, VEC>(b, lds, want, block, s);
        default: return launch_backward<G, CPT, ROWPOS, 0, LIM, VEC>(b, lds, want, block, s);
    }
}

template <int G, int CPT, bool ROWPOS>
static hipError_t dispatch_backward_g(int pm, bool vec, const BwdArgs& b, size_t lds, int64_t want, int block, hipStream_t s)
{
    const bool lim = b.f.flags & SOT_FLAG_LIMIT_Q;
    if (ROWPOS || !vec)
        return lim ? dispatch_backward_pm<G, CPT, ROWPOS, true, false>(pm, b, lds, want, block, s)
                   : dispatch_backward_pm<G, CPT, ROWPOS, false, false>(pm, b, lds, want, block, s);
    return lim ? dispatch_backward_pm<G, CPT, false, true, true>(pm, b, lds, want, block, s)
               : dispatch_backward_pm<G, CPT, false, false, true>(pm, b, lds, want, block, s);
}

template <bool ROWPOS>
hipError_t dispatch_backward(const LaunchCfg& c, int pm, bool vec, const BwdArgs& b, size_t lds, int64_t want, int block,
                             hipStream_t s)
{
    if (c.CPT == 16) return dispatch_backward_g<1024, 16, ROWPOS>(pm, vec, b, lds, want, block, s);
    switch (c.G) {
        case 64: return dispatch_backward_g<64, 8, ROWPOS>(pm, vec, b, lds, want, block, s);
        case 128: return dispatch_backward_g<128, 12, ROWPOS>(pm, vec, b, lds, want, block, s);
        case 256: return dispatch_backward_g<256, 8, ROWPOS>(pm, vec, b, lds, want, block, s);
        default: return dispatch_backward_g<1024, 8, ROWPOS>(pm, vec, b, lds, want, block, s);
    }
}

}  // namespace sot
