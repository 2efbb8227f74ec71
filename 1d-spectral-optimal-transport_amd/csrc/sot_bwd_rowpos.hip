// sot_bwd_rowpos.hip -- generic backward kernels, per-row positions (sot_dispatch.hpp).
#include "sot_dispatch.hpp"

namespace sot {

template hipError_t dispatch_backward<true>(const LaunchCfg&, int, bool, const BwdArgs&, size_t, int64_t, int, hipStream_t);

}  // namespace sot
