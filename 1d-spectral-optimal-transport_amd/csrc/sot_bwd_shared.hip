// sot_bwd_shared.hip -- generic backward kernels, shared positions (sot_dispatch.hpp).
#include "sot_dispatch.hpp"

namespace sot {

template hipError_t dispatch_backward<false>(const LaunchCfg&, int, bool, const BwdArgs&, size_t, int64_t, int, hipStream_t);

}  // namespace sot
