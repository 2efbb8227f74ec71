// sot_fwd_rowpos.hip -- generic forward kernels, per-row positions (sot_dispatch.hpp).
#include "sot_dispatch.hpp"

namespace sot {

template hipError_t dispatch_forward<true>(const LaunchCfg&, bool, int, bool, const FwdArgs&, size_t, int64_t, int, hipStream_t);

}  // namespace sot
