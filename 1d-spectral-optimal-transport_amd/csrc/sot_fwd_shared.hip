// sot_fwd_shared.hip -- generic forward kernels, shared positions, no cutoff; the quantile outputs of both cutoff flavours (sot_dispatch.hpp).
#include "sot_dispatch.hpp"

namespace sot {

SOT_FWD_SHARED_ALL(, false)
template hipError_t dispatch_forward<false>(const LaunchCfg&, bool, int, bool, const FwdArgs&, size_t, int64_t, int, hipStream_t);

}  // namespace sot
