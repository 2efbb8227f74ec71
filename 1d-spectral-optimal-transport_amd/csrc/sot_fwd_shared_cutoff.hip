// sot_fwd_shared_cutoff.hip -- generic forward kernels, shared positions, with the quantile cutoff (limit_quantile_range) (sot_dispatch.hpp).
#include "sot_dispatch.hpp"

namespace sot {

SOT_FWD_SHARED_ALL(, true)

}  // namespace sot
