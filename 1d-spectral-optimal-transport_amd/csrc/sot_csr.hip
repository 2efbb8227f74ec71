// sot_csr.hip -- CSR (ragged) forward: the generic per-row-position kernels with row offsets, and its C entry point.
#include "sot_launch.hpp"

namespace sot {

// ---- CSR (ragged) forward: BASELINE config 4's second input form ---------------------------------------------
template <int G, int CPT, int PM, bool LIM>
static hipError_t launch_forward_csr(const FwdArgs& a, size_t lds, int64_t want, int block, hipStream_t s)
{
    return launch_persistent<sot_forward_kernel<G, CPT, true, false, PM, LIM, false, true>>(a, lds, want, block, s);
}

template <int G, int CPT>
static hipError_t dispatch_forward_csr_g(int pm, bool lim, const FwdArgs& a, size_t lds, int64_t want, int block, hipStream_t s)
{
    if (lim) {
        switch (pm) {
            case 1: return launch_forward_csr<G, CPT, 1, true>(a, lds, want, block, s);
            case 2: return launch_forward_csr<G, CPT, 2, true>(a, lds, want, block, s);
            default: return launch_forward_csr<G, CPT, 0, true>(a, lds, want, block, s);
        }
    }
    switch (pm) {
        case 1: return launch_forward_csr<G, CPT, 1, false>(a, lds, want, block, s);
        case 2: return launch_forward_csr<G, CPT, 2, false>(a, lds, want, block, s);
        default: return launch_forward_csr<G, CPT, 0, false>(a, lds, want, block, s);
    }
}

int run_forward_csr(const float* xw, const float* xp, const int64_t* xoff, int64_t x_nnz, const float* yw, const float* yp,
                    const int64_t* yoff, int64_t y_nnz, int64_t B, int max_n, int max_m, float p, uint32_t flags, float* row_loss,
                    void* stream)
{
    if (!(p >= 1.0f)) return SOT_ERR_INVALID_P;
    if (B < 0 || max_n < 1 || max_m < 1 || x_nnz < 1 || y_nnz < 1) return SOT_ERR_BAD_SHAPE;
    if (B == 0) return SOT_OK;
    if (!xw || !xp || !xoff || !yw || !yp || !yoff || !row_loss) return SOT_ERR_NULL_POINTER;
    LaunchCfg cfg; size_t lds = 0; int block = 0, rpw = 1;
    if (!pick_cfg(max_n, max_m, true, false, &cfg, &lds, &block, &rpw)) return SOT_ERR_UNSUPPORTED_SIZE;
    FwdArgs a{};
    a.x = xw; a.y = yw; a.xpos = xp; a.ypos = yp; a.xoff = xoff; a.yoff = yoff;
    a.B = B; a.n = max_n; a.m = max_m;
    a.p = p; a.flags = flags; a.row_loss = row_loss;
    const int pm = (p == 1.0f) ? 1 : ((p == 2.0f) ? 2 : 0);
    const bool lim = flags & SOT_FLAG_LIMIT_Q;
    const int64_t want = (B + rpw - 1) / rpw;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t e;
    if (cfg.CPT == 16) e = dispatch_forward_csr_g<1024, 16>(pm, lim, a, lds, want, block, s);
    else if (cfg.G == 64) e = dispatch_forward_csr_g<64, 8>(pm, lim, a, lds, want, block, s);
    else if (cfg.G == 128) e = dispatch_forward_csr_g<128, 12>(pm, lim, a, lds, want, block, s);
    else if (cfg.G == 256) e = dispatch_forward_csr_g<256, 8>(pm, lim, a, lds, want, block, s);
    else e = dispatch_forward_csr_g<1024, 8>(pm, lim, a, lds, want, block, s);
    return launch_status(e);
}

}  // namespace sot

extern "C" int sot_w1d_forward_csr(const float* x_weights, const float* x_positions, const int64_t* x_offsets, int64_t x_nnz,
                                   const float* y_weights, const float* y_positions, const int64_t* y_offsets, int64_t y_nnz,
                                   int64_t B, int32_t max_n, int32_t max_m, float p, uint32_t flags, float* row_loss, void* stream)
{
    return sot::run_forward_csr(x_weights, x_positions, x_offsets, x_nnz, y_weights, y_positions, y_offsets, y_nnz, B, max_n,
                                max_m, p, flags, row_loss, stream);
}
