// sot_spec_distance.hip -- MI355X (gfx950) kernels for the spectral distance of the reference's MSSLoss (losses.py:365-425;
// mean_difference, losses.py:7-36; safe_log, utils.py:145-151): over `count` magnitudes,
//   d = mag_weight * mean(D(t - v)) + logmag_weight * mean(D(slog(t) - slog(v))),  D = |.| (L1) or (.)^2 (L2),
//   slog(x) = log(x <= eps ? eps : x).
// Forward: per-workgroup fp64 partial sums (fixed assignment of elements to workgroups), a second one-workgroup kernel
// adds the partials in index order: deterministic.  Backward: elementwise.
// The magnitudes come from the STFT producer (csrc/sot_stft.hip); nothing here is a transform.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "sot_host.hpp"

namespace sot_dist {

constexpr int kThreads = 256;

struct DistArgs {
    const float* target; const float* value; int64_t count;
    float mag_weight, logmag_weight, eps; int l2;
    double* partial; int n_partial; float* out; int accumulate;   // forward; accumulate: out += d (the sum over the scales of MSSLoss)
    const float* upstream; float grad_scale;               // backward: d(loss)/d(d) as a device scalar, times grad_scale
    float* grad_target; float* grad_value;                 // either may be null
};

__device__ __forceinline__ float safe_logf(float x, float eps) { return logf(x <= eps ? eps : x); }

// (The per-element term of the two forward kernels and the per-element gradient of the two backward kernels stand in each kernel's own
// text.  As a shared __forceinline__ function the term moves the code of spec_distance_partial_kernel and of spec_distance_rows_kernel (one
// VGPR more each), the gradient that of spec_distance_backward_kernel and of spec_distance_rows_backward_kernel: each tried alone, in
// one kernel at a time.)

__global__ __launch_bounds__(kThreads) void spec_distance_partial_kernel(const DistArgs a)
{
    __shared__ double red[kThreads / 64];
    double acc_m = 0.0, acc_l = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.count; i += (int64_t)gridDim.x * kThreads) {
        const float t = a.target[i], v = a.value[i];
        if (a.mag_weight > 0.0f) { const float d = t - v; acc_m += a.l2 ? (double)(d * d) : (double)fabsf(d); }
        if (a.logmag_weight > 0.0f) { const float d = safe_logf(t, a.eps) - safe_logf(v, a.eps); acc_l += a.l2 ? (double)(d * d) : (double)fabsf(d); }
    }
    double acc = (double)a.mag_weight * acc_m + (double)a.logmag_weight * acc_l;
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) tot += red[w];
        a.partial[blockIdx.x] = tot;
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in index order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(kThreads) void spec_distance_finish_kernel(const DistArgs a)
{
    __shared__ double red[kThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < a.n_partial; i += kThreads) acc += a.partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float d = (float)(red[0] / (double)a.count);
        a.out[0] = a.accumulate ? a.out[0] + d : d;
    }
}

__global__ __launch_bounds__(kThreads) void spec_distance_backward_kernel(const DistArgs a)
{
    const float gs = a.upstream[0] * a.grad_scale / (float)a.count;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.count; i += (int64_t)gridDim.x * kThreads) {
        const float t = a.target[i], v = a.value[i];
        float gt = 0.0f, gv = 0.0f;   // d(distance * count)/dt, /dv
        if (a.mag_weight > 0.0f) {
            const float d = t - v;
            const float g = a.l2 ? 2.0f * d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));   // torch: sgn(0) = 0
            gt += a.mag_weight * g; gv -= a.mag_weight * g;
        }
        if (a.logmag_weight > 0.0f) {
            const float d = safe_logf(t, a.eps) - safe_logf(v, a.eps);
            const float g = a.l2 ? 2.0f * d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
            gt += (t <= a.eps) ? 0.0f : a.logmag_weight * g / t;    // where(x <= eps, eps, x): no gradient below eps
            gv -= (v <= a.eps) ? 0.0f : a.logmag_weight * g / v;
        }
        if (a.grad_target) a.grad_target[i] = gs * gt;
        if (a.grad_value) a.grad_value[i] = gs * gv;
    }
}

// The same distance PER ROW (MSSLoss called with dims = the two spectrogram axes: one value per clip, losses.py:406-425 with
// mean_difference's `dims`): row r owns `count` consecutive magnitudes; one workgroup per row, thread t adds elements t, t + 1024, ...
// in fp64, then a fixed tree: deterministic.  Backward: elementwise with the row's own upstream gradient.
constexpr int kRowDistThreads = 1024;
__global__ __launch_bounds__(kRowDistThreads) void spec_distance_rows_kernel(const DistArgs a)
{
    __shared__ double red[kRowDistThreads];
    const float* t_ = a.target + (int64_t)blockIdx.x * a.count;
    const float* v_ = a.value + (int64_t)blockIdx.x * a.count;
    double acc_m = 0.0, acc_l = 0.0;
    for (int64_t i = threadIdx.x; i < a.count; i += kRowDistThreads) {
        const float t = t_[i], v = v_[i];
        if (a.mag_weight > 0.0f) { const float d = t - v; acc_m += a.l2 ? (double)(d * d) : (double)fabsf(d); }
        if (a.logmag_weight > 0.0f) { const float d = safe_logf(t, a.eps) - safe_logf(v, a.eps); acc_l += a.l2 ? (double)(d * d) : (double)fabsf(d); }
    }
    red[threadIdx.x] = (double)a.mag_weight * acc_m + (double)a.logmag_weight * acc_l;
    __syncthreads();
    for (int off = kRowDistThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float d = (float)(red[0] / (double)a.count);
        a.out[blockIdx.x] = a.accumulate ? a.out[blockIdx.x] + d : d;
    }
}

__global__ __launch_bounds__(kThreads) void spec_distance_rows_backward_kernel(const DistArgs a, int64_t rows)
{
    const int64_t total = rows * a.count;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        const float gs = a.upstream[i / a.count] * a.grad_scale / (float)a.count;
        const float t = a.target[i], v = a.value[i];
        float gt = 0.0f, gv = 0.0f;
        if (a.mag_weight > 0.0f) {
            const float d = t - v;
            const float g = a.l2 ? 2.0f * d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
            gt += a.mag_weight * g; gv -= a.mag_weight * g;
        }
        if (a.logmag_weight > 0.0f) {
            const float d = safe_logf(t, a.eps) - safe_logf(v, a.eps);
            const float g = a.l2 ? 2.0f * d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
            gt += (t <= a.eps) ? 0.0f : a.logmag_weight * g / t;
            gv -= (v <= a.eps) ? 0.0f : a.logmag_weight * g / v;
        }
        if (a.grad_target) a.grad_target[i] = gs * gt;
        if (a.grad_value) a.grad_value[i] = gs * gv;
    }
}

constexpr int kDistBlocks = 1024;      // workgroups (and fp64 partial sums) of the forward over all magnitudes
constexpr int kGradBlocks = 256 * 32;  // grid cap of the elementwise backward kernels

static DistArgs dist_args(const float* target, const float* value, int64_t count, float mag_weight, float logmag_weight, float eps, int l2)
{
    DistArgs a{};
    a.target = target; a.value = value; a.count = count; a.mag_weight = mag_weight; a.logmag_weight = logmag_weight; a.eps = eps; a.l2 = l2;
    return a;
}

// grid of an elementwise backward over `elements` magnitudes
static int grad_grid(int64_t elements)
{
    const int64_t need = (elements + kThreads - 1) / kThreads;
    return (int)(need < kGradBlocks ? need : kGradBlocks);
}

}  // namespace sot_dist

extern "C" {

size_t sot_spec_distance_workspace_bytes(void) { return sizeof(double) * (size_t)sot_dist::kDistBlocks; }

int sot_spec_distance_forward(const float* target, const float* value, int64_t count, float mag_weight, float logmag_weight,
                              float eps, int l2, float* out, int accumulate, void* workspace, size_t workspace_bytes, void* stream)
{
    using namespace sot_dist;
    if (count < 1) return SOT_ERR_BAD_SHAPE;
    if (target == nullptr || value == nullptr || out == nullptr || workspace == nullptr) return SOT_ERR_NULL_POINTER;
    if (workspace_bytes < sot_spec_distance_workspace_bytes()) return SOT_ERR_WORKSPACE;
    DistArgs a = dist_args(target, value, count, mag_weight, logmag_weight, eps, l2);
    a.partial = reinterpret_cast<double*>(workspace); a.out = out; a.accumulate = accumulate;
    const int64_t need = (count + kThreads - 1) / kThreads;
    a.n_partial = (int)(need < kDistBlocks ? need : kDistBlocks);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(spec_distance_partial_kernel, dim3(a.n_partial), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(spec_distance_finish_kernel, dim3(1), dim3(kThreads), 0, st, a);
    return sot::launch_status();
}

int sot_spec_distance_backward(const float* target, const float* value, int64_t count, float mag_weight, float logmag_weight,
                               float eps, int l2, const float* upstream, float grad_scale, float* grad_target, float* grad_value,
                               void* stream)
{
    using namespace sot_dist;
    if (count < 1) return SOT_ERR_BAD_SHAPE;
    if (target == nullptr || value == nullptr || upstream == nullptr) return SOT_ERR_NULL_POINTER;
    if (grad_target == nullptr && grad_value == nullptr) return SOT_OK;
    DistArgs a = dist_args(target, value, count, mag_weight, logmag_weight, eps, l2);
    a.upstream = upstream; a.grad_scale = grad_scale; a.grad_target = grad_target; a.grad_value = grad_value;
    (void)hipGetLastError();
    hipLaunchKernelGGL(spec_distance_backward_kernel, dim3(grad_grid(count)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sot::launch_status();
}

int sot_spec_distance_rows_forward(const float* target, const float* value, int64_t rows, int64_t count_per_row, float mag_weight,
                                   float logmag_weight, float eps, int l2, float* out, int accumulate, void* stream)
{
    using namespace sot_dist;
    if (rows < 1 || count_per_row < 1 || rows > 0x7fffffff) return SOT_ERR_BAD_SHAPE;
    if (target == nullptr || value == nullptr || out == nullptr) return SOT_ERR_NULL_POINTER;
    DistArgs a = dist_args(target, value, count_per_row, mag_weight, logmag_weight, eps, l2);
    a.out = out; a.accumulate = accumulate;
    (void)hipGetLastError();
    hipLaunchKernelGGL(spec_distance_rows_kernel, dim3((unsigned)rows), dim3(kRowDistThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sot::launch_status();
}

int sot_spec_distance_rows_backward(const float* target, const float* value, int64_t rows, int64_t count_per_row, float mag_weight,
                                    float logmag_weight, float eps, int l2, const float* upstream, float grad_scale, float* grad_target,
                                    float* grad_value, void* stream)
{
    using namespace sot_dist;
    if (rows < 1 || count_per_row < 1) return SOT_ERR_BAD_SHAPE;
    if (target == nullptr || value == nullptr || upstream == nullptr) return SOT_ERR_NULL_POINTER;
    if (grad_target == nullptr && grad_value == nullptr) return SOT_OK;
    DistArgs a = dist_args(target, value, count_per_row, mag_weight, logmag_weight, eps, l2);
    a.upstream = upstream; a.grad_scale = grad_scale; a.grad_target = grad_target; a.grad_value = grad_value;
    (void)hipGetLastError();
    hipLaunchKernelGGL(spec_distance_rows_backward_kernel, dim3(grad_grid(rows * count_per_row)), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), a, rows);
    return sot::launch_status();
}

}  // extern "C"
