// Worst relative error (in units of eps = 2^-24) and worst ulp error of the device sinf / sincosf against the host double sin / cos: the source
// of U_SIN in tests/synth_model.py.  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -o sinf_accuracy tools/sinf_accuracy.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

__global__ void probe(const float* x, float* s1, float* s2, float* c2, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    s1[i] = sinf(x[i]);
    float s, c;
    sincosf(x[i], &s, &c);
    s2[i] = s; c2[i] = c;
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(r_), __LINE__); return 2; } } while (0)

int main()
{
    const int n = 1 << 25;
    std::vector<float> x(n), s1(n), s2(n), c2(n);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < n; ++i) {
        if (i < n / 2) x[i] = (float)((double)i * (1.3e5 / (n / 2)));
        else {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t r = (uint32_t)(st >> 32);
            const uint32_t e = 117 + r % 28;                      // 2^-10 ... 2^17
            const uint32_t bits = (e << 23) | ((r >> 5) & 0x7fffff);
            memcpy(&x[i], &bits, 4);
        }
    }
    float *dx, *d1, *d2, *d3;
    CK(hipMalloc(&dx, 4ull * n)); CK(hipMalloc(&d1, 4ull * n)); CK(hipMalloc(&d2, 4ull * n)); CK(hipMalloc(&d3, 4ull * n));
    CK(hipMemcpy(dx, x.data(), 4ull * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, dx, d1, d2, d3, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(s1.data(), d1, 4ull * n, hipMemcpyDeviceToHost));
    CK(hipMemcpy(s2.data(), d2, 4ull * n, hipMemcpyDeviceToHost));
    CK(hipMemcpy(c2.data(), d3, 4ull * n, hipMemcpyDeviceToHost));
    const double eps = ldexp(1.0, -24);
    const double edges[4] = {16.0, 2.2e4, 1.3e5, 3e5};
    double rel[4][3] = {}, ulp[4][3] = {};
    float argmax[4][3] = {};
    for (int i = 0; i < n; ++i) {
        const double xs = (double)x[i], es = sin(xs), ec = cos(xs);
        int r = 0;
        while (r < 3 && xs > edges[r]) ++r;
        const double got[3] = {(double)s1[i], (double)s2[i], (double)c2[i]}, want[3] = {es, es, ec};
        for (int j = 0; j < 3; ++j) {
            if (want[j] == 0.0) continue;
            const double err = fabs(got[j] - want[j]);
            int ex; frexp(want[j], &ex);
            const double u = err / ldexp(1.0, ex - 24), rl = err / (eps * fabs(want[j]));
            if (rl > rel[r][j]) { rel[r][j] = rl; argmax[r][j] = x[i]; }
            if (u > ulp[r][j]) ulp[r][j] = u;
        }
    }
    const char* names[3] = {"sinf", "sincosf.sin", "sincosf.cos"};
    for (int r = 0; r < 4; ++r)
        for (int j = 0; j < 3; ++j)
            printf("x <= %-8g %-12s worst rel err / eps %.4f (at x = %.9g)   worst ulp %.4f\n", edges[r], names[j], rel[r][j], argmax[r][j], ulp[r][j]);
    return 0;
}
