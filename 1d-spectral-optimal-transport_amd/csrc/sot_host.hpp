// sot_host.hpp -- the host launch layer of EVERY object of the library: the LDS limit and its opt-in, the CU count, grids capped by
// what is resident, the launch of a persistent kernel and the status of a launch.  Host code only: no kernel and no device function is
// declared here, so the signal objects (sot_stft, sot_mss, sot_osc, sot_fir) include it without the row kernels; the row-kernel objects
// get it through sot_launch.hpp.  Everything is static inline or a template: the objects are linked into one library, also in mixed variants.
//
// Launch state is kept PER DEVICE and is safe against concurrent callers: a process may use several GPUs (the binding switches devices
// per call), and calls arrive from several host threads (autograd runs backward on its own thread; ctypes drops the GIL).
// A new launch site copies from here: allow_full_lds_once<kernel>() where the kernel's dynamic LDS may pass 64 KiB, capped_grid() or
// launch_persistent<kernel>() for the grid, launch_status() for the return value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>

#include "../../include/sot_hip.h"

namespace sot {

constexpr size_t kLdsLimit = 160 * 1024;
constexpr int kMaxDevices = 64;

static inline int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    return dev;
}

// SOT_OK when `e` -- by default the runtime's last error, which this clears -- is hipSuccess.  A launch site clears a stale error with
// (void)hipGetLastError() BEFORE its launches and returns launch_status() after them.
static inline int launch_status(hipError_t e = hipGetLastError()) { return e == hipSuccess ? SOT_OK : SOT_ERR_LAUNCH; }

// CUs of the current device (256 where the runtime cannot tell); leaves no sticky error behind.
static inline int device_cu_count()
{
    static std::atomic<int> cus[kMaxDevices];   // zero-initialised; written with the same value by whoever gets there first
    const int dev = current_device();
    const bool cacheable = dev >= 0 && dev < kMaxDevices;
    int n = cacheable ? cus[dev].load(std::memory_order_relaxed) : 0;
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) { (void)hipGetLastError(); n = 256; }
    if (cacheable) cus[dev].store(n, std::memory_order_relaxed);
    return n;
}

// Grid of a kernel whose workgroups stride over `groups` units of work, `per_cu` of them resident on a CU.
static inline int capped_grid(int64_t groups, int per_cu)
{
    const int64_t cap = (int64_t)device_cu_count() * per_cu;
    return (int)(groups < cap ? groups : cap);
}

// Allow a kernel to use up to the CU's full 160 KiB of dynamic LDS; leaves no sticky error behind.
static inline void allow_full_lds(const void* kernel)
{
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit) != hipSuccess)
        (void)hipGetLastError();
}

// Per-device launch state of ONE kernel instantiation: the full-LDS opt-in (hipFuncSetAttribute applies to the current device only) and
// its resident grid (per LDS size: the generic kernels' LDS request depends on n, m).  The mutex is held across the runtime calls, so a
// second thread never launches before the first one's opt-in is in place.  Owned by the function templates below, one per kernel.
struct GridCache {
    std::mutex mu;
    struct Entry { size_t lds; int grid; bool attr; } e[kMaxDevices] = {};
};

// Once per device: opt the kernel `Kern` in to the full LDS, before its first launch there (kernels launched with a grid of their own).
template <auto Kern>
static inline void allow_full_lds_once()
{
    static GridCache gc;   // function-local static: thread-safe initialisation
    const void* kernel = reinterpret_cast<const void*>(Kern);
    const int dev = current_device();
    if (dev < 0 || dev >= kMaxDevices) { allow_full_lds(kernel); return; }
    std::lock_guard<std::mutex> lock(gc.mu);
    if (!gc.e[dev].attr) { allow_full_lds(kernel); gc.e[dev].attr = true; }
}

// Persistent grid: exactly as many workgroups as are co-resident (registers, LDS and wave slots all
// taken into account by the occupancy query), never more than there are row groups.
template <typename Kernel>
static inline int resident_grid(Kernel kern, int block, size_t lds, int64_t want)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, block, lds) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    return capped_grid(want, per_cu);
}

// Grid of a persistent kernel whose workgroups stride over `want` row groups, at most `cap` of them resident (some run one
// round more: splitting the rows evenly over fewer workgroups was measured 5 % slower for the training form).
static inline int persistent_grid(int64_t want, int cap)
{
    return want <= cap ? (int)want : cap;
}

// resident_grid() of one kernel instantiation, cached per device and LDS size; the first use on a device also opts the kernel in to
// the CU's full LDS there.
template <typename Kernel>
static inline int cached_resident_grid(GridCache& gc, Kernel kern, int block, size_t lds)
{
    const int dev = current_device();
    if (dev < 0 || dev >= kMaxDevices) {
        allow_full_lds(reinterpret_cast<const void*>(kern));
        return resident_grid(kern, block, lds, INT32_MAX);
    }
    std::lock_guard<std::mutex> lock(gc.mu);
    GridCache::Entry& e = gc.e[dev];
    if (!e.attr) { allow_full_lds(reinterpret_cast<const void*>(kern)); e.attr = true; }
    if (e.grid == 0 || e.lds != lds) { e.grid = resident_grid(kern, block, lds, INT32_MAX); e.lds = lds; }
    return e.grid;
}

// The launch of a persistent kernel: its grid of resident workgroups from a cache of its own (one per kernel `Kern`, per device inside),
// never more workgroups than the `want` row groups, and the launch's own error.
template <auto Kern, class Args>
static inline hipError_t launch_persistent(const Args& args, size_t lds, int64_t want, int block, hipStream_t s)
{
    static GridCache cache;
    const int grid = persistent_grid(want, cached_resident_grid(cache, Kern, block, lds));
    (void)hipGetLastError();  // do not inherit a stale error from earlier runtime calls
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), lds, s, args);
    return hipGetLastError();
}

}  // namespace sot
