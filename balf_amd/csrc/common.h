// Shared helpers for the gfx950 kernels of libbalf_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

#include "../../include/balf_hip.h"

#define BALF_LAUNCH_CHECK()                      \
    do {                                         \
        if (hipGetLastError() != hipSuccess)     \
            return BALF_ERR_LAUNCH;              \
    } while (0)

static inline int balf_ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
static inline size_t balf_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Bump allocator over a workspace: slices of 256-byte granularity in call order.  `used` is the layout's size so far (start it
// at a byte offset to continue a layout); base == nullptr sizes a layout without handing out pointers.  A unit states its layout
// ONCE, in a function that walks a cursor and that both its size query and its entry point call.
struct WorkspaceCursor {
    char *base;
    size_t used;
    size_t offset(size_t bytes) { const size_t at = used; used += balf_align_up(bytes, 256); return at; }
    template <typename T> T *take(size_t bytes) { const size_t at = offset(bytes); return base ? reinterpret_cast<T *>(base + at) : nullptr; }
    // the LAST slice of a layout whose documented total ends on the slice's own bytes, not on the next 256
    template <typename T> T *take_exact(size_t bytes) { T *p = take<T>(0); used += bytes; return p; }
};

// Opt-in for `bytes` of dynamic LDS at the launches of Kernel on the current device.  Up to 48 KiB a kernel needs none, and the
// call costs nothing.  Above that, hipFuncSetAttribute is a driver round trip (tens of microseconds), so the largest size granted
// so far is kept per kernel and device, and the driver is asked only by a launch that needs more than that.  False: the driver
// refused, or the device index is outside the table.
template <auto Kernel>
bool balf_allow_dynamic_lds(int bytes) {
    if (bytes <= 48 * 1024) return true;
    static std::atomic<int> granted[64];                         // [device]; zero-initialised
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (bytes <= granted[dev].load(std::memory_order_acquire)) return true;
    static std::mutex grow;                                      // the driver keeps the LAST size set: growing is serialised
    std::lock_guard<std::mutex> lock(grow);
    if (bytes <= granted[dev].load(std::memory_order_relaxed)) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    granted[dev].store(bytes, std::memory_order_release);
    return true;
}

// 32-bit fill as a KERNEL of the library's own (nms_topk.hip).  Not hipMemsetAsync: a memset node captured from it into a hipGraph
// (torch.cuda.graph) on ROCm 7.0 clears correctly on the FIRST replay and writes a garbage value from the second replay on
// (tools/memset_capture_probe.py: 0, then 2046820352) -- the NMS counters of a replayed pipeline then sent stores out of bounds.
// A kernel node carries its arguments by value like every other launch.
int balf_fill_u32(void *dst_dev, unsigned value, size_t n_words, hipStream_t stream);
