// Host-side helpers every translation unit of libcaster_gvp.so launches and reports through: the typed kernel launch,
// the launch status and the pointer check of the C entry points.  No device code and no GVP math: the opt-in units
// (optimizer, metrics, structure, features) include this header alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/caster_gvp.h"

// One launch of `Kernel`; returns 0, a CGVP_ERR_* code or the hipError_t of a failed attribute call.  A launch that needs
// more dynamic LDS than the 64 KB every kernel may use raises hipFuncAttributeMaxDynamicSharedMemorySize to `reserve`
// bytes first, ONCE per kernel and device (hipFuncSetAttribute is a host call of tens of microseconds; a backward pass
// made 13 of them): the static below exists per instantiation = per kernel and holds the bytes set on each device.  A
// later launch of the same kernel that asks for more than was set is refused instead of faulting on the device.
// The launch itself is not checked here: an entry point launches everything and reads launch_status() once at its end.
template <auto Kernel, class... A>
int launch_reserving(dim3 grid, dim3 block, size_t lds, size_t reserve, hipStream_t st, const A&... args) {
  if (lds > 64 * 1024) {
    static std::atomic<int> set_bytes[64];      // zero = not set on that device yet; idempotent, benign process state
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<int>& set = set_bytes[dev & 63];
    int have = set.load(std::memory_order_acquire);
    if (!have && lds <= reserve) {
      if (hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)reserve))
        return (int)err;
      set.store(have = (int)reserve, std::memory_order_release);
    }
    if (lds > (size_t)have) return CGVP_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
  return 0;
}
// the usual case: the kernel has ONE dynamic LDS size
template <auto Kernel, class... A>
int launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  return launch_reserving<Kernel>(grid, block, lds, lds, st, args...);
}

// 0, or the hipError_t of the launches since the last call.  A bad launch configuration shows here; a fault inside a
// kernel does not: it ends the process at the next synchronisation instead of reaching the caller as a code.
inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// NULL, or not aligned to `n` bytes (a power of two)
inline bool bad_ptr(const void* p, uintptr_t n) { return !p || ((uintptr_t)p & (n - 1)); }
