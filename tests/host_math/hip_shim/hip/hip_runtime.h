// Just enough of the HIP built-ins to compile a kernel that uses none of the hardware (no LDS, no shuffles, no atomics)
// with g++ and run it lane by lane on the CPU, under the host sanitizers.  Test scaffolding (tests/host_math/
// host_resident.cpp), never part of the product.
#pragma once
#include <cstddef>
#include <cstdint>
#define __device__
#define __global__
#define __host__
#define __launch_bounds__(...)
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct alignas(16) uint4 { uint32_t x, y, z, w; };       // alignas: UBSan reports a 16-byte access that is not aligned
struct alignas(16) longlong2 { long long x, y; };
inline dim3 threadIdx, blockIdx, gridDim, blockDim;
typedef void* hipStream_t;
typedef int hipError_t;
constexpr int hipSuccess = 0;
constexpr int hipFuncAttributeMaxDynamicSharedMemorySize = 0;
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return 0; }
// a launch = every lane of every workgroup, one after the other
#define hipLaunchKernelGGL(K, grid, block, lds, st, ...)   \
  do {                                                     \
    gridDim = grid;                                        \
    blockDim = block;                                      \
    for (unsigned bx_ = 0; bx_ < gridDim.x; ++bx_)         \
      for (unsigned tx_ = 0; tx_ < blockDim.x; ++tx_) {    \
        blockIdx.x = bx_;                                  \
        threadIdx.x = tx_;                                 \
        K(__VA_ARGS__);                                    \
      }                                                    \
  } while (0)
