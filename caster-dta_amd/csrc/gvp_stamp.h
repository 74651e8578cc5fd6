// gvp_stamp.h -- the -DCGVP_STAMPS diagnostic of the tile-kernel units: per-wave clock stamps into a debug buffer that
// nothing else reads (tools/stamp_*.py); without the flag every macro is a no-op and the library contains none of it.
//
// The including unit says where its stamps go BEFORE the include:
//   #define CGVP_STAMP_BUF <symbol>   its own `__device__ unsigned long long*`, declared under CGVP_STAMPS before the
//                                     include (the unit also keeps the exported setter that tools/ load by name)
//   #define CGVP_STAMP_WPB <name>     optional: waves per workgroup of STAMP / STAMP_REAL, where the unit has a constant
// Buffer layout: [wave][16] cycle stamps, wave = blockIdx.x * waves per workgroup + wave of the workgroup; behind 4096 such
// rows the wall stamps [kind][4096 waves][start, end].  Stamps are written by lane 0 with ordinary vector stores.
#pragma once

#ifdef CGVP_STAMPS
#ifndef CGVP_STAMP_WPB
#define CGVP_STAMP_WPB (blockDim.x >> 6)
#endif
#define CGVP_STAMP_WAVE ((size_t)blockIdx.x * CGVP_STAMP_WPB + (threadIdx.x >> 6))
// s_memtime: the XCD's cycle counter, after everything the wave has in flight
#define STAMP(slot)                                                                          \
  do {                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    unsigned long long t_;                                                                   \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    if (CGVP_STAMP_BUF && (threadIdx.x & 63) == 0) CGVP_STAMP_BUF[CGVP_STAMP_WAVE * 16 + (slot)] = t_; \
  } while (0)
// wall-clock stamp (s_memrealtime: 100 MHz, one counter for the whole device -- s_memtime counters are per XCD)
#define STAMP_REAL(slot)                                                                     \
  do {                                                                                       \
    unsigned long long t_;                                                                   \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");           \
    if (CGVP_STAMP_BUF && (threadIdx.x & 63) == 0) CGVP_STAMP_BUF[CGVP_STAMP_WAVE * 16 + (slot)] = t_; \
  } while (0)
// wall-clock start / end of every wave of a kernel, kept per kernel kind behind the cycle stamps:
// buffer[4096 * 16 + (kind * 4096 + wave) * 2 + {0: start, 1: end}]
struct WallStamp {
  int kind;
  __device__ __forceinline__ explicit WallStamp(int k) : kind(k) { put(0); }
  __device__ __forceinline__ ~WallStamp() { put(1); }
  __device__ __forceinline__ void put(int which) const {
    unsigned long long t_;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
    const size_t wave = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (CGVP_STAMP_BUF && (threadIdx.x & 63) == 0 && wave < 4096)
      CGVP_STAMP_BUF[4096 * 16 + ((size_t)kind * 4096 + wave) * 2 + which] = t_;
  }
};
#define WALL_STAMP(kind) WallStamp wall_stamp_(kind)
#else
#define STAMP(slot) do {} while (0)
#define STAMP_REAL(slot) do {} while (0)
#define WALL_STAMP(kind) do {} while (0)
#endif
