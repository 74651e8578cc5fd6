// What the translation units of the varlen cross attention (attn_kernels.hip, attn_score_kernels.hip) share: the MFMA
// tile primitives, the exp that produces AND consumes the saved log-sum-exp, the tile -> pair scan, and the host checks
// of one side of one problem.  Each unit keeps its own Prob / Args and kernels in its own anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gvp_host.h"

namespace attn {

typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int WAVE = 64, TILE = 16;                               // head_dim = TILE * M

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// exp through v_exp_f32 (2^x of x * log2 e): one multiply and one transcendental instead of expf's range reduction
// (~12 VALU); every argument is <= 0 or a difference from a saved log-sum-exp, nowhere near overflow.  The kernels that
// recompute exp(s - lse) must use the function that produced the lse: this one.
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ float quad_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 16));
  return fmaxf(x, __shfl_xor(x, 32));
}
__device__ __forceinline__ float quad_sum(float x) {
  x += __shfl_xor(x, 16);
  return x + __shfl_xor(x, 32);
}

// Which pair owns tile `t` when every pair b contributes ceil((ptr[b+1] - ptr[b]) / 16) consecutive tiles?
// Wave-parallel prefix scan over the pairs, 64 at a time (B is a few dozen to a few hundred; any B).  Returns false past
// the last tile.  All lanes return the same (b, first row of the tile, end row of the pair).
__device__ __forceinline__ bool locate(const int64_t* __restrict__ ptr, int B, int t, int lane, int& b, int64_t& row0,
                                       int64_t& row_end) {
  int base = 0;
  for (int c = 0; c < B; c += WAVE) {
    const int i = c + lane;
    const int64_t lo = i < B ? ptr[i] : 0, hi = i < B ? ptr[i + 1] : 0;
    const int tiles = (int)((hi - lo + TILE - 1) / TILE);
    int incl = tiles;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int y = __shfl_up(incl, d);
      if (lane >= d) incl += y;
    }
    const int total = __shfl(incl, WAVE - 1);
    if (t < base + total) {
      const bool mine = t >= base + incl - tiles && t < base + incl;
      const unsigned long long vote = __ballot(mine);
      const int src = __ffsll((long long)vote) - 1;
      b = c + src;
      const int first = __shfl(base + incl - tiles, src);
      const int64_t plo = __shfl((long long)lo, src), phi = __shfl((long long)hi, src);
      row0 = plo + (int64_t)(t - first) * TILE;
      row_end = phi;
      return true;
    }
    base += total;
  }
  return false;
}

// The problem a wave works on, BY VALUE and selected with a wave-uniform index: `const Prob& P = a.p[pi]` with an index the
// compiler cannot prove uniform turned every P.k / P.v / ... inside the loops into a vector load of the pointer from the
// kernel-argument segment followed by s_waitcnt vmcnt(0) -- five dependent load pairs per key tile, 70-83 us per launch
// for 6 us of matrix work (profiles/r03/kernel_stats_davis_b64_joint_before.csv).
template <class Args>
__device__ __forceinline__ auto pick(const Args& a, int pi) { return pi ? a.p[1] : a.p[0]; }
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// ---- host
// One side (the query rows or the key rows) of one problem: a row count, its [B + 1] offsets, and rows of E floats that
// the kernels can address with 32-bit element offsets (a tile may start up to 16 rows behind the last one).
inline bool side_ok(int64_t rows, const int64_t* ptr, int64_t E) {
  return rows >= 0 && ptr && (rows + TILE) * E < ((int64_t)1 << 31);
}
// every pointer NULL or a multiple of `n` bytes (a power of two)
template <class... P>
bool aligned(uintptr_t n, P... p) { return (((uintptr_t)p | ...) & (n - 1)) == 0; }

// head_dim -> M: `f` is called with std::integral_constant<int, M>; any other head_dim is refused before anything else.
template <class F>
int with_m(int head_dim, F&& f) {
  switch (head_dim) {
    case 16: return f(std::integral_constant<int, 1>{});
    case 32: return f(std::integral_constant<int, 2>{});
    case 64: return f(std::integral_constant<int, 4>{});
    default: return CGVP_ERR_UNSUPPORTED_DIMS;
  }
}

}  // namespace attn
