// Test harness (never loaded by the product): the attention-dropout factor of csrc/gvp_rng.h compiled with g++.
#include "../../caster-dta_amd/csrc/gvp_rng.h"

// out [heads][nq][nk]: the factor of (head, q0 + i, k0 + j), q0 / k0 GLOBAL rows.  form 0: the definition, one (q, k)
// at a time; 1: the 1 x 4 key runs of the forward and d Q kernels; 2: the 4 x 1 query runs of the d K / d V kernel
// (runs start at q0 / k0, as a pair's tiles start at its first row; nq resp. nk need not be a multiple of 4).
extern "C" void host_attn_dropout(unsigned long long seed, unsigned long long offset, int stream, float p, int heads,
                                  long long q0, long long nq, long long k0, long long nk, int form, float* out) {
  const gvp::DropRule rule = gvp::drop_rule(p);
  for (int h = 0; h < heads; ++h) {
    float* o = out + (long long)h * nq * nk;
    if (form == 0) {
      for (long long i = 0; i < nq; ++i)
        for (long long j = 0; j < nk; ++j) o[i * nk + j] = gvp::attn_drop_factor(seed, offset, stream, h, q0 + i, k0 + j, rule);
    } else if (form == 1) {
      for (long long i = 0; i < nq; ++i)
        for (long long j = 0; j < nk; j += 4) {
          float f[4];
          gvp::attn_drop_run_k(seed, offset, stream, h, (uint32_t)(q0 + i), (uint32_t)((k0 + j) >> 2), (uint32_t)((k0 + j) & 3), rule, f);
          for (int r = 0; r < 4 && j + r < nk; ++r) o[i * nk + j + r] = f[r];
        }
    } else {
      for (long long i = 0; i < nq; i += 4)
        for (long long j = 0; j < nk; ++j) {
          float f[4];
          gvp::attn_drop_run_q(seed, offset, stream, h, (uint32_t)((q0 + i) >> 1), (uint32_t)((q0 + i) & 1), (uint32_t)(k0 + j), rule, f);
          for (int r = 0; r < 4 && i + r < nq; ++r) o[(i + r) * nk + j] = f[r];
        }
    }
  }
}
