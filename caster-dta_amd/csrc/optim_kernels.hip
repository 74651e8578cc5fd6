// optim_kernels.hip -- the optimizer update of a training step (include/caster_gvp_optim.h; opt-in).
//
// The reference ends every iteration with scaler.unscale_, clip_grad_norm_, scaler.step(optimizer) and
// scaler.update() (train_model.py:578-587): stock PyTorch over every parameter tensor, several multi-tensor launches
// and a host loop per step, for 764k fp32 elements -- about 21 MB of traffic, bound by launch latency.  Here it is
//
//   norm_kernel     one workgroup per CHUNK of one segment: sum of g^2 in fp64 -> partial[chunk]
//   finish_kernel   one workgroup: the partials in a fixed order -> grad_norm, found_inf, step, the loss scale and
//                   its growth tracker, and the four per-step factors the update needs (workspace)
//   apply_kernel    one workgroup per CHUNK of one segment: Adam / AdamW on p, m, v from g * inv * clip
//
// with the segment table BY VALUE in the kernel arguments and every scalar that changes between steps read from
// device memory: a captured launch replays as it is.
//
// found_inf needs no flag of its own: the square of a finite float is at most 1.2e77 in fp64, so a sum over fewer
// than 1e230 finite elements is finite, and a NaN or an Inf element makes its partial (and the total) non-finite.
//
// Every thread owns the same elements of a chunk whatever the alignment of the arrays (groups of four, 16-byte
// access where the array's address allows it, guarded scalar access elsewhere and in the tail), so the norm of the
// same values at other addresses is bitwise the same.  No access leaves [0, numel) of its segment.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/caster_gvp_optim.h"
#include "gvp_block_sum.h"
#include "gvp_host.h"

namespace {

constexpr int CHUNK = CGVP_OPTIM_CHUNK, THREADS = 256, WAVES = THREADS / 64, CAP = CGVP_OPTIM_MAX_SEGMENTS;
constexpr int GROUPS = CHUNK / (4 * THREADS);          // float4 groups per thread and chunk
static_assert(CHUNK % (4 * THREADS) == 0, "a chunk is a whole number of float4 rounds of the workgroup");

// The segments of one launch; first[i] = first chunk (= workgroup) of segment i, first[count] = chunks of the launch.
struct Table {
  cgvp_optim_segment seg[CAP];
  int32_t first[CAP + 1];
  int32_t count;
};
static_assert(sizeof(Table) + 128 <= 4096, "the table and the scalars beside it must fit the 4 KB of kernel arguments");

// What finish_kernel leaves for apply_kernel at the front of the workspace (the partials follow at kPartials).
struct StepFactors {
  float gscale;       // inv * clip
  float step_size;    // lr / (1 - beta1^step)
  float bc2_sqrt;     // sqrt(1 - beta2^step)
  float decay;        // 1 - lr * weight_decay
  int32_t skip;       // found_inf: the update does not run
};
constexpr int64_t kPartials = 64;

struct FinishArgs {
  const double* partial;
  int64_t chunks;
  StepFactors* factors;
  const float* lr;
  float* step;
  float* scale;
  int32_t* growth_tracker;
  float* grad_norm;
  float* found_inf;
  double beta1, beta2, weight_decay, max_norm, growth_factor, backoff_factor;
  int32_t growth_interval, dry;
};

struct ApplyArgs {
  const StepFactors* factors;
  float one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
  int32_t decoupled;
};

// segment of workgroup `chunk`: the last i with first[i] <= chunk (uniform over the workgroup)
__device__ inline int segment_of(const Table& t, int chunk) {
  int lo = 0, hi = t.count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.first[mid] <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// four elements at p, the first `valid` of them inside the segment (the others read as 0 and are never stored)
__device__ inline float4 load4(const float* p, bool vec, int valid) {
  if (vec && valid == 4) return *reinterpret_cast<const float4*>(p);
  float4 r;
  r.x = p[0];
  r.y = valid > 1 ? p[1] : 0.f;
  r.z = valid > 2 ? p[2] : 0.f;
  r.w = valid > 3 ? p[3] : 0.f;
  return r;
}
__device__ inline void store4(float* p, bool vec, int valid, float4 r) {
  if (vec && valid == 4) { *reinterpret_cast<float4*>(p) = r; return; }
  p[0] = r.x;
  if (valid > 1) p[1] = r.y;
  if (valid > 2) p[2] = r.z;
  if (valid > 3) p[3] = r.w;
}

__global__ __launch_bounds__(THREADS) void norm_kernel(Table t, double* __restrict__ partial) {
  const int chunk = blockIdx.x, s = segment_of(t, chunk);
  const int64_t off = (int64_t)(chunk - t.first[s]) * CHUNK, left = t.seg[s].numel - off;
  const int n = left < CHUNK ? (int)left : CHUNK;
  const float* __restrict__ g = t.seg[s].grad + off;
  const bool vec = aligned16(g);
  double acc[1] = {0.0};
#pragma unroll
  for (int k = 0; k < GROUPS; ++k) {
    const int i = 4 * (k * THREADS + (int)threadIdx.x);
    if (i < n) {
      const float4 x = load4(g + i, vec, n - i < 4 ? n - i : 4);
      acc[0] += (double)x.x * (double)x.x;
      acc[0] += (double)x.y * (double)x.y;
      acc[0] += (double)x.z * (double)x.z;
      acc[0] += (double)x.w * (double)x.w;
    }
  }
  block_sum<WAVES>(acc);                                     // fixed order (gvp_block_sum.h); valid in thread 0
  if (threadIdx.x == 0) partial[chunk] = acc[0];
}

// base^n for a whole n >= 0 by repeated squaring
__device__ inline double pow_whole(double base, uint32_t n) {
  double r = 1.0;
  for (; n; n >>= 1, base *= base)
    if (n & 1) r *= base;
  return r;
}

__global__ __launch_bounds__(THREADS) void finish_kernel(FinishArgs a) {
  double acc[1] = {0.0};
  for (int64_t i = threadIdx.x; i < a.chunks; i += THREADS) acc[0] += a.partial[i];
  block_sum<WAVES>(acc);
  if (threadIdx.x != 0) return;
  const double total = acc[0];
  const bool bad = !isfinite(total);
  const double inv = a.scale ? 1.0 / (double)a.scale[0] : 1.0;
  const double norm = inv * sqrt(total);
  a.grad_norm[0] = (float)norm;
  a.found_inf[0] = bad ? 1.f : 0.f;
  if (a.dry) return;
  StepFactors f = {0.f, 0.f, 1.f, 1.f, 1};
  if (!bad) {
    const double clip = a.max_norm > 0.0 ? fmin(1.0, a.max_norm / (norm + 1e-6)) : 1.0;
    const float step = a.step[0] + 1.f;
    const double lr = (double)a.lr[0];
    a.step[0] = step;
    f.gscale = (float)(inv * clip);
    f.step_size = (float)(lr / (1.0 - pow_whole(a.beta1, (uint32_t)step)));
    f.bc2_sqrt = (float)sqrt(1.0 - pow_whole(a.beta2, (uint32_t)step));
    f.decay = (float)(1.0 - lr * a.weight_decay);
    f.skip = 0;
  }
  *a.factors = f;
  if (a.scale) {                                             // GradScaler.update()
    if (bad) {
      a.scale[0] = (float)((double)a.scale[0] * a.backoff_factor);
      a.growth_tracker[0] = 0;
    } else {
      const int32_t good = a.growth_tracker[0] + 1;
      if (good >= a.growth_interval) {
        const float grown = (float)((double)a.scale[0] * a.growth_factor);
        if (isfinite(grown)) a.scale[0] = grown;
        a.growth_tracker[0] = 0;
      } else {
        a.growth_tracker[0] = good;
      }
    }
  }
}

__device__ inline void adam(float& p, float g, float& m, float& v, const StepFactors& f, const ApplyArgs& a) {
  g *= f.gscale;
  if (a.decoupled) p *= f.decay;
  else if (a.weight_decay != 0.f) g += a.weight_decay * p;
  m += (g - m) * a.one_minus_beta1;
  v = v * a.beta2 + a.one_minus_beta2 * g * g;
  p -= f.step_size * (m / (sqrtf(v) / f.bc2_sqrt + a.eps));
}

__global__ __launch_bounds__(THREADS) void apply_kernel(Table t, ApplyArgs a) {
  const StepFactors f = *a.factors;
  if (f.skip) return;
  const int chunk = blockIdx.x, s = segment_of(t, chunk);
  const int64_t off = (int64_t)(chunk - t.first[s]) * CHUNK, left = t.seg[s].numel - off;
  const int n = left < CHUNK ? (int)left : CHUNK;
  float* __restrict__ P = t.seg[s].param + off;
  const float* __restrict__ G = t.seg[s].grad + off;
  float* __restrict__ M = t.seg[s].exp_avg + off;
  float* __restrict__ V = t.seg[s].exp_avg_sq + off;
  const bool vp = aligned16(P), vg = aligned16(G), vm = aligned16(M), vv = aligned16(V);
#pragma unroll
  for (int k = 0; k < GROUPS; ++k) {
    const int i = 4 * (k * THREADS + (int)threadIdx.x);
    if (i < n) {
      const int valid = n - i < 4 ? n - i : 4;
      float4 p = load4(P + i, vp, valid), m = load4(M + i, vm, valid), v = load4(V + i, vv, valid);
      const float4 g = load4(G + i, vg, valid);
      adam(p.x, g.x, m.x, v.x, f, a);
      adam(p.y, g.y, m.y, v.y, f, a);
      adam(p.z, g.z, m.z, v.z, f, a);
      adam(p.w, g.w, m.w, v.w, f, a);
      store4(P + i, vp, valid, p);
      store4(M + i, vm, valid, m);
      store4(V + i, vv, valid, v);
    }
  }
}

inline int64_t chunks_of(int64_t numel) { return (numel + CHUNK - 1) / CHUNK; }

}  // namespace

extern "C" int cgvp_optim_version(void) { return CGVP_OPTIM_VERSION; }

extern "C" int64_t cgvp_optim_workspace_bytes(const int64_t* numel, int32_t num_segments) {
  if (num_segments < 0 || (num_segments > 0 && !numel)) return CGVP_ERR_BAD_ARG;
  int64_t chunks = 0;
  for (int32_t i = 0; i < num_segments; ++i) {
    if (numel[i] < 0) return CGVP_ERR_BAD_ARG;
    chunks += chunks_of(numel[i]);
    if (chunks > 0x7fffffffll) return CGVP_ERR_BAD_ARG;
  }
  return kPartials + 8 * chunks;
}

extern "C" int cgvp_optim_adam_step(const cgvp_optim_segment* segs, int32_t num_segments, const cgvp_optim_hyper* hyper,
                                    const float* lr, float* step, float* scale, int32_t* growth_tracker,
                                    float* grad_norm, float* found_inf, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  if (num_segments < 0 || (num_segments > 0 && !segs) || !hyper) return CGVP_ERR_BAD_ARG;
  const cgvp_optim_hyper& h = *hyper;
  if (!(h.beta1 >= 0.0 && h.beta1 < 1.0) || !(h.beta2 >= 0.0 && h.beta2 < 1.0) || !(h.eps >= 0.0) || h.growth_interval < 1)
    return CGVP_ERR_BAD_ARG;
  if (bad_ptr(lr, 4) || bad_ptr(step, 4) || bad_ptr(grad_norm, 4) || bad_ptr(found_inf, 4)) return CGVP_ERR_BAD_ARG;
  if ((scale == nullptr) != (growth_tracker == nullptr) || (scale && (bad_ptr(scale, 4) || bad_ptr(growth_tracker, 4)))) return CGVP_ERR_BAD_ARG;
  int64_t chunks = 0;
  for (int32_t i = 0; i < num_segments; ++i) {
    const cgvp_optim_segment& s = segs[i];
    if (s.numel < 0) return CGVP_ERR_BAD_ARG;
    if (s.numel == 0) continue;
    if (bad_ptr(s.param, 4) || bad_ptr(s.grad, 4) || bad_ptr(s.exp_avg, 4) || bad_ptr(s.exp_avg_sq, 4)) return CGVP_ERR_BAD_ARG;
    chunks += chunks_of(s.numel);
    if (chunks > 0x7fffffffll) return CGVP_ERR_BAD_ARG;
  }
  if (bad_ptr(workspace, 8) || workspace_bytes < kPartials + 8 * chunks) return CGVP_ERR_BAD_ARG;

  hipStream_t st = (hipStream_t)stream;
  StepFactors* factors = static_cast<StepFactors*>(workspace);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + kPartials);
  const ApplyArgs apply{factors, (float)(1.0 - h.beta1), (float)h.beta2, (float)(1.0 - h.beta2), (float)h.eps,
                        (float)h.weight_decay, h.decoupled ? 1 : 0};
  // pass 0: the norm partials of every table, then the scalars; pass 1: the update over the same tables
  for (int pass = 0; pass < (h.dry ? 1 : 2); ++pass) {
    Table t;
    t.count = 0;
    t.first[0] = 0;
    int64_t base = 0;                                        // chunks of the tables already launched in this pass
    for (int32_t i = 0; i <= num_segments; ++i) {
      if (i < num_segments && segs[i].numel > 0) {
        t.seg[t.count] = segs[i];
        t.first[t.count + 1] = t.first[t.count] + (int32_t)chunks_of(segs[i].numel);
        ++t.count;
      }
      if (t.count == CAP || (i == num_segments && t.count > 0)) {
        const unsigned grid = (unsigned)t.first[t.count];
        if (pass == 0) launch<norm_kernel>(dim3(grid), dim3(THREADS), 0, st, t, partial + base);
        else launch<apply_kernel>(dim3(grid), dim3(THREADS), 0, st, t, apply);
        if (const int rc = launch_status()) return rc;
        base += grid;
        t.count = 0;
      }
    }
    if (pass == 0) {
      const FinishArgs f{partial, chunks, factors, lr, step, scale, growth_tracker, grad_norm, found_inf,
                         h.beta1, h.beta2, h.weight_decay, h.max_norm, h.growth_factor, h.backoff_factor,
                         h.growth_interval, h.dry ? 1 : 0};
      launch<finish_kernel>(dim3(1), dim3(THREADS), 0, st, f);
      if (const int rc = launch_status()) return rc;
    }
  }
  return 0;
}
