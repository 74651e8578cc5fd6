// metrics_kernels.hip -- the evaluation metrics of a run (include/caster_gvp_metrics.h; opt-in).
//
// The reference reads a loss back from the device after every batch (train_model.py:609-631, 645-674) and ends a run
// with a Python double loop over all pairs of test rows for the concordance index (train_model.py:773-790, "very
// slow" by its own comment).  Here
//
//   reset_kernel     one thread: the append state {rows stored, rows dropped} = 0
//   append_kernel    one workgroup: a batch of (prediction, target) rows behind the cursor the state holds
//   moments1_kernel  one workgroup per CHUNK rows: fp64 sums of p, t, (p - t)^2, |p - t| -> partial
//   means_kernel     one workgroup: those partials in a fixed order -> the two means, mse, mae (workspace)
//   moments2_kernel  one workgroup per CHUNK rows: fp64 sums of p~^2, t~^2, p~ t~ (centred) -> partial
//   pair_kernel      one workgroup per tile pair (bi >= bj) of the lower triangle, TILE rows a side: each thread keeps
//                    its row (t_i, p_i) in registers, the other tile's (t_j, p_j) are staged once in LDS as float2 and
//                    read as broadcasts; 32-bit counters per thread, 64-bit per workgroup -> partial
//   finish_kernel    one workgroup: the partials in a fixed order -> out_counts, out_vals
//
// with the row count read from device memory by every kernel: the grids are sized from the capacity, workgroups
// beyond the count exit, and a captured launch replays as it is.  No atomics anywhere: the floating-point sums have
// a fixed order, the integer sums need none.  No access leaves [0, n) of the two arrays, and rows of a partial tile
// that lie behind n enter the count as a NaN target, which no comparison accepts.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/caster_gvp_metrics.h"
#include "gvp_block_sum.h"
#include "gvp_host.h"

namespace {

constexpr int TILE = CGVP_METRICS_TILE, CHUNK = CGVP_METRICS_CHUNK, THREADS = 256, WAVES = THREADS / 64;
constexpr int64_t MAX_ROWS = CGVP_METRICS_MAX_ROWS;
// Most workgroups of the pair count; a triangle with more tile pairs is walked with this stride.
constexpr int64_t PAIR_GRID = 65536;
static_assert(TILE == THREADS, "one thread per row of a tile");
static_assert(CHUNK % THREADS == 0, "a chunk is a whole number of rounds of the workgroup");
// a thread counts at most TILE pairs per tile pair: its 32-bit counters hold the longest walk
static_assert(((MAX_ROWS / TILE) * (MAX_ROWS / TILE + 1) / 2 / PAIR_GRID + 1) * TILE < (int64_t(1) << 32), "counter width");

// What means_kernel leaves at the front of the workspace; the partials follow at kPartials.
struct Means {
  double mean_p, mean_t, mse, mae;
};
constexpr int64_t kPartials = 64;

typedef unsigned long long u64;

__device__ inline int64_t rows_of(const int64_t* count_dev, int64_t max_rows) {
  if (!count_dev) return max_rows;
  const int64_t n = count_dev[0];
  return n < 0 ? 0 : (n > max_rows ? max_rows : n);
}

__global__ void reset_kernel(int64_t* __restrict__ state) {
  state[0] = 0;
  state[1] = 0;
}

__global__ __launch_bounds__(THREADS) void append_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                         int64_t n, float* __restrict__ pred_buf,
                                                         float* __restrict__ target_buf, int64_t capacity,
                                                         int64_t* __restrict__ state, int32_t dry) {
  if (dry) return;
  int64_t cursor = state[0];
  cursor = cursor < 0 ? 0 : (cursor > capacity ? capacity : cursor);
  __syncthreads();                                           // every thread has the cursor of BEFORE this append
  const int64_t room = capacity - cursor, stored = n < room ? n : room;
  for (int64_t k = threadIdx.x; k < stored; k += THREADS) {
    pred_buf[cursor + k] = pred[k];
    target_buf[cursor + k] = target[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    state[0] = cursor + stored;
    state[1] += n - stored;
  }
}

__global__ __launch_bounds__(THREADS) void moments1_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           const int64_t* __restrict__ count_dev, int64_t max_rows,
                                                           double* __restrict__ partial) {
  const int64_t n = rows_of(count_dev, max_rows), base = (int64_t)blockIdx.x * CHUNK;
  if (base >= n) return;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < CHUNK / THREADS; ++k) {
    const int64_t i = base + k * THREADS + (int)threadIdx.x;
    if (i < n) {
      const double p = (double)pred[i], t = (double)target[i], d = p - t;
      acc[0] += p;
      acc[1] += t;
      acc[2] += d * d;
      acc[3] += fabs(d);
    }
  }
  block_sum<WAVES>(acc);
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) partial[4 * (int64_t)blockIdx.x + k] = acc[k];
}

__global__ __launch_bounds__(THREADS) void means_kernel(const double* __restrict__ partial,
                                                        const int64_t* __restrict__ count_dev, int64_t max_rows,
                                                        Means* __restrict__ means) {
  const int64_t n = rows_of(count_dev, max_rows), chunks = (n + CHUNK - 1) / CHUNK;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t c = threadIdx.x; c < chunks; c += THREADS)
    for (int k = 0; k < 4; ++k) acc[k] += partial[4 * c + k];
  block_sum<WAVES>(acc);
  if (threadIdx.x != 0) return;
  const double rows = (double)n;                             // n == 0: 0 / 0 = NaN, as the header says
  means->mean_p = acc[0] / rows;
  means->mean_t = acc[1] / rows;
  means->mse = acc[2] / rows;
  means->mae = acc[3] / rows;
}

__global__ __launch_bounds__(THREADS) void moments2_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           const int64_t* __restrict__ count_dev, int64_t max_rows,
                                                           const Means* __restrict__ means, double* __restrict__ partial) {
  const int64_t n = rows_of(count_dev, max_rows), base = (int64_t)blockIdx.x * CHUNK;
  if (base >= n) return;
  const double mean_p = means->mean_p, mean_t = means->mean_t;
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < CHUNK / THREADS; ++k) {
    const int64_t i = base + k * THREADS + (int)threadIdx.x;
    if (i < n) {
      const double p = (double)pred[i] - mean_p, t = (double)target[i] - mean_t;
      acc[0] += p * p;
      acc[1] += t * t;
      acc[2] += p * t;
    }
  }
  block_sum<WAVES>(acc);
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; ++k) partial[3 * (int64_t)blockIdx.x + k] = acc[k];
}

__host__ __device__ inline int64_t triangle(int64_t tiles) { return tiles * (tiles + 1) / 2; }

// The pairs of this thread's row (t, p) with rows [0, count) of the staged tile; DIAG: only those with j < lim.
template <bool DIAG>
__device__ inline void count_tile(const float2* __restrict__ other, int count, int lim, float t, float p,
                                  uint32_t& concordant, uint32_t& tied, uint32_t& comparable) {
#pragma unroll 8
  for (int j = 0; j < count; ++j) {
    const float2 o = other[j];                               // the same address in every lane: a broadcast
    bool gt = t > o.x, lt = t < o.x;
    if (DIAG) {
      gt = gt && j < lim;
      lt = lt && j < lim;
    }
    const bool both = gt | lt;
    comparable += both ? 1u : 0u;
    concordant += ((gt & (p > o.y)) | (lt & (p < o.y))) ? 1u : 0u;
    tied += (both & (p == o.y)) ? 1u : 0u;
  }
}

__global__ __launch_bounds__(THREADS) void pair_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const int64_t* __restrict__ count_dev, int64_t max_rows,
                                                       int64_t* __restrict__ partial) {
  __shared__ float2 other[TILE];
  const int64_t n = rows_of(count_dev, max_rows), tiles = (n + TILE - 1) / TILE, tile_pairs = triangle(tiles);
  if ((int64_t)blockIdx.x >= tile_pairs) return;
  const float nan = __int_as_float(0x7fc00000);
  const int lane_row = (int)threadIdx.x;
  uint32_t concordant = 0, tied = 0, comparable = 0;
  for (int64_t q = blockIdx.x; q < tile_pairs; q += gridDim.x) {
    // q = triangle(bi) + bj with bj <= bi
    int64_t bi = (int64_t)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while (triangle(bi) > q) --bi;
    while (triangle(bi + 1) <= q) ++bi;
    const int64_t bj = q - triangle(bi), i = bi * TILE + lane_row, j = bj * TILE + lane_row;
    const float t = i < n ? target[i] : nan, p = i < n ? pred[i] : 0.f;
    __syncthreads();                                         // the readers of the tile before are done
    other[lane_row] = j < n ? make_float2(target[j], pred[j]) : make_float2(nan, 0.f);
    __syncthreads();
    if (bi == bj) {
      const int upto = 64 * (lane_row / 64 + 1);             // uniform over the wave: no row of it has j beyond
      count_tile<true>(other, upto < TILE ? upto : TILE, lane_row, t, p, concordant, tied, comparable);
    } else {
      count_tile<false>(other, TILE, TILE, t, p, concordant, tied, comparable);
    }
  }
  u64 acc[3] = {concordant, tied, comparable};
  block_sum<WAVES>(acc);
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; ++k) partial[3 * (int64_t)blockIdx.x + k] = (int64_t)acc[k];
}

__global__ __launch_bounds__(THREADS) void finish_kernel(const double* __restrict__ moments, const int64_t* __restrict__ pairs,
                                                         int64_t pair_grid, const Means* __restrict__ means,
                                                         const int64_t* __restrict__ count_dev, int64_t max_rows,
                                                         int64_t* __restrict__ out_counts, double* __restrict__ out_vals) {
  const int64_t n = rows_of(count_dev, max_rows), chunks = (n + CHUNK - 1) / CHUNK;
  const int64_t tile_pairs = triangle((n + TILE - 1) / TILE), used = tile_pairs < pair_grid ? tile_pairs : pair_grid;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t c = threadIdx.x; c < chunks; c += THREADS)
    for (int k = 0; k < 3; ++k) acc[k] += moments[3 * c + k];
  block_sum<WAVES>(acc);
  u64 cnt[3] = {0, 0, 0};
  for (int64_t g = threadIdx.x; g < used; g += THREADS)
    for (int k = 0; k < 3; ++k) cnt[k] += (u64)pairs[3 * g + k];
  block_sum<WAVES>(cnt);
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t concordant = (int64_t)cnt[0], tied = (int64_t)cnt[1], comparable = (int64_t)cnt[2];
  out_counts[0] = n;
  out_counts[1] = concordant;
  out_counts[2] = tied;
  out_counts[3] = comparable;
  if (n == 0) {
    out_vals[0] = out_vals[1] = out_vals[2] = out_vals[4] = out_vals[5] = nan;
    out_vals[3] = 0.0;
    return;
  }
  out_vals[0] = means->mse;
  out_vals[1] = means->mae;
  out_vals[2] = (acc[0] == 0.0 || acc[1] == 0.0) ? nan : acc[2] / sqrt(acc[0] * acc[1]);
  out_vals[3] = comparable ? ((double)concordant + 0.5 * (double)tied) / (double)comparable : 0.0;
  out_vals[4] = means->mean_p;
  out_vals[5] = means->mean_t;
}

inline int64_t chunks_of(int64_t rows) { return (rows + CHUNK - 1) / CHUNK; }

inline int64_t pair_grid_of(int64_t rows) {
  const int64_t tile_pairs = triangle((rows + TILE - 1) / TILE);
  return tile_pairs < PAIR_GRID ? tile_pairs : PAIR_GRID;
}

// byte offsets behind the Means block: [chunks x 4 doubles | chunks x 3 doubles | pair_grid x 3 int64]
inline int64_t workspace_of(int64_t rows) { return kPartials + 8 * (7 * chunks_of(rows) + 3 * pair_grid_of(rows)); }

}  // namespace

extern "C" int cgvp_metrics_version(void) { return CGVP_METRICS_VERSION; }

extern "C" int cgvp_metrics_reset(int64_t* state, void* stream) {
  if (bad_ptr(state, 8)) return CGVP_ERR_BAD_ARG;
  launch<reset_kernel>(dim3(1), dim3(1), 0, (hipStream_t)stream, state);
  return launch_status();
}

extern "C" int cgvp_metrics_append(const float* pred, const float* target, int64_t n, float* pred_buf, float* target_buf,
                                   int64_t capacity, int64_t* state, int32_t dry, void* stream) {
  if (n < 0 || capacity < 0 || capacity > MAX_ROWS || bad_ptr(state, 8)) return CGVP_ERR_BAD_ARG;
  if (n > 0 && (bad_ptr(pred, 4) || bad_ptr(target, 4))) return CGVP_ERR_BAD_ARG;
  if (capacity > 0 ? (bad_ptr(pred_buf, 4) || bad_ptr(target_buf, 4)) : (((uintptr_t)pred_buf | (uintptr_t)target_buf) & 3) != 0)
    return CGVP_ERR_BAD_ARG;
  if (n == 0) return 0;
  launch<append_kernel>(dim3(1), dim3(THREADS), 0, (hipStream_t)stream, pred, target, n, pred_buf, target_buf,
                        capacity, state, dry ? 1 : 0);
  return launch_status();
}

extern "C" int64_t cgvp_metrics_workspace_bytes(int64_t max_rows) {
  if (max_rows < 0 || max_rows > MAX_ROWS) return CGVP_ERR_BAD_ARG;
  return workspace_of(max_rows);
}

extern "C" int cgvp_metrics_compute(const float* pred_buf, const float* target_buf, const int64_t* count_dev,
                                    int64_t max_rows, int64_t* out_counts, double* out_vals, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  if (max_rows < 0 || max_rows > MAX_ROWS) return CGVP_ERR_BAD_ARG;
  if (max_rows > 0 ? (bad_ptr(pred_buf, 4) || bad_ptr(target_buf, 4)) : (((uintptr_t)pred_buf | (uintptr_t)target_buf) & 3) != 0)
    return CGVP_ERR_BAD_ARG;
  if ((count_dev && bad_ptr(count_dev, 8)) || bad_ptr(out_counts, 8) || bad_ptr(out_vals, 8)) return CGVP_ERR_BAD_ARG;
  if (bad_ptr(workspace, 8) || workspace_bytes < workspace_of(max_rows)) return CGVP_ERR_BAD_ARG;

  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = chunks_of(max_rows), pair_grid = pair_grid_of(max_rows);
  Means* means = static_cast<Means*>(workspace);
  double* part1 = reinterpret_cast<double*>(static_cast<char*>(workspace) + kPartials);
  double* part2 = part1 + 4 * chunks;
  int64_t* pairs = reinterpret_cast<int64_t*>(part2 + 3 * chunks);
  if (max_rows > 0) {
    launch<moments1_kernel>(dim3((unsigned)chunks), dim3(THREADS), 0, st, pred_buf, target_buf, count_dev,
                            max_rows, part1);
    if (const int rc = launch_status()) return rc;
    launch<means_kernel>(dim3(1), dim3(THREADS), 0, st, part1, count_dev, max_rows, means);
    if (const int rc = launch_status()) return rc;
    launch<moments2_kernel>(dim3((unsigned)chunks), dim3(THREADS), 0, st, pred_buf, target_buf, count_dev,
                            max_rows, means, part2);
    if (const int rc = launch_status()) return rc;
    launch<pair_kernel>(dim3((unsigned)pair_grid), dim3(THREADS), 0, st, pred_buf, target_buf, count_dev,
                        max_rows, pairs);
    if (const int rc = launch_status()) return rc;
  }
  launch<finish_kernel>(dim3(1), dim3(THREADS), 0, st, part2, pairs, pair_grid, means, count_dev, max_rows,
                        out_counts, out_vals);
  return launch_status();
}
