// graph_index_kernels.hip -- the integer-only graph-index code of libcaster_gvp.so: the library's zero fill, the
// dst-sorted CSR build (a stable counting sort of the edges by target in four launches: count, scan, fill, rank), the
// source-order index of the deterministic mode (the same sort by source, over the sorted positions) and the per-batch
// collate of per-graph CSR tables.  No GVP arithmetic, no floats.  Callers: the whole-pass entry points of pass_api.hip
// (quad::csr_build; in a training pass cgvp_lba_pass_begin's fused count has done the count launch's work), the
// deterministic backward (quad::src_index) and the four C entry points at the end; quad::zero_words serves every unit.
#include "gvp_internal.h"

namespace {

constexpr int WAVE = 64;

// ------------------------------------------------------------------ CSR build
// Stable counting sort of the edges by target in four launches:
//   count  : cnt[dst] += 1                                     (int atomics, one thread per edge)
//   scan   : exclusive scan of cnt -> rowptr; cnt is left as it is     (N <= 64k: independent 1024-entry workgroups, each
//            sums the counts before its chunk itself; longer tables: ONE block, LDS tiles with a carry)
//   fill   : pos = rowptr[dst] + --cnt[dst] -> tmp[pos] = edge id, edst[pos] = dst   (reverse arrival order inside a
//            segment; the counters count back down to the all-zero state the next call expects)
//   rank   : every position ranks its edge id inside its segment (deg reads, all independent) and writes
//            eperm / esrc at the ranked position: segments end up ordered by edge id = the reference's index_add
//            order, run-to-run reproducible; the same launch zeroes the counters again for the next call.
// Zero fill by a kernel of our own.  hipMemsetAsync is NOT used anywhere in this library: captured into a HIP graph, a
// memset of a size that is not a multiple of 256 B (the runtime splits it into body + tail fills) left the buffer
// un-zeroed on the second and later replays on this ROCm build (round 2: the GINE input gradients turned into garbage from
// replay 1 on; tests/test_hip_models.py::test_joint_training_step_replays_from_a_hip_graph).
__global__ void zero_words_kernel(uint32_t* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}

// (pass_begin_kernel of gvp_quad_kernels.hip carries a copy of this edge test and count: keep the two alike)
__global__ void csr_count_kernel(const int64_t* __restrict__ ei, int64_t N, int64_t E,
                                 int32_t* __restrict__ cnt, unsigned long long* rng_state, unsigned long long* rng_out) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (rng_state && e == 0) {             // optional: advance the persistent dropout generator (cgvp_rng_next's work)
    const unsigned long long off = rng_state[1] + 1;
    rng_state[1] = off;
    rng_out[0] = rng_state[0];
    rng_out[1] = off;
  }
  if (e >= E) return;
  int64_t s = ei[e], d = ei[E + e];
  if (s < 0 || s >= N || d < 0 || d >= N) return;   // malformed edge: dropped, never faults
  atomicAdd(&cnt[d], 1);
}

// Exclusive scan of cnt[0..N) by ONE 1024-thread block; rowptr[N] = total.  The table goes through LDS in tiles of
// SCAN_LDS entries (coalesced global traffic both ways) with a running carry, so long tables cost tiles x the
// short-table time, not a strided crawl.  Tables of at most SCAN_MULTI_MAX entries take csr_scan_multi_kernel below.
constexpr int SCAN_LDS = 36 * 1024;   // 144 KB of the 160 KB LDS
__global__ __launch_bounds__(1024) void csr_scan_kernel(const int32_t* __restrict__ cnt, int64_t N,
                                                        int32_t* __restrict__ rowptr) {
  extern __shared__ int32_t sbuf[];             // [tile][1024 partials + 32]
  const int t = threadIdx.x;
  const int tile_cap = (int)(N < SCAN_LDS ? (N + 3) / 4 * 4 : SCAN_LDS);
  int32_t* part = sbuf + tile_cap;
  int32_t carry = 0;
  for (int64_t base = 0; base < N || base == 0; base += SCAN_LDS) {
    const int64_t rem = N - base;
    const int n = (int)(rem < SCAN_LDS ? (rem > 0 ? rem : 0) : SCAN_LDS);     // entries of this tile
    // all global loads in flight at once (9 x int4 per thread covers SCAN_LDS), then LDS
    constexpr int VPT = SCAN_LDS / 4096;
    int4 v[VPT];
    const int n4 = n >> 2;
    const int4* src4 = reinterpret_cast<const int4*>(cnt + base);     // base is a multiple of SCAN_LDS: 16-B aligned
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int q = t + 1024 * k;
      v[k] = q < n4 ? src4[q] : make_int4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int q = t + 1024 * k;
      if (q < n4) reinterpret_cast<int4*>(sbuf)[q] = v[k];
    }
    if (t < (n & 3)) sbuf[(n4 << 2) + t] = cnt[base + (n4 << 2) + t];
    __syncthreads();
    const int chunk = (n + 1023) / 1024;
    const int lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    int32_t sum = 0;
    for (int i = lo; i < hi; ++i) sum += sbuf[i];
    // inclusive scan of the 1024 per-thread sums: shuffles inside each wave, the 16 wave totals through
    // LDS (2 barriers instead of the 20 of a block-wide Hillis-Steele)
    int32_t inc = sum;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const int32_t u = __shfl_up(inc, off);
      if ((t & (WAVE - 1)) >= off) inc += u;
    }
    if ((t & (WAVE - 1)) == WAVE - 1) part[t >> 6] = inc;
    __syncthreads();
    if (t < 16) {
      int32_t w = part[t];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const int32_t u = __shfl_up(w, off, 16);
        if (t >= off) w += u;
      }
      part[16 + t] = w;            // inclusive totals of waves 0..t
    }
    __syncthreads();
    const int32_t wave_base = (t >> 6) > 0 ? part[16 + (t >> 6) - 1] : 0;
    const int32_t total = part[31];
    int32_t run = carry + wave_base + inc - sum;   // exclusive prefix of this thread's chunk
    for (int i = lo; i < hi; ++i) { const int32_t c = sbuf[i]; sbuf[i] = run; run += c; }
    __syncthreads();
    if ((((uintptr_t)(rowptr + base)) & 15) == 0) {                   // 16-B stores (the usual case: allocator-aligned rowptr)
      for (int q = t; q < n4; q += 1024) {
        const int4 x = reinterpret_cast<const int4*>(sbuf)[q];
        reinterpret_cast<int4*>(rowptr + base)[q] = x;
      }
      if (t < (n & 3)) rowptr[base + (n4 << 2) + t] = sbuf[(n4 << 2) + t];
    } else {
      for (int i = t; i < n; i += 1024) rowptr[base + i] = sbuf[i];
    }
    carry += total;
    __syncthreads();
    if (N == 0) break;
  }
  if (t == 0) rowptr[N] = carry;
}

// The scan for tables of at most SCAN_MULTI_MAX entries (every batch of the benchmark configs but the long-graph one):
// workgroup b owns entries [1024 b, 1024 b + 1024) and gets the sum of everything before them by reading those counts
// itself (<= 64 int4 per thread, all L2 hits) -- no carry chain between workgroups, no second launch, ~1/1024 of the
// quadratic cost.  256-thread workgroups on purpose: the drug encoder's build runs on a side stream beside the protein
// encoder's CU-filling kernels, and a 1024-thread / 4-waves-per-SIMD block found no CU to start on until those had
// drained (59 us gap in the first round-4 step trace); one wave per SIMD fits beside them.
// `cnt` holds `counters` (a multiple of 64, > N) zero-initialised words: entries N.. are zero, so rowptr[N] = total
// falls out of the same exclusive scan.
constexpr int SCAN_MULTI_MAX = 65536, SCAN_MULTI_T = 256, SCAN_MULTI_CHUNK = 4 * SCAN_MULTI_T;
__global__ __launch_bounds__(SCAN_MULTI_T) void csr_scan_multi_kernel(const int32_t* __restrict__ cnt, int32_t N,
                                                                      int32_t counters, int32_t* __restrict__ rowptr) {
  __shared__ int32_t part[2 * (SCAN_MULTI_T / WAVE)];
  const int t = threadIdx.x, wv = t >> 6;
  const int4* c4 = reinterpret_cast<const int4*>(cnt);             // `work` is 16-B aligned (csr_build checks)
  int32_t pre = 0;
  for (int q = t; q < (int)blockIdx.x * SCAN_MULTI_T; q += SCAN_MULTI_T) {
    const int4 v = c4[q];
    pre += (v.x + v.y) + (v.z + v.w);
  }
  const int i0 = (int)blockIdx.x * SCAN_MULTI_CHUNK + 4 * t;
  const int4 v = i0 < counters ? c4[i0 >> 2] : make_int4(0, 0, 0, 0);
  const int32_t sum = (v.x + v.y) + (v.z + v.w);
  int32_t inc = sum;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int32_t u = __shfl_up(inc, off);
    if ((t & (WAVE - 1)) >= off) inc += u;
    pre += __shfl_xor(pre, off);
  }
  if ((t & (WAVE - 1)) == WAVE - 1) { part[wv] = inc; part[SCAN_MULTI_T / WAVE + wv] = pre; }
  __syncthreads();
  int32_t run = inc - sum;                         // exclusive prefix of this thread's four entries
#pragma unroll
  for (int w = 0; w < SCAN_MULTI_T / WAVE; ++w) {
    run += part[SCAN_MULTI_T / WAVE + w];
    if (w < wv) run += part[w];
  }
  const int32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k <= N) rowptr[i0 + k] = run;
    run += x[k];
  }
}

__global__ void csr_fill_kernel(const int64_t* __restrict__ ei, int64_t N, int64_t E, const int32_t* __restrict__ rowptr,
                                int32_t* __restrict__ cnt, int32_t* __restrict__ tmp, int32_t* __restrict__ edst) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  int64_t s = ei[e], d = ei[E + e];
  if (s < 0 || s >= N || d < 0 || d >= N) return;
  int32_t pos = rowptr[d] + atomicSub(&cnt[d], 1) - 1;
  // pos < E always holds when the counters were zero on entry (the contract).  The guard makes a violated contract a wrong
  // table instead of a wild write: round 2's recorded GPU fault ("write access to a read-only page" on replay of a captured
  // step) was exactly this store -- the counters were then zero-filled by a captured hipMemsetAsync, which zeroes only
  // part of its range from the second graph replay on (tools/memset_capture_probe.py), so counts accumulated over replays
  // and `pos` ran past the E-element tables.
  if (pos < 0 || pos >= E) return;
  tmp[pos] = (int32_t)e;
  edst[pos] = (int32_t)d;
}

// Position p of target n's segment holds SOME edge of n (arrival order of the fill).  Its final place is its rank
// among the segment's edge ids; deg independent reads per position instead of a serial per-node insertion sort.
// Threads t < counters also restore the zeroed-counters contract of `work`.
// Positions rowptr[N] .. E of the sorted tables exist only when edges were dropped (endpoint out of range): they get
// eperm = -1, esrc = edst = 0, so a kernel that walks all E positions (the edge-embedding backward) can skip them.
__global__ void csr_rank_kernel(const int64_t* __restrict__ ei, int64_t N, int64_t E, int64_t counters,
                                const int32_t* __restrict__ rowptr, const int32_t* __restrict__ tmp,
                                int32_t* __restrict__ edst, int32_t* __restrict__ eperm,
                                int32_t* __restrict__ esrc, int32_t* __restrict__ cnt) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < counters) cnt[t] = 0;
  if (t >= rowptr[N] || t >= E) {
    if (t < E) { eperm[t] = -1; esrc[t] = 0; edst[t] = 0; }
    return;
  }
  // (the range checks below never fire on tables built from zeroed counters; they keep every access inside the
  // E-element tables whatever the counters held -- see csr_fill_kernel)
  const int32_t n = edst[t];
  if (n < 0 || n >= N) return;
  int32_t lo = rowptr[n], hi = rowptr[n + 1];
  const int32_t key = tmp[t];
  if (lo < 0 || hi > E || lo > hi || key < 0 || key >= E) return;
  int32_t rank = 0;
  for (int32_t j = lo; j < hi; ++j) rank += tmp[j] < key ? 1 : 0;
  eperm[lo + rank] = key;
  esrc[lo + rank] = (int32_t)ei[key];
}

// ===================================================================== source-order index (deterministic mode)
// The sorted positions of every SOURCE of a dst-sorted CSR, in increasing position: the read-back order of the per-source
// sums that replace the d h[src] / d x[src] float atomics (quad::src_sum).  Count / scan / fill as in the CSR build
// (integer atomics: only the fill order depends on arrival), then each position's rank among its source's positions
// fixes the order.  The fill counts the counters back down to zero.
__global__ void src_count_kernel(const int32_t* __restrict__ esrc, const int32_t* __restrict__ rowptr, int64_t N,
                                 int32_t* __restrict__ cnt) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= rowptr[N]) return;
  const int32_t s = esrc[p];
  if (s >= 0 && s < N) atomicAdd(&cnt[s], 1);
}
__global__ void src_fill_kernel(const int32_t* __restrict__ esrc, const int32_t* __restrict__ rowptr, int64_t N,
                                const int32_t* __restrict__ sptr, int32_t* __restrict__ cnt, int32_t* __restrict__ tmp) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t ev = rowptr[N];
  if (p >= ev) return;
  const int32_t s = esrc[p];
  if (s < 0 || s >= N) return;
  const int32_t pos = sptr[s] + atomicSub(&cnt[s], 1) - 1;
  if (pos >= 0 && pos < ev) tmp[pos] = (int32_t)p;
}
__global__ void src_rank_kernel(const int32_t* __restrict__ esrc, const int32_t* __restrict__ rowptr, int64_t N,
                                const int32_t* __restrict__ sptr, const int32_t* __restrict__ tmp, int32_t* __restrict__ spos) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t ev = rowptr[N];
  if (k >= ev) return;
  const int32_t p = tmp[k];
  if (p < 0 || p >= ev) return;
  const int32_t s = esrc[p];
  if (s < 0 || s >= N) return;
  const int32_t lo = sptr[s], hi = sptr[s + 1];
  if (lo < 0 || hi > ev || lo > hi) return;
  int32_t rank = 0;
  for (int32_t j = lo; j < hi; ++j) rank += tmp[j] < p ? 1 : 0;
  spos[lo + rank] = p;
}

// Batch CSR by CONCATENATION of per-graph CSRs (a dataset's few hundred unique
// graphs are sorted once; a batch is their blocks shifted by node / edge offsets).  One workgroup
// per batch slot; `sel[b]` is the slot's graph in the store, whose tables hold LOCAL indices.
struct CsrCollateArgs {
  const int32_t* st_rowptr; const int32_t* st_eperm; const int32_t* st_esrc; const int32_t* st_edst;
  const int64_t* st_node_off; const int64_t* st_edge_off;      // [G+1] prefix sums over the store's graphs
  const int64_t* sel; const int64_t* b_node_off; const int64_t* b_edge_off;   // [B], [B+1], [B+1]
  int64_t B; int32_t* rowptr; int32_t* eperm; int32_t* esrc; int32_t* edst;
  int table_mode;      // 1: eperm = position in the STORE's dst-sorted feature tables (features stay resident, read in place)
};
__global__ __launch_bounds__(256) void csr_collate_kernel(CsrCollateArgs a) {
  const int64_t b = blockIdx.x;
  const int64_t g = a.sel[b];
  const int64_t sn = a.st_node_off[g], se = a.st_edge_off[g];
  const int64_t n = a.st_node_off[g + 1] - sn, e = a.st_edge_off[g + 1] - se;
  const int64_t bn = a.b_node_off[b], be = a.b_edge_off[b];
  const int32_t* rp = a.st_rowptr + sn + g;                     // every graph stores n + 1 row pointers
  for (int64_t k = threadIdx.x; k < n; k += 256) a.rowptr[bn + k] = (int32_t)(be + rp[k]);
  if (b == a.B - 1 && threadIdx.x == 0) a.rowptr[bn + n] = (int32_t)(be + e);
  for (int64_t k = threadIdx.x; k < e; k += 256) {
    a.eperm[be + k] = a.table_mode ? (int32_t)(se + k) : (int32_t)(be + a.st_eperm[se + k]);
    a.esrc[be + k] = (int32_t)(bn + a.st_esrc[se + k]);
    a.edst[be + k] = (int32_t)(bn + a.st_edst[se + k]);
  }
}

// ------------------------------------------------------------------ what the two drivers share
constexpr int TPB = 256;                // threads per workgroup of the per-edge / per-position launches
inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }
// words of the counter table: N + 1 rounded up to 64 (the scan reads them as int4; csr_rank zeroes exactly these)
inline int64_t counters_of(int64_t N) { return (N + 1 + 63) / 64 * 64; }
// node / edge ids are int32 in every table; the scans read `work` as int4
inline bool bad_sizes(int64_t N, int64_t E, const int32_t* work) {
  return N >= (int64_t)1 << 31 || E >= (int64_t)1 << 31 || ((uintptr_t)work & 15);
}
// exclusive scan of cnt[0 .. N] -> out (out[N] = total): independent workgroups for short tables, ONE block for long ones
int scan_counts(const int32_t* cnt, int64_t N, int64_t counters, int32_t* out, hipStream_t s) {
  if (N < SCAN_MULTI_MAX)
    return launch<csr_scan_multi_kernel>(dim3((unsigned)((N + 1 + SCAN_MULTI_CHUNK - 1) / SCAN_MULTI_CHUNK)),
                                         dim3(SCAN_MULTI_T), 0, s, cnt, (int32_t)N, (int32_t)counters, out);
  const int64_t tile = N < SCAN_LDS ? (N + 3) / 4 * 4 : SCAN_LDS;
  return launch<csr_scan_kernel>(dim3(1), dim3(1024), (size_t)(tile + 1024 + 32) * sizeof(int32_t), s, cnt, N, out);
}

}  // namespace

namespace quad {

void zero_words(void* p, size_t words, hipStream_t s) {
  if (words == 0 || !p) return;
  size_t blocks = (words + 1023) / 1024;                     // 4 words per thread at most
  if (blocks > 2048) blocks = 2048;
  launch<zero_words_kernel>(dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<uint32_t*>(p), words);
}

// cgvp_csr_from_coo; rng_state / rng_out (both or neither): the count launch also advances the dropout generator
// (cgvp_rng_next's work) -- with E == 0 or work_is_zero == 2 there is no count launch and a 1-thread launch does it.
int csr_build(const int64_t* edge_index, int64_t N, int64_t E, int32_t* rowptr, int32_t* eperm, int32_t* esrc,
              int32_t* edst, int32_t* work, int work_is_zero, int32_t* ids_scratch, unsigned long long* rng_state,
              unsigned long long* rng_out, hipStream_t s) {
  if (N < 0 || E < 0 || !rowptr || !work || (E > 0 && (!edge_index || !eperm || !esrc || !edst || !ids_scratch)))
    return CGVP_ERR_BAD_ARG;
  if (bad_sizes(N, E, work)) return CGVP_ERR_BAD_ARG;
  const int64_t counters = counters_of(N);
  if (work_is_zero == 0) zero_words(work, (size_t)counters, s);
  if (E > 0 && work_is_zero != 2)     // 2: cgvp_lba_pass_begin already counted into `work`
    launch<csr_count_kernel>(dim3(blocks_of(E)), dim3(TPB), 0, s, edge_index, N, E, work, rng_state, rng_out);
  else if (rng_state)
    rng_next(rng_state, rng_out, s);
  if (int rc = scan_counts(work, N, counters, rowptr, s)) return rc;
  if (E > 0) launch<csr_fill_kernel>(dim3(blocks_of(E)), dim3(TPB), 0, s, edge_index, N, E, rowptr, work, ids_scratch, edst);
  launch<csr_rank_kernel>(dim3(blocks_of(E > counters ? E : counters)), dim3(TPB), 0, s, edge_index, N, E, counters, rowptr,
                          ids_scratch, edst, eperm, esrc, work);
  return launch_status();
}

// work: [counters (N + 1 rounded up to 64) | tmp (E)]
int64_t src_index_work_ints(int64_t N, int64_t E) { return counters_of(N) + (E > 0 ? E : 1); }

int src_index(const int32_t* rowptr, const int32_t* esrc, int64_t N, int64_t E, int32_t* sptr, int32_t* spos,
              int32_t* work, hipStream_t s) {
  if (N < 0 || E < 0 || !rowptr || !sptr || !work || (E > 0 && (!esrc || !spos))) return CGVP_ERR_BAD_ARG;
  if (bad_sizes(N, E, work)) return CGVP_ERR_BAD_ARG;
  const int64_t counters = counters_of(N);
  int32_t* cnt = work;
  int32_t* tmp = work + counters;
  zero_words(cnt, (size_t)counters, s);
  if (E > 0) launch<src_count_kernel>(dim3(blocks_of(E)), dim3(TPB), 0, s, esrc, rowptr, N, cnt);
  if (int rc = scan_counts(cnt, N, counters, sptr, s)) return rc;
  if (E > 0) {
    launch<src_fill_kernel>(dim3(blocks_of(E)), dim3(TPB), 0, s, esrc, rowptr, N, sptr, cnt, tmp);
    launch<src_rank_kernel>(dim3(blocks_of(E)), dim3(TPB), 0, s, esrc, rowptr, N, sptr, tmp, spos);
  }
  return launch_status();
}

}  // namespace quad

// ===================================================================== C ABI
extern "C" {

int cgvp_csr_from_coo(const int64_t* edge_index, int64_t N, int64_t E, int32_t* rowptr,
                      int32_t* eperm, int32_t* esrc, int32_t* edst, int32_t* work, int32_t work_is_zero,
                      int32_t* ids_scratch, void* stream) {
  return quad::csr_build(edge_index, N, E, rowptr, eperm, esrc, edst, work, work_is_zero, ids_scratch, nullptr, nullptr,
                         (hipStream_t)stream);
}

int cgvp_csr_collate(const int32_t* st_rowptr, const int32_t* st_eperm, const int32_t* st_esrc,
                     const int32_t* st_edst, const int64_t* st_node_off, const int64_t* st_edge_off,
                     const int64_t* sel, const int64_t* b_node_off, const int64_t* b_edge_off, int64_t B,
                     int32_t table_mode, int32_t* rowptr, int32_t* eperm, int32_t* esrc, int32_t* edst, void* stream) {
  if (B < 0 || !rowptr) return CGVP_ERR_BAD_ARG;
  if (B == 0) return 0;
  if (!st_rowptr || !st_node_off || !st_edge_off || !sel || !b_node_off || !b_edge_off) return CGVP_ERR_BAD_ARG;
  CsrCollateArgs a{st_rowptr, st_eperm, st_esrc, st_edst, st_node_off, st_edge_off, sel, b_node_off, b_edge_off, B,
                   rowptr, eperm, esrc, edst, table_mode ? 1 : 0};
  launch<csr_collate_kernel>(dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status();
}

int64_t cgvp_src_index_work_ints(int64_t num_nodes, int64_t num_edges) {
  if (num_nodes < 0 || num_edges < 0) return CGVP_ERR_BAD_ARG;
  return quad::src_index_work_ints(num_nodes, num_edges);
}

int cgvp_src_index(const int32_t* rowptr, const int32_t* esrc, int64_t num_nodes, int64_t num_edges, int32_t* sptr,
                   int32_t* spos, int32_t* work, void* stream) {
  return quad::src_index(rowptr, esrc, num_nodes, num_edges, sptr, spos, work, (hipStream_t)stream);
}

}  // extern "C"
