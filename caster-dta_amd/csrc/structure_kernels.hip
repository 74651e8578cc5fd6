// structure_kernels.hip -- backbone coordinates -> protein graph on the device (opt-in).
//
// The reference builds every protein graph once per protein on the CPU: 17 + 9 node features from the N, CA, C
// backbone (utils/create_protein_features.py:27-92), a dense L x L distance matrix thresholded by radius or by the k
// nearest neighbours (:290-331) and an O(L^2) Python list of index pairs filtered by NaN (utils/create_graphs.py:29,
// 44-45).  The kernels here produce the same tensors for a whole batch from 48 B of coordinates per residue:
//
//   node_feat_kernel   one thread per residue: dihedral cos/sin, property-table row, chain steps, side-chain
//                      direction; fp64 arithmetic on the fp32 coordinates (N residues only: the cost does not
//                      matter, and sin(arccos(c)) of a near-planar dihedral stays well conditioned)
//   radius_count_kernel / knn_select_kernel / graph_fill_kernel
//                      one wave per SOURCE residue i, lanes striding over the targets j of the same graph; the
//                      key of a pair is (|CA_i - CA_j|^2 in fp64, j).  count: popcount of the kept lanes.  select:
//                      k rounds of a wave-wide lexicographic min, each over the keys above the previous round's,
//                      leave the k-th smallest key tau_i.  fill: per 64-wide stripe a ballot of "key <= tau_i"
//                      (radius: d2 <= r^2) and the popcount of the lower lanes place the kept j in increasing
//                      order behind a running base: the reference's row-major COO bit for bit, without a sort.
//
// The exclusive scan between count and fill is the caller's.  Every offset read from `ptr` is clamped and every
// store position is checked against the tensor it goes to: malformed input gives a wrong graph, never a fault.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/caster_gvp_structure.h"
#include "gvp_host.h"

namespace {

constexpr int WAVE = 64, WAVES_PER_BLOCK = 4;

struct D3 { double x, y, z; };
__device__ inline D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline D3 unit(D3 a) {                                   // normalize_vecs :360-365: zero stays zero
  const double n = sqrt(dot(a, a));
  return n != 0.0 ? D3{a.x / n, a.y / n, a.z / n} : D3{0.0, 0.0, 0.0};
}
__device__ inline D3 load3(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }

__device__ inline int64_t clamp_row(int64_t v, int64_t n) { return v < 0 ? 0 : (v > n ? n : v); }

// Graph b and its rows [lo, hi) for row n: the largest b in [0, B-1] with ptr[b] <= n (a non-monotone ptr still ends
// inside [0, B-1]; only ptr[0..B] is read).  A row its graph's clamped range does not hold is a graph of its own.
__device__ inline void graph_range(const int64_t* ptr, int64_t B, int64_t N, int64_t n, int64_t& b, int64_t& lo, int64_t& hi) {
  int64_t l = 0, r = B - 1;
  while (l < r) {
    const int64_t m = (l + r + 1) >> 1;
    if (ptr[m] <= n) l = m; else r = m - 1;
  }
  b = l;
  lo = clamp_row(ptr[l], N);
  hi = clamp_row(ptr[l + 1], N);
  if (!(lo <= n && n < hi)) { lo = n; hi = n + 1; }
}

// angle of create_protein_features.py:37-53 for four consecutive chain atoms, as (cos, sin)
__device__ inline void dihedral(D3 a0, D3 a1, D3 a2, D3 a3, double& c, double& s) {
  const D3 u2 = unit(sub(a1, a0)), u1 = unit(sub(a2, a1)), u0 = unit(sub(a3, a2));
  const D3 n1 = unit(cross(u1, u0)), n2 = unit(cross(u2, u1));
  double cs = dot(n1, n2);
  cs = cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);
  const double sd = dot(n1, u2);
  const double sign = (double)((sd > 0.0) - (sd < 0.0));
  const double ang = acos(cs) * sign;
  c = cos(ang);
  s = sin(ang);
}

struct NodeArgs {
  const float* coords; const int64_t* types; const int64_t* ptr; const float* props;
  int64_t N, B; int T, P; float* x_s; float* x_v; int64_t* batch; int64_t* seq;
};

__global__ __launch_bounds__(256) void node_feat_kernel(NodeArgs a) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  int64_t b, lo, hi;
  graph_range(a.ptr, a.B, a.N, n, b, lo, hi);
  if (a.batch) a.batch[n] = b;
  if (a.seq) a.seq[n] = n - lo;
  const float* me = a.coords + 12 * n;
  const D3 aN = load3(me), aCA = load3(me + 3), aC = load3(me + 6);
  const bool first = n == lo, last = n + 1 == hi;
  double c[3] = {1.0, 1.0, 1.0}, s[3] = {0.0, 0.0, 0.0};            // padded angles are 0 (:58)
  D3 fwd{0.0, 0.0, 0.0}, bwd{0.0, 0.0, 0.0};
  if (!first) {
    const D3 pCA = load3(me - 12 + 3), pC = load3(me - 12 + 6);
    dihedral(pC, aN, aCA, aC, c[0], s[0]);                          // phi
    const D3 step = unit(sub(aCA, pCA));
    bwd = {-step.x, -step.y, -step.z};
  }
  if (!last) {
    const D3 nN = load3(me + 12), nCA = load3(me + 12 + 3);
    dihedral(aN, aCA, aC, nN, c[1], s[1]);                          // psi
    dihedral(aCA, aC, nN, nCA, c[2], s[2]);                         // omega
    fwd = unit(sub(nCA, aCA));
  }
  const D3 dn = unit(sub(aN, aCA)), dc = unit(sub(aC, aCA));
  const D3 bis = unit(add(dn, dc)), perp = unit(cross(dc, dn));
  const double k1 = sqrt(1.0 / 3.0), k2 = sqrt(2.0 / 3.0);
  const D3 side{-bis.x * k1 - perp.x * k2, -bis.y * k1 - perp.y * k2, -bis.z * k1 - perp.z * k2};

  float* xs = a.x_s + n * (int64_t)(6 + a.P);
#pragma unroll
  for (int t = 0; t < 3; ++t) { xs[t] = (float)c[t]; xs[3 + t] = (float)s[t]; }
  if (a.P > 0) {
    int64_t ty = a.types[n];
    ty = ty < 0 ? 0 : (ty >= a.T ? a.T - 1 : ty);                   // an unknown type reads the nearest row
    const float* row = a.props + ty * (int64_t)a.P;
    for (int p = 0; p < a.P; ++p) xs[6 + p] = row[p];
  }
  float* xv = a.x_v + 9 * n;
  xv[0] = (float)fwd.x; xv[1] = (float)fwd.y; xv[2] = (float)fwd.z;
  xv[3] = (float)bwd.x; xv[4] = (float)bwd.y; xv[5] = (float)bwd.z;
  xv[6] = (float)side.x; xv[7] = (float)side.y; xv[8] = (float)side.z;
}

struct EdgeArgs {
  const float* ca; const int64_t* ptr; int64_t N, B;
  double r2; int k; int keep_self;
  const double* tau_d2_in; const int64_t* tau_j_in;                 // fill (NULL: radius rule)
  double* tau_d2; int64_t* tau_j; int64_t* deg;                     // count / select outputs
  const int64_t* rowstart; int64_t E; int64_t* ei;                  // fill
};

__device__ inline double dist2(D3 p, const float* ca, int64_t j) {
  const double dx = p.x - (double)ca[3 * j], dy = p.y - (double)ca[3 * j + 1], dz = p.z - (double)ca[3 * j + 2];
  return dx * dx + dy * dy + dz * dz;
}

// the wave's source residue; false for the waves past the last one (uniform per wave)
__device__ inline bool wave_source(const EdgeArgs& a, int64_t& i, int& lane, int64_t& lo, int64_t& hi, D3& p) {
  i = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x / WAVE);
  lane = threadIdx.x % WAVE;
  if (i >= a.N) return false;
  int64_t b;
  graph_range(a.ptr, a.B, a.N, i, b, lo, hi);
  p = load3(a.ca + 3 * i);
  return true;
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void radius_count_kernel(EdgeArgs a) {
  int64_t i, lo, hi; int lane; D3 p;
  if (!wave_source(a, i, lane, lo, hi, p)) return;
  int64_t count = 0;
  for (int64_t s = lo; s < hi; s += WAVE) {
    const int64_t j = s + lane;
    const bool keep = j < hi && (a.keep_self || j != i) && dist2(p, a.ca, j) <= a.r2;
    count += __popcll(__ballot(keep));
  }
  if (lane == 0) a.deg[i] = count;
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void knn_select_kernel(EdgeArgs a) {
  int64_t i, lo, hi; int lane; D3 p;
  if (!wave_source(a, i, lane, lo, hi, p)) return;
  double pd = -1.0; int64_t pj = -1;                                // no key is <= (-1, -1): d2 >= 0
  int found = 0;
  for (int round = 0; round < a.k; ++round) {
    double bd = INFINITY; int64_t bj = INT64_MAX;                   // smallest key above (pd, pj) among this lane's j
    for (int64_t j = lo + lane; j < hi; j += WAVE) {
      if (!a.keep_self && j == i) continue;
      const double d2 = dist2(p, a.ca, j);
      const bool after = d2 > pd || (d2 == pd && j > pj);
      const bool better = d2 < bd || (d2 == bd && j < bj);
      if (after && better) { bd = d2; bj = j; }
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      const double od = __shfl_xor(bd, off, WAVE);
      const int64_t oj = (int64_t)__shfl_xor((long long)bj, off, WAVE);
      if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
    }
    if (bj == INT64_MAX) break;                                     // fewer than k candidates (uniform)
    pd = bd; pj = bj; ++found;
  }
  if (lane == 0) { a.tau_d2[i] = pd; a.tau_j[i] = pj; a.deg[i] = found; }
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void graph_fill_kernel(EdgeArgs a) {
  int64_t i, lo, hi; int lane; D3 p;
  if (!wave_source(a, i, lane, lo, hi, p)) return;
  const bool knn = a.tau_d2_in != nullptr;
  const double td = knn ? a.tau_d2_in[i] : a.r2;
  const int64_t tj = knn ? a.tau_j_in[i] : INT64_MAX;
  int64_t base = a.rowstart[i];
  for (int64_t s = lo; s < hi; s += WAVE) {
    const int64_t j = s + lane;
    bool keep = j < hi && (a.keep_self || j != i);
    if (keep) {
      const double d2 = dist2(p, a.ca, j);
      keep = d2 < td || (d2 == td && j <= tj);
    }
    const unsigned long long mask = __ballot(keep);
    const int64_t pos = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && pos >= 0 && pos < a.E) { a.ei[pos] = i; a.ei[a.E + pos] = j; }
    base += __popcll(mask);
  }
}

inline bool grid_for(int64_t items, int per_block, unsigned& blocks) {
  const int64_t n = (items + per_block - 1) / per_block;
  if (n > 0x7fffffffll) return false;
  blocks = (unsigned)n;
  return true;
}

}  // namespace

extern "C" int cgvp_structure_version(void) { return CGVP_STRUCTURE_VERSION; }

extern "C" int cgvp_node_featurise(const float* coords, const int64_t* types, const int64_t* ptr, const float* props,
                                   int64_t num_nodes, int64_t num_graphs, int32_t num_types, int32_t num_props,
                                   float* x_s, float* x_v, int64_t* batch, int64_t* seq, void* stream) {
  if (num_nodes < 0 || num_graphs < 0 || num_types < 0 || num_props < 0) return CGVP_ERR_BAD_ARG;
  if (num_props > 0 && (!props || num_types < 1 || !types)) return CGVP_ERR_BAD_ARG;
  if (num_nodes == 0) return 0;
  unsigned blocks;
  if (!coords || !ptr || !x_s || !x_v || num_graphs < 1 || !grid_for(num_nodes, 256, blocks)) return CGVP_ERR_BAD_ARG;
  NodeArgs a{coords, types, ptr, props, num_nodes, num_graphs, num_types, num_props, x_s, x_v, batch, seq};
  launch<node_feat_kernel>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status();
}

extern "C" int cgvp_radius_graph_count(const float* ca_xyz, const int64_t* ptr, int64_t num_nodes, int64_t num_graphs,
                                       double radius, int32_t keep_self_loops, int64_t* deg, void* stream) {
  if (num_nodes < 0 || num_graphs < 0 || !(radius >= 0.0) || !isfinite(radius)) return CGVP_ERR_BAD_ARG;
  if (num_nodes == 0) return 0;
  unsigned blocks;
  if (!ca_xyz || !ptr || !deg || num_graphs < 1 || !grid_for(num_nodes, WAVES_PER_BLOCK, blocks)) return CGVP_ERR_BAD_ARG;
  EdgeArgs a{};
  a.ca = ca_xyz; a.ptr = ptr; a.N = num_nodes; a.B = num_graphs; a.r2 = radius * radius; a.keep_self = keep_self_loops != 0;
  a.deg = deg;
  launch<radius_count_kernel>(dim3(blocks), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream, a);
  return launch_status();
}

extern "C" int cgvp_knn_graph_select(const float* ca_xyz, const int64_t* ptr, int64_t num_nodes, int64_t num_graphs,
                                     int32_t k, int32_t keep_self_loops, double* tau_d2, int64_t* tau_j, int64_t* deg,
                                     void* stream) {
  if (num_nodes < 0 || num_graphs < 0 || k < 1 || k > CGVP_KNN_MAX) return CGVP_ERR_BAD_ARG;
  if (num_nodes == 0) return 0;
  unsigned blocks;
  if (!ca_xyz || !ptr || !tau_d2 || !tau_j || !deg || num_graphs < 1 || !grid_for(num_nodes, WAVES_PER_BLOCK, blocks))
    return CGVP_ERR_BAD_ARG;
  EdgeArgs a{};
  a.ca = ca_xyz; a.ptr = ptr; a.N = num_nodes; a.B = num_graphs; a.k = k; a.keep_self = keep_self_loops != 0;
  a.tau_d2 = tau_d2; a.tau_j = tau_j; a.deg = deg;
  launch<knn_select_kernel>(dim3(blocks), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream, a);
  return launch_status();
}

extern "C" int cgvp_graph_fill(const float* ca_xyz, const int64_t* ptr, int64_t num_nodes, int64_t num_graphs,
                               double radius, const double* tau_d2, const int64_t* tau_j, int32_t keep_self_loops,
                               const int64_t* rowstart, int64_t num_edges, int64_t* edge_index, void* stream) {
  if (num_nodes < 0 || num_graphs < 0 || num_edges < 0 || (tau_d2 == nullptr) != (tau_j == nullptr)) return CGVP_ERR_BAD_ARG;
  if (!tau_d2 && (!(radius >= 0.0) || !isfinite(radius))) return CGVP_ERR_BAD_ARG;
  if (num_nodes == 0 || num_edges == 0) return 0;
  unsigned blocks;
  if (!ca_xyz || !ptr || !rowstart || !edge_index || num_graphs < 1 || !grid_for(num_nodes, WAVES_PER_BLOCK, blocks))
    return CGVP_ERR_BAD_ARG;
  EdgeArgs a{};
  a.ca = ca_xyz; a.ptr = ptr; a.N = num_nodes; a.B = num_graphs; a.r2 = radius * radius; a.keep_self = keep_self_loops != 0;
  a.tau_d2_in = tau_d2; a.tau_j_in = tau_j; a.rowstart = rowstart; a.E = num_edges; a.ei = edge_index;
  launch<graph_fill_kernel>(dim3(blocks), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream, a);
  return launch_status();
}
