// attn_pairs_kernels.hip -- the varlen cross attention over a list of pairs of UNIQUE graphs, forward only
// (include/caster_gvp_attnpairs.h; inference).
//
// Scoring one protein against 1,024 drugs through attn_kernels.hip needs the protein's rows 1,024 times: its Prob ties
// pair b to rows ptr[b] .. ptr[b+1] of q, k, v and out alike.  Here q / k / v hold every unique graph once and two index
// tables say which query graph and which key graph pair b uses; only `out` (and the lse) are per pair:
//
//     out[out_ptr[b] + r] = softmax_k( scale * q[q_ptr[q_graph[b]] + r] . k[key] ) v[key],
//                           key in rows k_ptr[k_graph[b]] .. k_ptr[k_graph[b] + 1]
//
// Work unit: one wave per (16-row OUTPUT tile of one pair, head), found with attn::locate over out_ptr.  From there on
// the kernel is attn_fwd_kernel<false, M> of attn_kernels.hip restated -- lane orientation, prefetched key tile,
// unconditional loads clamped to the pair's last key, peeled partial tail, 32-bit element offsets, online-softmax order,
// epilogue -- so that a pair's arithmetic is the same instruction sequence on the same values: tests/test_pair_scoring.py
// holds the two kernels together bitwise.  (Lifting the loop out of attn_kernels.hip instead would change the code of a
// measured kernel.)  No dropout, no backward, no weights.
//
// cgvp_expand_rows is the copy that goes with it: the per-pair rows of the unique graphs (the residual stream the
// attention output is added to) and the pair id of every row (the `batch` vector of the pooling).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/caster_gvp_attnpairs.h"
#include "attn_common.h"

namespace {

using namespace attn;
constexpr int WPB = 4, TPB = WAVE * WPB;

struct Prob {
  const float* q; const float* k; const float* v;         // [Nq][E], [Nk][E], [Nk][E]: rows of the unique graphs
  const int64_t* q_ptr; const int64_t* k_ptr;             // [Gq + 1], [Gk + 1]
  const int64_t* q_graph; const int64_t* k_graph;         // [B]
  const int64_t* out_ptr;                                  // [B + 1]
  float* out; float* lse;                                  // [No][E], [No][H] or NULL
  int32_t units;                                           // upper bound of the output tiles: ceil(No / 16) + B
};
struct Args { Prob p[2]; int nprob; int B; int H; int E; float scale; };

template <int M>
__global__ __launch_bounds__(TPB) void attn_fwd_pairs_kernel(Args a) {
  constexpr int HD = TILE * M;
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  int64_t u = (int64_t)blockIdx.x * WPB + wave_id();
  int pi = 0;
  if (u >= (int64_t)a.p[0].units * a.H) { u -= (int64_t)a.p[0].units * a.H; pi = 1; }
  if (pi >= a.nprob) return;
  const Prob P = pick(a, pi);
  if (u >= (int64_t)P.units * a.H) return;
  const int h = (int)(u % a.H), t = (int)(u / a.H);
  int b;
  int64_t o0_, o_end_;
  if (!locate(P.out_ptr, a.B, t, lane, b, o0_, o_end_)) return;
  // rows and element offsets in 32 bits (the host checks rows x E < 2^31 for q, k and out), see attn_fwd_kernel
  const int64_t qg = P.q_graph[b], kg = P.k_graph[b];
  const int o0 = (int)o0_, o_end = (int)o_end_;
  const int q0 = (int)P.q_ptr[qg] + (o0 - (int)P.out_ptr[b]);        // the tile's first row in the query graph
  const int k0 = (int)P.k_ptr[kg], k_end = (int)P.k_ptr[kg + 1];
  const int qr = q0 + n, orow = o0 + n;
  const bool qv = orow < o_end;                                      // (the pair's rows in out ARE the graph's length)
  const unsigned E = a.E, col = h * HD;
  f4 qs[M], acc[M];
#pragma unroll
  for (int c = 0; c < M; ++c) qs[c] = f4{0.f, 0.f, 0.f, 0.f};
  if (qv) {
#pragma unroll
    for (int c = 0; c < M; ++c) qs[c] = *reinterpret_cast<const f4*>(P.q + ((unsigned)qr * E + col + 4 * g + TILE * c)) * a.scale;
  }
#pragma unroll
  for (int c = 0; c < M; ++c) acc[c] = f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  // the key-tile loop of attn_fwd_kernel: the NEXT tile's K / V rows are loaded while the current one is computed;
  // loads are unconditional on offsets that advance by 16 rows per call and are clamped to the pair's last key
  const unsigned k_step = TILE * E;
  const unsigned ko_last = (unsigned)(k_end - 1) * E + col + 4 * g, vo_last = (unsigned)(k_end - 1) * E + col + n;
  unsigned ko = (unsigned)(k0 + n) * E + col + 4 * g;
  unsigned vo[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) vo[r] = (unsigned)(k0 + 4 * g + r) * E + col + n;
  auto load_tile = [&](f4 (&kk)[M], float (&va)[M][4]) {           // the next 16 keys, call by call
    const unsigned kc = ko < ko_last ? ko : ko_last;
#pragma unroll
    for (int c = 0; c < M; ++c) kk[c] = *reinterpret_cast<const f4*>(P.k + (kc + TILE * c));
    ko += k_step;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned vc = vo[r] < vo_last ? vo[r] : vo_last;
#pragma unroll
      for (int c = 0; c < M; ++c) va[c][r] = P.v[vc + TILE * c];
      vo[r] += k_step;
    }
  };
  f4 kk_n[M];
  float va_n[M][4];
#pragma unroll
  for (int c = 0; c < M; ++c) {
    kk_n[c] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) va_n[c][r] = 0.f;
  }
  if (k0 < k_end) load_tile(kk_n, va_n);
  auto tile = [&](int kb, auto tail) {
    f4 kk[M];
    float va[M][4];
#pragma unroll
    for (int c = 0; c < M; ++c) {
      kk[c] = kk_n[c];
#pragma unroll
      for (int r = 0; r < 4; ++r) va[c][r] = va_n[c][r];
    }
    load_tile(kk_n, va_n);                                  // past the end: copies of the last key, never used
    f4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < M; ++c) {
#pragma unroll
      for (int s = 0; s < 4; ++s) st = mfma(kk[c][s], qs[c][s], st);
    }
    if constexpr (decltype(tail)::value) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kb + 4 * g + r >= k_end) st[r] = -INFINITY;
    }
    const float m_new = fmaxf(m, quad_max(fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3]))));   // finite: a tile holds a valid key
    const float alpha = fexp(m - m_new);                    // m = -inf before the first tile: exp2(-inf) = 0
    float p[4], ps = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { p[r] = fexp(st[r] - m_new); ps += p[r]; }
    l = l * alpha + quad_sum(ps);
#pragma unroll
    for (int c = 0; c < M; ++c) acc[c] *= alpha;
    m = m_new;
#pragma unroll
    for (int c = 0; c < M; ++c) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[c] = mfma(va[c][r], p[r], acc[c]);
    }
  };
  int kb = k0;
  for (; kb + TILE <= k_end; kb += TILE) tile(kb, std::false_type{});
  if (kb < k_end) tile(kb, std::true_type{});
  if (qv) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int c = 0; c < M; ++c) *reinterpret_cast<f4*>(P.out + ((unsigned)orow * E + col + 4 * g + TILE * c)) = acc[c] * inv;
    if (g == 0 && P.lse) P.lse[(unsigned)orow * a.H + h] = (l > 0.f) ? m + logf(l) : -INFINITY;
  }
}

// One wave per 16-row tile of one pair's rows in out: lanes walk the tile's float4s (16 rows x width / 4), a row's
// lanes read consecutive addresses of one source row.
struct ExpandArgs {
  const float* src; const int64_t* src_ptr; const int64_t* graph; const int64_t* out_ptr;
  float* out; int64_t* batch_out;
  int B; int W4; int32_t units;                             // W4 = width / 4; units: ceil(No / 16) + B
};

__global__ __launch_bounds__(TPB) void expand_rows_kernel(ExpandArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * WPB + wave_id();
  if (t >= a.units) return;
  int b;
  int64_t o0, o_end;
  if (!locate(a.out_ptr, a.B, (int)t, lane, b, o0, o_end)) return;
  const int64_t s0 = a.src_ptr[a.graph[b]] + (o0 - a.out_ptr[b]);
  const int rows = (int)(o_end - o0 < TILE ? o_end - o0 : TILE);
  const float4* __restrict__ src = reinterpret_cast<const float4*>(a.src) + s0 * a.W4;
  float4* __restrict__ dst = reinterpret_cast<float4*>(a.out) + o0 * a.W4;
  const int total = rows * a.W4;                            // the tile's rows are contiguous on both sides
  for (int i = lane; i < total; i += WAVE) dst[i] = src[i];
  if (a.batch_out && lane < rows) a.batch_out[o0 + lane] = b;
}

int fwd_pairs(const cgvp_attn_pairs_problem* probs, int nprob, int64_t B, int H, int head_dim, float scale, hipStream_t st) {
  return with_m(head_dim, [&](auto m) -> int {
    constexpr int M = decltype(m)::value;
    if (!probs || nprob < 1 || nprob > 2 || B < 0 || B >= ((int64_t)1 << 30) || H < 1) return CGVP_ERR_BAD_ARG;
    const int64_t E = (int64_t)H * TILE * M;
    Args a;
    a.nprob = nprob; a.B = (int)B; a.H = H; a.E = (int)E; a.scale = scale;
    // the problem whose waves loop over the longer key graphs gets the low workgroup indices (they start first), as
    // cgvp_attn_fwd orders its two: 1 protein x 1,024 drugs 0.640 ms against 0.653 ms in the given order, 16 proteins x
    // 64 drugs 0.879 against 0.936 (profiles/pair_scoring/)
    const bool swap = nprob == 2 && (double)probs[1].num_k * (double)(probs[0].num_k_graphs > 0 ? probs[0].num_k_graphs : 1) >
                                        (double)probs[0].num_k * (double)(probs[1].num_k_graphs > 0 ? probs[1].num_k_graphs : 1);
    for (int i = 0; i < 2; ++i) {
      Prob& p = a.p[i];
      p = Prob{};
      if (i >= nprob) continue;
      const cgvp_attn_pairs_problem& s = probs[swap ? 1 - i : i];
      if (s.num_q_graphs < 0 || s.num_k_graphs < 0 || !s.q_graph || !s.k_graph) return CGVP_ERR_BAD_ARG;
      if (!side_ok(s.num_q, s.q_ptr, E) || !side_ok(s.num_k, s.k_ptr, E) || !side_ok(s.num_out, s.out_ptr, E)) return CGVP_ERR_BAD_ARG;
      if ((s.num_q > 0 && !s.q) || (s.num_k > 0 && (!s.k || !s.v)) || (s.num_out > 0 && !s.out)) return CGVP_ERR_BAD_ARG;
      if (!aligned(16, s.q, s.k, s.v, s.out) || !aligned(8, s.q_ptr, s.k_ptr, s.q_graph, s.k_graph, s.out_ptr) || !aligned(4, s.lse))
        return CGVP_ERR_BAD_ARG;
      p.q = s.q; p.k = s.k; p.v = s.v; p.q_ptr = s.q_ptr; p.k_ptr = s.k_ptr; p.q_graph = s.q_graph; p.k_graph = s.k_graph;
      p.out_ptr = s.out_ptr; p.out = s.out; p.lse = s.lse;
      p.units = (int32_t)((s.num_out + TILE - 1) / TILE + B);
    }
    if (B == 0) return 0;
    const int64_t units = ((int64_t)a.p[0].units + a.p[1].units) * H;
    if (int rc = launch<attn_fwd_pairs_kernel<M>>(dim3((unsigned)((units + WPB - 1) / WPB)), dim3(TPB), 0, st, a)) return rc;
    return launch_status();
  });
}

}  // namespace

extern "C" int cgvp_attn_pairs_version(void) { return CGVP_ATTN_PAIRS_VERSION; }

extern "C" int cgvp_attn_fwd_pairs(const cgvp_attn_pairs_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads,
                                   int32_t head_dim, float scale, void* stream) {
  return fwd_pairs(probs, num_problems, num_pairs, heads, head_dim, scale, (hipStream_t)stream);
}

extern "C" int cgvp_expand_rows(const float* src, const int64_t* src_ptr, const int64_t* graph, const int64_t* out_ptr,
                                int64_t num_pairs, int64_t num_out, int32_t width, float* out, int64_t* batch_out, void* stream) {
  if (num_pairs < 0 || num_pairs >= ((int64_t)1 << 30) || num_out < 0 || num_out >= ((int64_t)1 << 33) || width < 4 || width % 4)
    return CGVP_ERR_BAD_ARG;
  if (!src_ptr || !graph || !out_ptr || (num_out > 0 && (!src || !out))) return CGVP_ERR_BAD_ARG;
  if (!aligned(16, src, out) || !aligned(8, src_ptr, graph, out_ptr, batch_out)) return CGVP_ERR_BAD_ARG;
  if (num_pairs == 0) return 0;
  ExpandArgs a{src, src_ptr, graph, out_ptr, out, batch_out, (int)num_pairs, width / 4,
               (int32_t)((num_out + TILE - 1) / TILE + num_pairs)};
  if (int rc = launch<expand_rows_kernel>(dim3((unsigned)((a.units + WPB - 1) / WPB)), dim3(TPB), 0, (hipStream_t)stream, a)) return rc;
  return launch_status();
}
