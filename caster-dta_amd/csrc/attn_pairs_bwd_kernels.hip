// attn_pairs_bwd_kernels.hip -- the backward of the varlen cross attention over a list of pairs of UNIQUE graphs, and of
// the per-pair row copy that goes with it (include/caster_gvp_pairtrain.h; training on pair lists).
//
// q / k / v hold every unique graph once (attn_pairs_kernels.hip); the gradient of a unique row is the sum over all the
// pairs that reference its graph.  No float atomics: the sum is an ordered one, in two stages.
//
//   1. attn_bwd_pairs_dq_kernel / attn_bwd_pairs_dkv_kernel: attn_bwd_dq_kernel<false, M> / attn_bwd_dkv_kernel<false, M>
//      of attn_kernels.hip restated over the index tables, as attn_fwd_pairs_kernel restates attn_fwd_kernel -- lane
//      orientation, prefetched tile, unconditional loads clamped to the pair's last row, peeled partial tail, 32-bit
//      element offsets.  The operands q, k, v are read at the rows of the pair's UNIQUE graphs; out, lse, g_out and
//      delta at the pair's own rows (out_ptr).  They write PER-PAIR partial gradients with plain stores: d Q at the
//      pair's out_ptr rows, d K / d V at its kout_ptr rows (the out_ptr of the other direction).
//   2. reduce_rows_kernel (cgvp_reduce_rows, the transpose of cgvp_expand_rows): one wave per 16-row tile of a unique
//      graph adds the tile's partial rows of the pairs that reference the graph, in ascending pair order, through the
//      inverse table of the pair list.  One owner per output row; a graph without pairs gets zeros.  One launch serves
//      all six gradients of a call.
//
// The summation order is a function of the tables alone: the gradients are bitwise reproducible in every mode.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/caster_gvp_pairtrain.h"
#include "attn_common.h"

namespace {

using namespace attn;
constexpr int WPB = 4, TPB = WAVE * WPB;

struct Prob {
  const float* q; const float* k; const float* v;         // [Nq][E], [Nk][E], [Nk][E]: rows of the unique graphs
  const int64_t* q_ptr; const int64_t* k_ptr;             // [Gq + 1], [Gk + 1]
  const int64_t* q_graph; const int64_t* k_graph;         // [B]
  const int64_t* out_ptr; const int64_t* kout_ptr;        // [B + 1]: the pairs' query rows / key rows
  const float* out; const float* lse; const float* g_out; // [No][E], [No][H], [No][E]: per pair
  float* delta;                                            // [No][H] = sum_d dO . O
  float* pq; float* pk; float* pv;                         // per-pair partials: [No][E], [Nko][E], [Nko][E]
  int32_t units_q, units_k;                                // upper bounds: ceil(No / 16) + B and ceil(Nko / 16) + B
};
struct Args { Prob p[2]; int nprob; int B; int H; int E; float scale; };

// ------------------------------------------------------------------------------------------------ d Q (per pair)
// attn_bwd_dq_kernel over the tables.  A pair without keys never enters the key loop (zero d Q, delta = 0 from its zero
// output rows); the guard on the recomputed probability keeps a row whose lse is -inf at exactly zero all the same.
template <int M>
__global__ __launch_bounds__(TPB) void attn_bwd_pairs_dq_kernel(Args a) {
  constexpr int HD = TILE * M;
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  int64_t u = (int64_t)blockIdx.x * WPB + wave_id();
  int pi = 0;
  if (u >= (int64_t)a.p[0].units_q * a.H) { u -= (int64_t)a.p[0].units_q * a.H; pi = 1; }
  if (pi >= a.nprob) return;
  const Prob P = pick(a, pi);
  if (u >= (int64_t)P.units_q * a.H) return;
  const int h = (int)(u % a.H), t = (int)(u / a.H);
  int b;
  int64_t o0_, o_end_;
  if (!locate(P.out_ptr, a.B, t, lane, b, o0_, o_end_)) return;
  // rows and element offsets in 32 bits (the host checks rows x E < 2^31 for q, k, out and the partials)
  const int64_t qg = P.q_graph[b], kg = P.k_graph[b];
  const int o0 = (int)o0_, o_end = (int)o_end_;
  const int q0 = (int)P.q_ptr[qg] + (o0 - (int)P.out_ptr[b]);        // the tile's first row in the query graph
  const int k0 = (int)P.k_ptr[kg], k_end = (int)P.k_ptr[kg + 1];
  const int qr = q0 + n, orow = o0 + n;
  const bool qv = orow < o_end;
  const unsigned E = a.E, col = h * HD;
  f4 qs[M], go[M], acc[M];
#pragma unroll
  for (int c = 0; c < M; ++c) qs[c] = go[c] = f4{0.f, 0.f, 0.f, 0.f};
  float lse = 0.f, dl = 0.f;
  if (qv) {
    const unsigned qo = (unsigned)qr * E + col + 4 * g, oo = (unsigned)orow * E + col + 4 * g;
#pragma unroll
    for (int c = 0; c < M; ++c) {                                   // delta: all chunks of the head, then the query's 4 lanes
      qs[c] = *reinterpret_cast<const f4*>(P.q + (qo + TILE * c)) * a.scale;
      go[c] = *reinterpret_cast<const f4*>(P.g_out + (oo + TILE * c));
      const f4 o = *reinterpret_cast<const f4*>(P.out + (oo + TILE * c));
      const float dc = go[c][0] * o[0] + go[c][1] * o[1] + go[c][2] * o[2] + go[c][3] * o[3];
      dl = c == 0 ? dc : dl + dc;
    }
    lse = P.lse[(unsigned)orow * a.H + h];
  }
  dl = quad_sum(dl);
  if (qv && g == 0) P.delta[(unsigned)orow * a.H + h] = dl;
  const bool live = lse > -INFINITY;                                // (a lane without a query: lse = 0)
#pragma unroll
  for (int c = 0; c < M; ++c) acc[c] = f4{0.f, 0.f, 0.f, 0.f};
  const unsigned k_step = TILE * E;                                // offsets advanced per call and clamped, see attn_fwd_kernel
  const unsigned ko_last = (unsigned)(k_end - 1) * E + col + 4 * g, to_last = (unsigned)(k_end - 1) * E + col + n;
  unsigned ko = (unsigned)(k0 + n) * E + col + 4 * g;
  unsigned to[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) to[r] = (unsigned)(k0 + 4 * g + r) * E + col + n;
  auto load_tile = [&](f4 (&kk)[M], f4 (&vv)[M], float (&ka)[M][4]) {   // the next 16 keys; no zeroing, tail peeled
    const unsigned o = ko < ko_last ? ko : ko_last;
#pragma unroll
    for (int c = 0; c < M; ++c) {
      kk[c] = *reinterpret_cast<const f4*>(P.k + (o + TILE * c));
      vv[c] = *reinterpret_cast<const f4*>(P.v + (o + TILE * c));
    }
    ko += k_step;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned tc = to[r] < to_last ? to[r] : to_last;
#pragma unroll
      for (int c = 0; c < M; ++c) ka[c][r] = P.k[tc + TILE * c];
      to[r] += k_step;
    }
  };
  f4 kk_n[M], vv_n[M];
  float ka_n[M][4];
#pragma unroll
  for (int c = 0; c < M; ++c) {
    kk_n[c] = vv_n[c] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) ka_n[c][r] = 0.f;
  }
  if (k0 < k_end) load_tile(kk_n, vv_n, ka_n);
  auto tile = [&](int kb, auto tail) {
    f4 kk[M], vv[M];
    float ka[M][4];
#pragma unroll
    for (int c = 0; c < M; ++c) {
      kk[c] = kk_n[c]; vv[c] = vv_n[c];
#pragma unroll
      for (int r = 0; r < 4; ++r) ka[c][r] = ka_n[c][r];
    }
    load_tile(kk_n, vv_n, ka_n);
    f4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < M; ++c) {
#pragma unroll
      for (int s = 0; s < 4; ++s) { st = mfma(kk[c][s], qs[c][s], st); dp = mfma(vv[c][s], go[c][s], dp); }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pr = live ? fexp(st[r] - lse) : 0.f;
      if constexpr (decltype(tail)::value) pr = kb + 4 * g + r < k_end ? pr : 0.f;
      const float ds = pr * (dp[r] - dl);
#pragma unroll
      for (int c = 0; c < M; ++c) acc[c] = mfma(ka[c][r], ds, acc[c]);
    }
  };
  int kb = k0;
  for (; kb + TILE <= k_end; kb += TILE) tile(kb, std::false_type{});
  if (kb < k_end) tile(kb, std::true_type{});
  if (qv) {
#pragma unroll
    for (int c = 0; c < M; ++c) *reinterpret_cast<f4*>(P.pq + ((unsigned)orow * E + col + 4 * g + TILE * c)) = acc[c] * a.scale;
  }
}

// ------------------------------------------------------------------------------------------------ d K, d V (per pair)
// attn_bwd_dkv_kernel over the tables: a wave owns a 16-key tile of one pair's key rows (kout_ptr) and loops over the
// pair's queries.  k / v of the tile and q of the loop are rows of the unique graphs; g_out, lse and delta of the loop
// are the pair's own rows, a wave-uniform distance from the query graph's (added to the clamped offsets, modulo 2^32:
// the sums are the pair's true offsets, below 2^31).  A pair without keys owns no tile; a pair without queries writes
// zero rows.
template <int M>
__global__ __launch_bounds__(TPB) void attn_bwd_pairs_dkv_kernel(Args a) {
  constexpr int HD = TILE * M;
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  int64_t u = (int64_t)blockIdx.x * WPB + wave_id();
  int pi = 0;
  if (u >= (int64_t)a.p[0].units_k * a.H) { u -= (int64_t)a.p[0].units_k * a.H; pi = 1; }
  if (pi >= a.nprob) return;
  const Prob P = pick(a, pi);
  if (u >= (int64_t)P.units_k * a.H) return;
  const int h = (int)(u % a.H), t = (int)(u / a.H);
  int b;
  int64_t kt0_, ko_end_;
  if (!locate(P.kout_ptr, a.B, t, lane, b, kt0_, ko_end_)) return;
  const int64_t qg = P.q_graph[b], kg = P.k_graph[b];
  const int kt0 = (int)kt0_, ko_end = (int)ko_end_;             // the pair's key rows in the partials
  const int q0 = (int)P.q_ptr[qg], q_end = (int)P.q_ptr[qg + 1];
  const int kro = kt0 + n;                                      // this lane's key: its row in pk / pv ...
  const int kr = (int)P.k_ptr[kg] + (kt0 - (int)P.kout_ptr[b]) + n;   // ... and in k / v
  const bool kv = kro < ko_end;
  const unsigned E = a.E, col = h * HD, H = a.H;
  const int shift = (int)P.out_ptr[b] - q0;                     // the pair's query rows: out_ptr[b] + (row - q0)
  const unsigned dE = (unsigned)shift * E, dH = (unsigned)shift * H;
  f4 kk[M], vv[M], accv[M], acck[M];
#pragma unroll
  for (int c = 0; c < M; ++c) kk[c] = vv[c] = f4{0.f, 0.f, 0.f, 0.f};
  if (kv) {
#pragma unroll
    for (int c = 0; c < M; ++c) {
      kk[c] = *reinterpret_cast<const f4*>(P.k + ((unsigned)kr * E + col + 4 * g + TILE * c));
      vv[c] = *reinterpret_cast<const f4*>(P.v + ((unsigned)kr * E + col + 4 * g + TILE * c));
    }
  }
#pragma unroll
  for (int c = 0; c < M; ++c) accv[c] = acck[c] = f4{0.f, 0.f, 0.f, 0.f};
  struct QT { f4 qa[M], ga[M]; float lse[4], dl[4], qt[M][4], gt[M][4]; };
  const unsigned q_step = TILE * E, h_step = TILE * H;              // offsets advanced per call and clamped, see attn_fwd_kernel
  const unsigned qo_last = (unsigned)(q_end - 1) * E + col + 4 * g, to_last = (unsigned)(q_end - 1) * E + col + n,
                 ho_last = (unsigned)(q_end - 1) * H + h;
  unsigned qo = (unsigned)(q0 + n) * E + col + 4 * g;
  unsigned to[4], ho[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { to[r] = (unsigned)(q0 + 4 * g + r) * E + col + n; ho[r] = (unsigned)(q0 + 4 * g + r) * H + h; }
  auto load_tile = [&](QT& T) {                                     // the next 16 queries; no zeroing, tail peeled
    const unsigned qmo = qo < qo_last ? qo : qo_last;
#pragma unroll
    for (int c = 0; c < M; ++c) {
      T.qa[c] = *reinterpret_cast<const f4*>(P.q + (qmo + TILE * c)) * a.scale;
      T.ga[c] = *reinterpret_cast<const f4*>(P.g_out + (qmo + dE + TILE * c));
    }
    qo += q_step;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                           // per k-slot r <-> query qb + 4g + r
      const unsigned tc = to[r] < to_last ? to[r] : to_last, hc = (ho[r] < ho_last ? ho[r] : ho_last) + dH;
      to[r] += q_step; ho[r] += h_step;
      T.lse[r] = P.lse[hc];
      T.dl[r] = P.delta[hc];
#pragma unroll
      for (int c = 0; c < M; ++c) {
        T.qt[c][r] = P.q[tc + TILE * c] * a.scale;          // Qs^T operand of tile c: lane (m = d - 16c, g)
        T.gt[c][r] = P.g_out[tc + dE + TILE * c];           // dO^T operand
      }
    }
  };
  QT nxt = {};
  if (q0 < q_end) load_tile(nxt);
  auto tile = [&](int qb, auto tail) {
    const QT cur = nxt;
    load_tile(nxt);
    const float (&lse)[4] = cur.lse, (&dl)[4] = cur.dl, (&qt)[M][4] = cur.qt, (&gt)[M][4] = cur.gt;
    f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < M; ++c) {
#pragma unroll
      for (int x = 0; x < 4; ++x) { s = mfma(cur.qa[c][x], kk[c][x], s); dp = mfma(cur.ga[c][x], vv[c][x], dp); }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // (the pair has a key, so its lse is finite; the guard keeps an lse of -inf at exactly zero all the same)
      float pr = lse[r] > -INFINITY ? fexp(s[r] - lse[r]) : 0.f;
      if constexpr (decltype(tail)::value) pr = qb + 4 * g + r < q_end ? pr : 0.f;
#pragma unroll
      for (int c = 0; c < M; ++c) {
        accv[c] = mfma(gt[c][r], pr, accv[c]);
        acck[c] = mfma(qt[c][r], pr * (dp[r] - dl[r]), acck[c]);
      }
    }
  };
  int qb = q0;
  for (; qb + TILE <= q_end; qb += TILE) tile(qb, std::false_type{});
  if (qb < q_end) tile(qb, std::true_type{});
  if (kv) {
#pragma unroll
    for (int c = 0; c < M; ++c) {
      *reinterpret_cast<f4*>(P.pv + ((unsigned)kro * E + col + 4 * g + TILE * c)) = accv[c];
      *reinterpret_cast<f4*>(P.pk + ((unsigned)kro * E + col + 4 * g + TILE * c)) = acck[c];
    }
  }
}

// ------------------------------------------------------------------------------------------------ ordered row sum
// One wave per 16-row tile of one unique graph (found with attn::locate over src_ptr): the tile's float4s on the lanes,
// EPL at a time in registers, and over them the loop over the graph's pairs in ascending order -- the next pair's row
// offset is fetched while the current pair's rows are added.  Up to MAXJ jobs (gradient arrays) share one launch.
constexpr int MAXJ = 6, EPL = 8;
struct ReduceJob {
  const float* part; const int64_t* optr; const int64_t* inv_ptr; const int64_t* inv_pairs; const int64_t* src_ptr;
  float* dst; int G; int W4; int32_t units;                 // W4 = width / 4; units: ceil(rows of dst / 16) + G
};
struct ReduceArgs { ReduceJob j[MAXJ]; int n; };

__global__ __launch_bounds__(TPB) void reduce_rows_kernel(ReduceArgs a) {
  const int lane = threadIdx.x & 63;
  int64_t t = (int64_t)blockIdx.x * WPB + wave_id();        // wave-uniform: the job is picked with scalar selects
  ReduceJob J = a.j[0];
  bool found = t < J.units;
#pragma unroll
  for (int i = 1; i < MAXJ; ++i) {
    if (!found && i < a.n) { t -= J.units; J = a.j[i]; found = t < J.units; }
  }
  if (!found) return;
  int gi;
  int64_t r0, r_end;
  if (!locate(J.src_ptr, J.G, (int)t, lane, gi, r0, r_end)) return;
  const int rows = (int)(r_end - r0 < TILE ? r_end - r0 : TILE);
  const int64_t off = r0 - J.src_ptr[gi];                   // the tile's first row inside its graph
  const int64_t j0 = J.inv_ptr[gi], j1 = J.inv_ptr[gi + 1];
  const int total = rows * J.W4;                            // the tile's rows are contiguous on both sides
  const f4* __restrict__ part = reinterpret_cast<const f4*>(J.part);
  f4* __restrict__ dst = reinterpret_cast<f4*>(J.dst) + r0 * J.W4;
  for (int base = 0; base < total; base += WAVE * EPL) {
    f4 acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = f4{0.f, 0.f, 0.f, 0.f};
    int64_t nxt = j0 < j1 ? J.optr[J.inv_pairs[j0]] : 0;
    for (int64_t j = j0; j < j1; ++j) {
      const f4* __restrict__ src = part + (nxt + off) * J.W4;
      if (j + 1 < j1) nxt = J.optr[J.inv_pairs[j + 1]];
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const int i = base + lane + WAVE * e;
        if (i < total) acc[e] += src[i];
      }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int i = base + lane + WAVE * e;
      if (i < total) dst[i] = acc[e];
    }
  }
}

bool reduce_job(ReduceJob& j, const float* part, const int64_t* optr, const int64_t* inv_ptr, const int64_t* inv_pairs,
                const int64_t* src_ptr, int64_t G, int64_t num_dst, int width, float* dst) {
  j = ReduceJob{part, optr, inv_ptr, inv_pairs, src_ptr, dst, (int)G, width / 4, (int32_t)((num_dst + TILE - 1) / TILE + G)};
  return G > 0 && num_dst > 0;                              // else: nothing to write
}

int launch_reduce(const ReduceArgs& r, hipStream_t st) {
  int64_t units = 0;
  for (int i = 0; i < r.n; ++i) units += r.j[i].units;
  if (units == 0) return 0;
  return launch<reduce_rows_kernel>(dim3((unsigned)((units + WPB - 1) / WPB)), dim3(TPB), 0, st, r);
}

// ---- host: the attention backward
struct Plan { int64_t pq, pk, pv, delta; };                  // offsets of one problem's sub-buffers in the workspace, floats
int64_t plan_workspace(const cgvp_attn_pairs_bwd_problem* probs, int nprob, int64_t H, int64_t E, Plan* plan) {
  int64_t at = 0;
  for (int i = 0; i < nprob; ++i) {
    const cgvp_attn_pairs_bwd_problem& s = probs[i];
    if (s.num_out < 0 || s.num_kout < 0) return CGVP_ERR_BAD_ARG;
    Plan p;
    p.pq = at; at += s.num_out * E;
    p.pk = at; at += s.num_kout * E;
    p.pv = at; at += s.num_kout * E;
    p.delta = at; at += (s.num_out * H + 3) / 4 * 4;         // every sub-buffer starts on 16 bytes
    if (plan) plan[i] = p;
  }
  return at;
}

int bwd_pairs(const cgvp_attn_pairs_bwd_problem* probs, int nprob, int64_t B, int H, int head_dim, float scale, float* ws,
              int64_t ws_floats, hipStream_t st) {
  return with_m(head_dim, [&](auto m) -> int {
    constexpr int M = decltype(m)::value;
    if (!probs || nprob < 1 || nprob > 2 || B < 0 || B >= ((int64_t)1 << 30) || H < 1) return CGVP_ERR_BAD_ARG;
    const int64_t E = (int64_t)H * TILE * M;
    for (int i = 0; i < nprob; ++i) {
      const cgvp_attn_pairs_bwd_problem& s = probs[i];
      if (s.num_q_graphs < 0 || s.num_k_graphs < 0 || s.num_q_graphs >= ((int64_t)1 << 30) || s.num_k_graphs >= ((int64_t)1 << 30))
        return CGVP_ERR_BAD_ARG;
      if (!s.q_graph || !s.k_graph || !s.q_inv_ptr || !s.q_inv_pairs || !s.k_inv_ptr || !s.k_inv_pairs) return CGVP_ERR_BAD_ARG;
      if (!side_ok(s.num_q, s.q_ptr, E) || !side_ok(s.num_k, s.k_ptr, E) || !side_ok(s.num_out, s.out_ptr, E) ||
          !side_ok(s.num_kout, s.kout_ptr, E))
        return CGVP_ERR_BAD_ARG;
      if ((s.num_q > 0 && (!s.q || !s.g_q)) || (s.num_k > 0 && (!s.k || !s.v || !s.g_k || !s.g_v)) ||
          (s.num_out > 0 && (!s.out || !s.lse || !s.g_out)))
        return CGVP_ERR_BAD_ARG;
      if (!aligned(16, s.q, s.k, s.v, s.out, s.g_out, s.g_q, s.g_k, s.g_v) || !aligned(4, s.lse) ||
          !aligned(8, s.q_ptr, s.k_ptr, s.q_graph, s.k_graph, s.out_ptr, s.kout_ptr, s.q_inv_ptr, s.q_inv_pairs, s.k_inv_ptr, s.k_inv_pairs))
        return CGVP_ERR_BAD_ARG;
    }
    Plan plan[2];
    const int64_t need = plan_workspace(probs, nprob, H, E, plan);
    if (need < 0) return (int)need;
    if (!aligned(16, ws) || ws_floats < need || (need > 0 && !ws)) return CGVP_ERR_BAD_ARG;
    // which problem gets the low workgroup indices: the one whose waves loop longest (d Q: over the keys, as the
    // forward orders its two; d K / d V: over the queries, so the other one)
    const auto avg = [](int64_t rows, int64_t graphs) { return (double)rows / (double)(graphs > 0 ? graphs : 1); };
    const bool swap_q = nprob == 2 && avg(probs[1].num_k, probs[1].num_k_graphs) > avg(probs[0].num_k, probs[0].num_k_graphs);
    const bool swap_k = nprob == 2 && avg(probs[1].num_q, probs[1].num_q_graphs) > avg(probs[0].num_q, probs[0].num_q_graphs);
    Args aq, ak;
    ReduceArgs red;                                          // (jobs behind `n` are never read: no fill, the library calls no memset)
    red.n = 0;
    for (Args* a : {&aq, &ak}) {
      a->nprob = nprob; a->B = (int)B; a->H = H; a->E = (int)E; a->scale = scale;
      const bool swap = a == &aq ? swap_q : swap_k;
      for (int i = 0; i < 2; ++i) {
        Prob& p = a->p[i];
        if (i >= nprob) { p.units_q = p.units_k = 0; continue; }    // an absent problem: no units, nothing else is read
        const int si = swap ? 1 - i : i;
        const cgvp_attn_pairs_bwd_problem& s = probs[si];
        p.q = s.q; p.k = s.k; p.v = s.v; p.q_ptr = s.q_ptr; p.k_ptr = s.k_ptr; p.q_graph = s.q_graph; p.k_graph = s.k_graph;
        p.out_ptr = s.out_ptr; p.kout_ptr = s.kout_ptr; p.out = s.out; p.lse = s.lse; p.g_out = s.g_out;
        p.delta = ws + plan[si].delta; p.pq = ws + plan[si].pq; p.pk = ws + plan[si].pk; p.pv = ws + plan[si].pv;
        p.units_q = (int32_t)((s.num_out + TILE - 1) / TILE + B);
        p.units_k = (int32_t)((s.num_kout + TILE - 1) / TILE + B);
      }
    }
    for (int i = 0; i < nprob; ++i) {
      const cgvp_attn_pairs_bwd_problem& s = probs[i];
      const float* pq = ws + plan[i].pq; const float* pk = ws + plan[i].pk; const float* pv = ws + plan[i].pv;
      red.n += reduce_job(red.j[red.n], pq, s.out_ptr, s.q_inv_ptr, s.q_inv_pairs, s.q_ptr, s.num_q_graphs, s.num_q, (int)E, s.g_q);
      red.n += reduce_job(red.j[red.n], pk, s.kout_ptr, s.k_inv_ptr, s.k_inv_pairs, s.k_ptr, s.num_k_graphs, s.num_k, (int)E, s.g_k);
      red.n += reduce_job(red.j[red.n], pv, s.kout_ptr, s.k_inv_ptr, s.k_inv_pairs, s.k_ptr, s.num_k_graphs, s.num_k, (int)E, s.g_v);
    }
    if (B == 0 && red.n == 0) return 0;                      // no pair and no row to zero: nothing to launch
    if (B > 0) {
      const int64_t uq = ((int64_t)aq.p[0].units_q + aq.p[1].units_q) * H;
      const int64_t uk = ((int64_t)ak.p[0].units_k + ak.p[1].units_k) * H;
      if (int rc = launch<attn_bwd_pairs_dq_kernel<M>>(dim3((unsigned)((uq + WPB - 1) / WPB)), dim3(TPB), 0, st, aq)) return rc;
      if (int rc = launch<attn_bwd_pairs_dkv_kernel<M>>(dim3((unsigned)((uk + WPB - 1) / WPB)), dim3(TPB), 0, st, ak)) return rc;
    }
    if (int rc = launch_reduce(red, st)) return rc;
    return launch_status();
  });
}

}  // namespace

extern "C" int cgvp_pair_train_version(void) { return CGVP_PAIR_TRAIN_VERSION; }

extern "C" int64_t cgvp_attn_bwd_pairs_floats(const cgvp_attn_pairs_bwd_problem* probs, int32_t num_problems, int32_t heads,
                                              int32_t head_dim) {
  if (int rc = with_m(head_dim, [](auto) { return 0; })) return rc;          // (head_dim first, as everywhere)
  if (!probs || num_problems < 1 || num_problems > 2 || heads < 1) return CGVP_ERR_BAD_ARG;
  return plan_workspace(probs, num_problems, heads, (int64_t)heads * head_dim, nullptr);
}

extern "C" int cgvp_attn_bwd_pairs(const cgvp_attn_pairs_bwd_problem* probs, int32_t num_problems, int64_t num_pairs,
                                   int32_t heads, int32_t head_dim, float scale, float* workspace, int64_t workspace_floats,
                                   void* stream) {
  return bwd_pairs(probs, num_problems, num_pairs, heads, head_dim, scale, workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int cgvp_reduce_rows(const float* part, const int64_t* optr, const int64_t* inv_ptr, const int64_t* inv_pairs,
                                const int64_t* src_ptr, int64_t num_graphs, int64_t num_pairs, int64_t num_part, int64_t num_dst,
                                int32_t width, float* dst, void* stream) {
  const int64_t lim30 = (int64_t)1 << 30, lim33 = (int64_t)1 << 33;
  if (num_graphs < 0 || num_graphs >= lim30 || num_pairs < 0 || num_pairs >= lim30 || num_part < 0 || num_part >= lim33 ||
      num_dst < 0 || num_dst >= lim33 || width < 4 || width % 4)
    return CGVP_ERR_BAD_ARG;
  if (!optr || !inv_ptr || !inv_pairs || !src_ptr || (num_part > 0 && !part) || (num_dst > 0 && !dst)) return CGVP_ERR_BAD_ARG;
  if (!aligned(16, part, dst) || !aligned(8, optr, inv_ptr, inv_pairs, src_ptr)) return CGVP_ERR_BAD_ARG;
  ReduceArgs r;
  r.n = reduce_job(r.j[0], part, optr, inv_ptr, inv_pairs, src_ptr, num_graphs, num_dst, width, dst);
  if (r.n == 0) return 0;                                    // no graph or no row: nothing to launch
  if (int rc = launch_reduce(r, (hipStream_t)stream)) return rc;
  return launch_status();
}
