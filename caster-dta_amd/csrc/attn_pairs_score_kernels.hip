// attn_pairs_score_kernels.hip -- per-node attention scores of the varlen cross attention over a list of pairs of
// UNIQUE graphs (include/caster_gvp_pairscore.h; inference).
//
// attn_score_kernels.hip ties pair b to rows ptr[b] .. ptr[b+1] of q, k and lse alike: the scores of one protein against
// 1,024 drugs would need the protein's projected rows 1,024 times.  Here q / k hold every unique graph once, two index
// tables say which query graph and which key graph pair b uses, and only the lse (cgvp_attn_fwd_pairs wrote it per pair,
// at the query side's output offsets) and the two outputs (at the key side's output offsets) are per pair:
//
//     w[r][j] = (1/H) sum_h exp(scale Q_h[q_ptr[qg] + r] . K_h[k_ptr[kg] + j] - lse[qout_ptr[b] + r][h])
//     mean[kout_ptr[b] + j] = (1/nq) sum_r w[r][j],   max[kout_ptr[b] + j] = max_r w[r][j]
//
// Work unit: one workgroup per 16-key tile of one pair, ALL heads, found with attn::locate over kout_ptr.  From there on
// the kernel is attn_node_scores_kernel<H, M> of attn_score_kernels.hip restated -- keys on the lanes, K of all heads in
// registers, the 8 waves taking the pair's query tiles round robin, prefetched next query tile with unconditional loads
// clamped to the pair's last query, peeled partial tail, quad_sum / quad_max, LDS join in wave order, 32-bit element
// offsets -- so that a pair's arithmetic is the same instruction sequence on the same values:
// tests/test_pair_node_scores.py holds the two kernels together bitwise.  The only differences are where the first query
// row, the first key row, the lse row and the output row come from.  (Lifting the loop out of attn_score_kernels.hip
// instead would change the code of a measured kernel.)  No atomics: the order of every sum is fixed by the shapes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/caster_gvp_pairscore.h"
#include "attn_common.h"

namespace {

using namespace attn;
constexpr int WPB = 8, TPB = WAVE * WPB, MAX_H = 8;       // H M <= 8: an embed width of at most 128

struct Prob {
  const float* q; const float* k; const float* lse;       // [Nq][E], [Nk][E] rows of the unique graphs; [Nqo][H] per pair
  const int64_t* q_ptr; const int64_t* k_ptr;             // [Gq + 1], [Gk + 1]
  const int64_t* q_graph; const int64_t* k_graph;         // [B]
  const int64_t* qout_ptr; const int64_t* kout_ptr;       // [B + 1]: the pairs' rows in lse / in the outputs
  float* out_mean; float* out_max;                         // [Nko]
  int32_t units;                                           // upper bound of the key tiles: ceil(Nko / 16) + B
};
struct Args { Prob p[2]; int nprob; int B; float scale; };

template <int H, int M>
__global__ __launch_bounds__(TPB) void attn_node_scores_pairs_kernel(Args a) {
  constexpr int J = H * M;                                        // 16-dim chunks of a row: chunk h M + c of head h
  __shared__ float2 part[WPB][TILE];                              // per wave and key: {sum, max} of w over the wave's queries
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4, wv = wave_id();
  int64_t t = blockIdx.x;
  int pi = 0;
  if (t >= a.p[0].units) { t -= a.p[0].units; pi = 1; }
  if (pi >= a.nprob) return;                                      // (every exit up to the barrier is workgroup-uniform)
  const Prob P = pick(a, pi);
  if (t >= P.units) return;
  int b;
  int64_t ot0_, o_end_;
  if (!locate(P.kout_ptr, a.B, (int)t, lane, b, ot0_, o_end_)) return;
  // rows and element offsets in 32 bits (the host checks rows x E < 2^31 for q and k, rows x H for the lse)
  const int64_t qg = P.q_graph[b], kg = P.k_graph[b];
  const int ot0 = (int)ot0_, o_end = (int)o_end_, ob = (int)P.kout_ptr[b];
  const int q0 = (int)P.q_ptr[qg], q_end = (int)P.q_ptr[qg + 1];
  const int l0 = (int)P.qout_ptr[b];                              // the lse row of query q0
  const int kt0 = (int)P.k_ptr[kg] + (ot0 - ob), k_end = (int)P.k_ptr[kg] + (o_end - ob);   // (the pair's rows in the
  const int kr = kt0 + n, orow = ot0 + n;                         //  outputs ARE the key graph's length)
  const bool kv = kr < k_end;
  constexpr unsigned E = J * TILE;
  float sum = 0.f, mx = 0.f;                                      // weights are >= 0: 0 is the maximum of no query
  int qb = q0 + TILE * wv;                                        // this wave's first query tile; the stride is WPB tiles
  if (qb < q_end) {
    // K of every head: a lane behind the pair's last key reads that last key's row (the tile holds at least one key)
    // and computes a finite column that is never stored
    f4 kk[J];
    {
      const unsigned ko = (unsigned)(kv ? kr : k_end - 1) * E + 4 * g;
#pragma unroll
      for (int j = 0; j < J; ++j) kk[j] = *reinterpret_cast<const f4*>(P.k + ko + j * TILE);
    }
    // The next query tile is loaded while the current one is computed, unconditionally, on offsets that advance per
    // call and are clamped to the pair's last query (see attn_node_scores_kernel): rows behind q_end are copies of the
    // last query's and are zeroed in the peeled tail iteration only.  The lse offsets walk the PAIR's rows (l0 ..), the
    // query offsets the graph's (q0 ..): the same rows, row for row.
    struct QT { f4 qa[J]; float lse[4][H]; };
    const unsigned q_step = WPB * TILE * E, h_step = WPB * TILE * H;
    const unsigned qo_last = (unsigned)(q_end - 1) * E + 4 * g, ho_last = (unsigned)(l0 + (q_end - q0) - 1) * H;
    unsigned qo = (unsigned)(qb + n) * E + 4 * g;                 // this lane's row as the M index of the score product
    unsigned ho[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ho[r] = (unsigned)(l0 + (qb - q0) + 4 * g + r) * H;   // rows of D this lane holds: queries qb + 4g + r
    auto load_tile = [&](QT& T) {
      const unsigned qc = qo < qo_last ? qo : qo_last;
      qo += q_step;
#pragma unroll
      for (int j = 0; j < J; ++j) T.qa[j] = *reinterpret_cast<const f4*>(P.q + qc + j * TILE) * a.scale;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned hc = ho[r] < ho_last ? ho[r] : ho_last;
        ho[r] += h_step;
        if constexpr (H % 4 == 0) {
#pragma unroll
          for (int h = 0; h < H; h += 4) {
            const f4 l = *reinterpret_cast<const f4*>(P.lse + hc + h);
            T.lse[r][h] = l[0]; T.lse[r][h + 1] = l[1]; T.lse[r][h + 2] = l[2]; T.lse[r][h + 3] = l[3];
          }
        } else {
#pragma unroll
          for (int h = 0; h < H; ++h) T.lse[r][h] = P.lse[hc + h];
        }
      }
    };
    QT nxt;
    load_tile(nxt);
    auto tile = [&](int qt, auto tail) {
      const QT cur = nxt;
      load_tile(nxt);                                             // past the end: copies of the last query, never used
      float w[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < H; ++h) {
        f4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < M; ++c) {
#pragma unroll
          for (int x = 0; x < 4; ++x) s = mfma(cur.qa[h * M + c][x], kk[h * M + c][x], s);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] += fexp(fminf(s[r] - cur.lse[r][h], 0.f));   // a probability: never above 1
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = w[r];
        if constexpr (decltype(tail)::value) x = qt + 4 * g + r < q_end ? x : 0.f;
        sum += x;
        mx = fmaxf(mx, x);
      }
    };
    for (; qb + TILE <= q_end; qb += WPB * TILE) tile(qb, std::false_type{});
    if (qb < q_end) tile(qb, std::true_type{});                   // the pair's partial last tile belongs to one wave
    sum = quad_sum(sum);
    mx = quad_max(mx);
  }
  if (g == 0) part[wv][n] = make_float2(sum, mx);
  __syncthreads();
  if (wv != 0 || g != 0 || !kv) return;
  float s = 0.f, m = 0.f;
#pragma unroll
  for (int i = 0; i < WPB; ++i) {                                 // wave order: fixed
    const float2 p = part[i][n];
    s += p.x;
    m = fmaxf(m, p.y);
  }
  const float invh = 1.0f / (float)H;
  const int nq = q_end - q0;
  P.out_mean[orow] = nq > 0 ? s * invh / (float)nq : 0.f;
  P.out_max[orow] = m * invh;                                     // a positive factor: commutes with the maximum
}

template <int H, int M>
int launch_scores(unsigned grid, hipStream_t st, const Args& a) {
  return launch<attn_node_scores_pairs_kernel<H, M>>(dim3(grid), dim3(TPB), 0, st, a);
}

// heads 1 .. MAX_H / M of head_dim 16 M (the caller has checked the range)
template <int M>
int launch_heads(int heads, unsigned grid, hipStream_t st, const Args& a) {
  switch (heads) {
    case 1: return launch_scores<1, M>(grid, st, a);
    case 2: return launch_scores<2, M>(grid, st, a);
    case 3: if constexpr (3 * M <= MAX_H) return launch_scores<3, M>(grid, st, a); break;
    case 4: if constexpr (4 * M <= MAX_H) return launch_scores<4, M>(grid, st, a); break;
    case 5: if constexpr (5 * M <= MAX_H) return launch_scores<5, M>(grid, st, a); break;
    case 6: if constexpr (6 * M <= MAX_H) return launch_scores<6, M>(grid, st, a); break;
    case 7: if constexpr (7 * M <= MAX_H) return launch_scores<7, M>(grid, st, a); break;
    case 8: if constexpr (8 * M <= MAX_H) return launch_scores<8, M>(grid, st, a); break;
  }
  return CGVP_ERR_UNSUPPORTED_DIMS;
}

int node_scores_pairs(const cgvp_attn_pairs_score_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads,
                      int head_dim, float scale, void* stream) {
  return with_m(head_dim, [&](auto m) -> int {
    constexpr int M = decltype(m)::value;
    if (!probs || num_problems < 1 || num_problems > 2 || num_pairs < 0 || num_pairs >= ((int64_t)1 << 30) || heads < 1)
      return CGVP_ERR_BAD_ARG;
    if ((int64_t)heads * M > MAX_H) return CGVP_ERR_UNSUPPORTED_DIMS;
    const int64_t E = (int64_t)heads * TILE * M;
    Args a;
    a.nprob = num_problems; a.B = (int)num_pairs; a.scale = scale;
    // the problem whose key tiles walk the longer query graphs gets the low workgroup indices (they start first), as
    // cgvp_attn_node_scores orders its two
    const auto graphs = [](int64_t n) { return (double)(n > 0 ? n : 1); };
    const bool swap = num_problems == 2 && (double)probs[1].num_q * graphs(probs[0].num_q_graphs) >
                                               (double)probs[0].num_q * graphs(probs[1].num_q_graphs);
    for (int i = 0; i < 2; ++i) {
      Prob& p = a.p[i];
      p = Prob{};
      if (i >= num_problems) continue;
      const cgvp_attn_pairs_score_problem& s = probs[swap ? 1 - i : i];
      if (s.num_q_graphs < 0 || s.num_k_graphs < 0 || !s.q_graph || !s.k_graph) return CGVP_ERR_BAD_ARG;
      if (!side_ok(s.num_q, s.q_ptr, E) || !side_ok(s.num_k, s.k_ptr, E) || !side_ok(s.num_qout, s.qout_ptr, heads) ||
          !side_ok(s.num_kout, s.kout_ptr, 1))
        return CGVP_ERR_BAD_ARG;
      if ((s.num_q > 0 && !s.q) || (s.num_qout > 0 && !s.lse) || (s.num_k > 0 && !s.k)) return CGVP_ERR_BAD_ARG;
      if (s.num_kout > 0 && (!s.out_mean || !s.out_max)) return CGVP_ERR_BAD_ARG;
      if (!aligned(16, s.q, s.k) || !aligned(heads % 4 == 0 ? 16 : 4, s.lse) || !aligned(4, s.out_mean, s.out_max) ||
          !aligned(8, s.q_ptr, s.k_ptr, s.q_graph, s.k_graph, s.qout_ptr, s.kout_ptr))
        return CGVP_ERR_BAD_ARG;
      p.q = s.q; p.k = s.k; p.lse = s.lse; p.q_ptr = s.q_ptr; p.k_ptr = s.k_ptr; p.q_graph = s.q_graph; p.k_graph = s.k_graph;
      p.qout_ptr = s.qout_ptr; p.kout_ptr = s.kout_ptr; p.out_mean = s.out_mean; p.out_max = s.out_max;
      p.units = (int32_t)((s.num_kout + TILE - 1) / TILE + num_pairs);
    }
    if (num_pairs == 0) return 0;
    const unsigned grid = (unsigned)((int64_t)a.p[0].units + a.p[1].units);
    if (int rc = launch_heads<M>(heads, grid, (hipStream_t)stream, a)) return rc;
    return launch_status();
  });
}

}  // namespace

extern "C" int cgvp_pair_score_version(void) { return CGVP_PAIR_SCORE_VERSION; }

extern "C" int cgvp_attn_node_scores_pairs(const cgvp_attn_pairs_score_problem* probs, int32_t num_problems, int64_t num_pairs,
                                           int32_t heads, int32_t head_dim, float scale, void* stream) {
  return node_scores_pairs(probs, num_problems, num_pairs, heads, head_dim, scale, stream);
}
