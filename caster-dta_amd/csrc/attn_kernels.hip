// attn_kernels.hip -- varlen multi-head cross attention between the residues and the atoms of each pair
// (SURVEY 8 f-1).  Replaces, for a CrossAttentionModule with head_dim 16, 32 or 64 (the shipped one: embed 128, 8 heads
// -> head_dim 16; include/caster_gvp_attnhd.h for the others), what
// nn.MultiheadAttention does between its input and output projections on `to_dense_batch`-padded tensors
// (joint_gnn.py:206-215, :379-380): per pair b and head h
//
//     O[q] = softmax_k( scale * Q[q] . K[k] ) V[k],   q in rows q_ptr[b]..q_ptr[b+1], k in rows k_ptr[b]..k_ptr[b+1]
//
// on the COMPACT row arrays ([N, E] residues / [Na, E] atoms with PyG ptr offsets): no padding to the longest
// protein, no [B, heads, Rmax, Amax] score tensor, no key-padding mask -- a pair only ever sees its own rows.
//
// Work unit: one wave per (16-query tile of one pair, head).  head_dim 16 = one v_mfma_f32_16x16x4_f32 tile:
//     S^T[key][q]  = sum_d K[key][d] Qs[q][d]    A = K rows  (lane (m = key, g): 4 dims as one float4), B = Qs rows
//     O^T[d][q]   += sum_key V[key][d] P[q][key]  A = V^T     (lane (m = d, g), k-slot r <-> key 4g + r), B = P
// The D tile of the first product (lane (n = q, g) holds keys 4g + r) IS the B operand of the second: scores never
// leave registers.  Online softmax over the key tiles (running max / sum per query; the 4 lanes of a query agree
// through two xor-shuffles), exact fp32 throughout.  The backward is two kernels without atomics: d Q with the same
// orientation (waves own query tiles), d K / d V with keys on the lanes (waves own key tiles and loop over the
// pair's query tiles); both recompute P from the saved log-sum-exp.
//
// head_dim 16 M, M in {1, 2, 4}: every kernel is a template on M (beside DROP).  The work unit, the lane orientation and
// the softmax are those above; a score product (S^T, dP, S) sums over M k-chunks -- chunk c holds the dims 16c + 4g + s,
// its float4 sits at column col + 16c + 4g -- and a product with a head_dim-wide output (O^T, d Qs, d V, d K) keeps M
// accumulator tiles, the transposed operand of tile c read at column col + 16c + n.  delta sums over all chunks before
// the lanes of a query are joined.  The dropout factor is a function of (head, q, k) alone: the same at every M.  M = 1 is
// the head_dim-16 code (every chunk loop has one trip).  The d K / d V kernel at M = 4 holds 64 accumulator registers,
// 32 of keys and twice 72 of (current, prefetched) query state: 194 VGPRs + 40 AGPRs with dropout, no scratch, two
// waves per SIMD (M = 1: four) -- so the full-tile prefetch is kept for every M and nothing is narrowed.
//
// Both directions of the module (residues -> atoms and atoms -> residues) go in ONE launch (two "problems") when their
// widths agree; a caller with unequal widths launches each direction on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/caster_gvp_attndrop.h"
#include "../../include/caster_gvp_attnhd.h"
#include "attn_common.h"
#include "gvp_rng.h"

namespace {

using namespace attn;
constexpr int WPB = 4, TPB = WAVE * WPB;

struct Prob {
  const float* q; const float* k; const float* v;         // [Nq][E], [Nk][E], [Nk][E]
  const int64_t* q_ptr; const int64_t* k_ptr;             // [B + 1]
  float* out; float* lse;                                  // [Nq][E], [Nq][H]
  const float* g_out; float* delta;                        // backward: d O [Nq][E]; delta [Nq][H] = sum_d dO . O
  float* g_q; float* g_k; float* g_v;
  float* w; int64_t w_lq, w_lk;                            // dense weights [B][w_lq][w_lk] (inference only)
  int32_t units_q, units_k;                                // upper bounds: (ceil(Nq/16) + B) and (ceil(Nk/16) + B)
};
struct Args { Prob p[2]; int nprob; int B; int H; int E; float scale; };

// ------------------------------------------------------------------------------------------------ attention dropout
// nn.MultiheadAttention's training arithmetic (include/caster_gvp_attndrop.h): the PROBABILITIES are dropped, after the
// softmax and before the product with V.  The three kernels are templates on (DROP, M); a DROP = true instantiation takes the
// per-problem generator arguments as a second kernel argument and multiplies the score tile, where it sits in registers,
// by factors f[q][k] in {0, 1/(1-p)} regenerated from (seed, offset, stream, head, q, k) (gvp_rng.h) -- nothing is
// stored.  The softmax normaliser and the saved log-sum-exp stay those of the undropped scores.
struct Drop { const unsigned long long* seed[2]; gvp::DropRule rule[2]; int stream[2]; };
struct NoDrop { int unused; };
template <bool DROP> using DropOf = std::conditional_t<DROP, Drop, NoDrop>;

// What a wave needs of its problem's generator.  `on` is wave-uniform: a problem with p = 0 beside one with p > 0 skips
// the generator and keeps factor 1.
struct Site { unsigned long long seed, offset; gvp::DropRule rule; int stream; bool on; };
__device__ __forceinline__ Site site_of(const Drop& d, int pi) {
  Site s;
  const unsigned long long* sp = pi ? d.seed[1] : d.seed[0];
  s.rule = pi ? d.rule[1] : d.rule[0];
  s.stream = pi ? d.stream[1] : d.stream[0];
  s.on = sp != nullptr && s.rule.thr < 65536u;
  s.seed = s.on ? sp[0] : 0ull;
  s.offset = s.on ? sp[1] : 0ull;
  return s;
}

// ------------------------------------------------------------------------------------------------ forward
template <bool DROP, int M>
__global__ __launch_bounds__(TPB) void attn_fwd_kernel(Args a, DropOf<DROP> d) {
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
  int64_t q0_, q_end_;
  if (!locate(P.q_ptr, a.B, t, lane, b, q0_, q_end_)) return;
  // rows and element offsets in 32 bits (the host checks rows x E < 2^31): a load is then base (SGPR pair) + one 32-bit
  // VGPR offset instead of a 64-bit multiply-add chain per address
  const int q0 = (int)q0_, q_end = (int)q_end_;
  const int k0 = (int)P.k_ptr[b], k_end = (int)P.k_ptr[b + 1];
  const int qr = q0 + n;
  const bool qv = qr < q_end;
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
  // The key-tile loop is a dependent chain (loads -> 4 MFMAs -> exp -> 4 MFMAs) and a pair's atoms attend to ~19 residue
  // tiles: the NEXT tile's K / V rows are loaded while the current one is computed (one global-load latency per wave
  // instead of one per key tile).
  //   S^T tile: lane (m = key, g) supplies K[key][16c + 4g..+3]; k-slot (s, g) of chunk c <-> dim 16c + 4g + s on both
  //   V^T operand of output tile c: lane (m = d - 16c, g), slot r <-> key kb + 4g + r
  // (loads are UNCONDITIONAL on rows clamped to the pair's last key and zeroed afterwards: with loads under lane masks
  // the compiler cannot count what is outstanding and waits for vmcnt(0), i.e. for the prefetch it has just issued)
  // element offsets of the tile's five loads, advanced by 16 rows per call and clamped to the pair's last key with one
  // 32-bit min each (offsets are monotone in the row)
  const unsigned k_step = TILE * E;
  const unsigned ko_last = (unsigned)(k_end - 1) * E + col + 4 * g, vo_last = (unsigned)(k_end - 1) * E + col + n;
  unsigned ko = (unsigned)(k0 + n) * E + col + 4 * g;
  unsigned vo[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) vo[r] = (unsigned)(k0 + 4 * g + r) * E + col + n;
  // Rows past the pair's last key are never zeroed: the clamp makes them copies of the last key's (finite) row, the tail
  // iteration sets their scores to -inf, and exp2(-inf) = 0 removes them from both sums.  Only the LAST tile of a pair can
  // be partial, so the loop over full tiles carries no masks at all (peeled tail).
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
  // DROP: this lane's 1 x 4 key run starts at key kb + 4g = 4 (kblk0 + g) + sk, sk the same for the whole pair
  [[maybe_unused]] Site S;
  [[maybe_unused]] unsigned sk = 0;
  if constexpr (DROP) { S = site_of(d, pi); sk = (unsigned)__builtin_amdgcn_readfirstlane(k0 & 3); }
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
    if constexpr (DROP) {                                   // after the row sum: l and the lse are the undropped ones
      if (S.on) {
        float f[4];
        gvp::attn_drop_run_k(S.seed, S.offset, S.stream, h, (unsigned)qr, ((unsigned)(kb - (int)sk) >> 2) + g, sk, S.rule, f);
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] *= f[r];           // (a key past the pair's end has p = 0 and stays 0)
      }
    }
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
    for (int c = 0; c < M; ++c) *reinterpret_cast<f4*>(P.out + ((unsigned)qr * E + col + 4 * g + TILE * c)) = acc[c] * inv;
    if (g == 0 && P.lse) P.lse[(unsigned)qr * a.H + h] = (l > 0.f) ? m + logf(l) : -INFINITY;
  }
}

// ------------------------------------------------------------------------------------------------ backward: d Q
// Same orientation as the forward.  Also writes delta[q][h] = sum_d dO[q][d] O[q][d] for the d K / d V kernel.
template <bool DROP, int M>
__global__ __launch_bounds__(TPB) void attn_bwd_dq_kernel(Args a, DropOf<DROP> d) {
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
  int64_t q0_, q_end_;
  if (!locate(P.q_ptr, a.B, t, lane, b, q0_, q_end_)) return;
  const int q0 = (int)q0_, q_end = (int)q_end_;                 // 32-bit rows / offsets, see attn_fwd_kernel
  const int k0 = (int)P.k_ptr[b], k_end = (int)P.k_ptr[b + 1];
  const int qr = q0 + n;
  const bool qv = qr < q_end;
  const unsigned E = a.E, col = h * HD;
  f4 qs[M], go[M], acc[M];
#pragma unroll
  for (int c = 0; c < M; ++c) qs[c] = go[c] = f4{0.f, 0.f, 0.f, 0.f};
  float lse = 0.f, dl = 0.f;
  if (qv) {
    const unsigned qo = (unsigned)qr * E + col + 4 * g;
#pragma unroll
    for (int c = 0; c < M; ++c) {                                   // delta: all chunks of the head, then the query's 4 lanes
      qs[c] = *reinterpret_cast<const f4*>(P.q + (qo + TILE * c)) * a.scale;
      go[c] = *reinterpret_cast<const f4*>(P.g_out + (qo + TILE * c));
      const f4 o = *reinterpret_cast<const f4*>(P.out + (qo + TILE * c));
      const float dc = go[c][0] * o[0] + go[c][1] * o[1] + go[c][2] * o[2] + go[c][3] * o[3];
      dl = c == 0 ? dc : dl + dc;
    }
    lse = P.lse[(unsigned)qr * a.H + h];
  }
  dl = quad_sum(dl);
  if (qv && g == 0) P.delta[(unsigned)qr * a.H + h] = dl;
#pragma unroll
  for (int c = 0; c < M; ++c) acc[c] = f4{0.f, 0.f, 0.f, 0.f};
  // next key tile prefetched while the current one is computed (see attn_fwd_kernel)
  //   ka: K^T operand of d Qs tile c: lane (m = d - 16c, g), slot r <-> key kb + 4g + r
  const unsigned k_step = TILE * E;                                // offsets advanced per call and clamped, see attn_fwd_kernel
  const unsigned ko_last = (unsigned)(k_end - 1) * E + col + 4 * g, to_last = (unsigned)(k_end - 1) * E + col + n;
  unsigned ko = (unsigned)(k0 + n) * E + col + 4 * g;
  unsigned to[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) to[r] = (unsigned)(k0 + 4 * g + r) * E + col + n;
  auto load_tile = [&](f4 (&kk)[M], f4 (&vv)[M], float (&ka)[M][4]) {   // the next 16 keys; no zeroing, tail peeled (attn_fwd_kernel)
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
  [[maybe_unused]] Site S;                                          // DROP: the forward's factors again, see attn_fwd_kernel
  [[maybe_unused]] unsigned sk = 0;
  if constexpr (DROP) { S = site_of(d, pi); sk = (unsigned)__builtin_amdgcn_readfirstlane(k0 & 3); }
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
    if constexpr (DROP) {                                           // d P = (d O V^T) o f
      if (S.on) {
        float f[4];
        gvp::attn_drop_run_k(S.seed, S.offset, S.stream, h, (unsigned)qr, ((unsigned)(kb - (int)sk) >> 2) + g, sk, S.rule, f);
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[r] *= f[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // (a lane without a query computes a finite column that is never stored; keys past the pair's end only in the tail)
      float pr = fexp(st[r] - lse);
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
    for (int c = 0; c < M; ++c) *reinterpret_cast<f4*>(P.g_q + ((unsigned)qr * E + col + 4 * g + TILE * c)) = acc[c] * a.scale;
  }
}

// ------------------------------------------------------------------------------------------------ backward: d K, d V
// Keys on the lanes: a wave owns a 16-key tile of one pair and loops over the pair's query tiles.
//   S[q][key]   = D[m = q][n = key]: A = Qs rows (lane (m = q, g): float4 of dims), B = K rows
//   dP[q][key]  = D[m = q][n = key]: A = dO rows, B = V rows
//   dV[key][d]  = D[m = d][n = key] += sum_q dO[q][d] P[q][key]   A: lane (m = d, g), slot r <-> query qb + 4g + r
//   dK[key][d]  = D[m = d][n = key] += sum_q Qs[q][d] dS[q][key]
template <bool DROP, int M>
__global__ __launch_bounds__(TPB) void attn_bwd_dkv_kernel(Args a, DropOf<DROP> d) {
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
  int64_t kt0_, k_end_;
  if (!locate(P.k_ptr, a.B, t, lane, b, kt0_, k_end_)) return;
  const int kt0 = (int)kt0_, k_end = (int)k_end_;               // 32-bit rows / offsets, see attn_fwd_kernel
  const int q0 = (int)P.q_ptr[b], q_end = (int)P.q_ptr[b + 1];
  const int kr = kt0 + n;
  const bool kv = kr < k_end;
  const unsigned E = a.E, col = h * HD, H = a.H;
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
  // next query tile prefetched while the current one is computed (an atom-key tile loops over ~19 residue tiles)
  struct QT { f4 qa[M], ga[M]; float lse[4], dl[4], qt[M][4], gt[M][4]; };
  const unsigned q_step = TILE * E, h_step = TILE * H;              // offsets advanced per call and clamped, see attn_fwd_kernel
  const unsigned qo_last = (unsigned)(q_end - 1) * E + col + 4 * g, to_last = (unsigned)(q_end - 1) * E + col + n,
                 ho_last = (unsigned)(q_end - 1) * H + h;
  unsigned qo = (unsigned)(q0 + n) * E + col + 4 * g;
  unsigned to[4], ho[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { to[r] = (unsigned)(q0 + 4 * g + r) * E + col + n; ho[r] = (unsigned)(q0 + 4 * g + r) * H + h; }
  auto load_tile = [&](QT& T) {                                     // the next 16 queries; no zeroing, tail peeled (attn_fwd_kernel)
    const unsigned qmo = qo < qo_last ? qo : qo_last;               // this lane's row as the M index of the two score products
#pragma unroll
    for (int c = 0; c < M; ++c) {
      T.qa[c] = *reinterpret_cast<const f4*>(P.q + (qmo + TILE * c)) * a.scale;
      T.ga[c] = *reinterpret_cast<const f4*>(P.g_out + (qmo + TILE * c));
    }
    qo += q_step;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                           // per k-slot r <-> query qb + 4g + r
      const unsigned tc = to[r] < to_last ? to[r] : to_last, hc = ho[r] < ho_last ? ho[r] : ho_last;
      to[r] += q_step; ho[r] += h_step;
      T.lse[r] = P.lse[hc];
      T.dl[r] = P.delta[hc];
#pragma unroll
      for (int c = 0; c < M; ++c) {
        T.qt[c][r] = P.q[tc + TILE * c] * a.scale;          // Qs^T operand of tile c: lane (m = d - 16c, g)
        T.gt[c][r] = P.g_out[tc + TILE * c];                // dO^T operand
      }
    }
  };
  QT nxt = {};
  if (q0 < q_end) load_tile(nxt);
  // DROP: this lane's 4 x 1 query run starts at query qb + 4g = 2 (h0 + 2g) + sq, sq the same for the whole pair; the
  // factors are those the forward applied to (query, key kr)
  [[maybe_unused]] Site S;
  [[maybe_unused]] unsigned sq = 0;
  if constexpr (DROP) { S = site_of(d, pi); sq = (unsigned)__builtin_amdgcn_readfirstlane(q0 & 1); }
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
    [[maybe_unused]] float f[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (DROP) {
      if (S.on)
        gvp::attn_drop_run_q(S.seed, S.offset, S.stream, h, ((unsigned)(qb - (int)sq) >> 1) + 2 * g, sq, (unsigned)kr, S.rule, f);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // (a lane without a key computes a finite column that is never stored; queries past the pair's end only in the tail)
      float pr = fexp(s[r] - lse[r]);
      if constexpr (decltype(tail)::value) pr = qb + 4 * g + r < q_end ? pr : 0.f;
      if constexpr (DROP) {                                 // d V = (P o f)^T d O,  d S = P o (d P o f - delta)
#pragma unroll
        for (int c = 0; c < M; ++c) {
          accv[c] = mfma(gt[c][r], pr * f[r], accv[c]);
          acck[c] = mfma(qt[c][r], pr * (dp[r] * f[r] - dl[r]), acck[c]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < M; ++c) {
          accv[c] = mfma(gt[c][r], pr, accv[c]);
          acck[c] = mfma(qt[c][r], pr * (dp[r] - dl[r]), acck[c]);
        }
      }
    }
  };
  int qb = q0;
  for (; qb + TILE <= q_end; qb += TILE) tile(qb, std::false_type{});
  if (qb < q_end) tile(qb, std::true_type{});
  if (kv) {
#pragma unroll
    for (int c = 0; c < M; ++c) {
      *reinterpret_cast<f4*>(P.g_v + ((unsigned)kr * E + col + 4 * g + TILE * c)) = accv[c];
      *reinterpret_cast<f4*>(P.g_k + ((unsigned)kr * E + col + 4 * g + TILE * c)) = acck[c];
    }
  }
}

// ------------------------------------------------------------------------------------------------ head-averaged weights
// nn.MultiheadAttention(need_weights=True, average_attn_weights=True): w[b][q][k] = mean_h P_h[q][k], written straight
// into the reference's dense layout [B][w_lq][w_lk] (zero elsewhere; the caller zero-fills; a pair with more than
// w_lq queries or w_lk keys is truncated to the layout, nothing is written outside it).  Inference only
// (inference/evaluation.py:43-66 slices it per pair); one wave per 16-query tile, all heads.
template <int M>
__global__ __launch_bounds__(TPB) void attn_weights_kernel(Args a) {
  constexpr int HD = TILE * M;
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  int64_t t = (int64_t)blockIdx.x * WPB + wave_id();
  int pi = 0;
  if (t >= a.p[0].units_q) { t -= a.p[0].units_q; pi = 1; }
  if (pi >= a.nprob) return;
  const Prob P = pick(a, pi);
  if (t >= P.units_q || !P.w) return;
  int b;
  int64_t q0, q_end;
  if (!locate(P.q_ptr, a.B, (int)t, lane, b, q0, q_end)) return;
  const int64_t k0 = P.k_ptr[b], k_end = P.k_ptr[b + 1], qbase = P.q_ptr[b];
  const int64_t qr = q0 + n;
  const bool qv = qr < q_end;
  const bool qw = qv && qr - qbase < P.w_lq;                     // a pair longer than the layout is truncated, never
  const int64_t k_stop = k_end < k0 + P.w_lk ? k_end : k0 + P.w_lk;   // written past [w_lq][w_lk]
  const int E = a.E;
  const float invh = 1.0f / (float)a.H;
  for (int64_t kb = k0; kb < k_stop; kb += TILE) {
    const int64_t kr = kb + n;
    f4 w = {0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < a.H; ++h) {
      const int col = h * HD;
      float lse = 0.f;
      if (qv) lse = P.lse[qr * a.H + h];
      f4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < M; ++c) {
        f4 qs = {0.f, 0.f, 0.f, 0.f}, kk = {0.f, 0.f, 0.f, 0.f};
        if (qv) qs = *reinterpret_cast<const f4*>(P.q + qr * E + col + TILE * c + 4 * g) * a.scale;
        if (kr < k_end) kk = *reinterpret_cast<const f4*>(P.k + kr * E + col + TILE * c + 4 * g);
#pragma unroll
        for (int s = 0; s < 4; ++s) st = mfma(kk[s], qs[s], st);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) w[r] += (qv && kb + 4 * g + r < k_end) ? fexp(st[r] - lse) * invh : 0.f;
    }
    if (qw) {
      float* row = P.w + ((int64_t)b * P.w_lq + (qr - qbase)) * P.w_lk + (kb - k0) + 4 * g;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kb + 4 * g + r < k_stop) row[r] = w[r];
    }
  }
}

// `long_first`: which of two problems gets the low workgroup indices -- the one whose waves loop longest (1: over the
// keys, the forward and d Q kernels; 2: over the queries, the d K / d V kernel).  Workgroups start in index order: with
// the residues -> atoms direction first, its 10k three-tile waves filled the chip and the 1.8k nineteen-tile waves of the
// other direction started last and ran alone at the end of the launch.
int fill(Args& a, const cgvp_attn_problem* probs, int nprob, int64_t B, int H, int HD, int long_first = 0, bool* swapped = nullptr) {
  if (!probs || nprob < 1 || nprob > 2 || B < 0 || H < 1) return CGVP_ERR_BAD_ARG;
  a.nprob = nprob; a.B = (int)B; a.H = H; a.E = H * HD;
  const bool swap = nprob == 2 && ((long_first == 1 && probs[1].num_k > probs[0].num_k) ||
                                   (long_first == 2 && probs[1].num_q > probs[0].num_q));
  if (swapped) *swapped = swap;
  for (int i = 0; i < 2; ++i) {
    Prob& p = a.p[i];
    p = Prob{};
    if (i >= nprob) continue;
    const cgvp_attn_problem& s = probs[swap ? 1 - i : i];
    if (!side_ok(s.num_q, s.q_ptr, (int64_t)H * HD) || !side_ok(s.num_k, s.k_ptr, (int64_t)H * HD)) return CGVP_ERR_BAD_ARG;
    if (s.num_q > 0 && (!s.q || !s.out || !s.lse)) return CGVP_ERR_BAD_ARG;
    if (s.num_k > 0 && (!s.k || !s.v)) return CGVP_ERR_BAD_ARG;
    if (!aligned(16, s.q, s.k, s.v, s.out, s.g_out, s.g_q, s.g_k, s.g_v)) return CGVP_ERR_BAD_ARG;
    p.q = s.q; p.k = s.k; p.v = s.v; p.q_ptr = s.q_ptr; p.k_ptr = s.k_ptr; p.out = s.out; p.lse = s.lse;
    p.g_out = s.g_out; p.delta = s.delta; p.g_q = s.g_q; p.g_k = s.g_k; p.g_v = s.g_v;
    p.w = s.weights; p.w_lq = s.weights_lq; p.w_lk = s.weights_lk;
    p.units_q = (int32_t)((s.num_q + TILE - 1) / TILE + B);
    p.units_k = (int32_t)((s.num_k + TILE - 1) / TILE + B);
  }
  return 0;
}

// The generator arguments of a call: 0 = no dropout anywhere (the DROP = false kernels run), 1 = at least one problem
// drops, < 0 = CGVP_ERR_BAD_ARG.  `nprob` has passed fill().
int drop_of(Drop& d, const cgvp_rng* rng, int nprob, int H) {
  d = Drop{};
  d.rule[0] = d.rule[1] = gvp::drop_rule(0.f);
  if (H > gvp::kAttnDropMaxHeads) return CGVP_ERR_BAD_ARG;      // the head has 7 bits of the counter
  int any = 0;
  for (int i = 0; rng && i < nprob; ++i) {
    const cgvp_rng& r = rng[i];
    if (!(r.p >= 0.f && r.p < 1.f) || ((uintptr_t)r.seed & 7)) return CGVP_ERR_BAD_ARG;       // (a NaN fails the first)
    if (!r.seed) continue;
    d.seed[i] = reinterpret_cast<const unsigned long long*>(r.seed);
    d.rule[i] = gvp::drop_rule(r.p);
    d.stream[i] = r.stream;
    any |= d.rule[i].thr < 65536u;
  }
  return any;
}
Drop ordered(const Drop& d, bool swap) {                          // in the order fill() gave the problems
  if (!swap) return d;
  return Drop{{d.seed[1], d.seed[0]}, {d.rule[1], d.rule[0]}, {d.stream[1], d.stream[0]}};
}

int attn_fwd(const cgvp_attn_problem* probs, int nprob, int64_t B, int H, int head_dim, float scale, const cgvp_rng* rng,
             bool check_rng, hipStream_t st) {
  return with_m(head_dim, [&](auto m) -> int {
    constexpr int M = decltype(m)::value;
    Args a;
    bool swap = false;
    if (int rc = fill(a, probs, nprob, B, H, TILE * M, 1, &swap)) return rc;
    a.scale = scale;
    Drop d;
    const int drop = check_rng ? drop_of(d, rng, nprob, H) : 0;
    if (drop < 0) return drop;
    if (B == 0) return 0;
    const int64_t units = ((int64_t)a.p[0].units_q + a.p[1].units_q) * H;
    const dim3 grid((unsigned)((units + WPB - 1) / WPB));
    if (drop) launch<attn_fwd_kernel<true, M>>(grid, dim3(TPB), 0, st, a, ordered(d, swap));
    else launch<attn_fwd_kernel<false, M>>(grid, dim3(TPB), 0, st, a, NoDrop{});
    return launch_status();
  });
}

int attn_bwd(const cgvp_attn_problem* probs, int nprob, int64_t B, int H, int head_dim, float scale, const cgvp_rng* rng,
             bool check_rng, hipStream_t st) {
  return with_m(head_dim, [&](auto m) -> int {
    constexpr int M = decltype(m)::value;
    Args a, ak;
    bool swap = false, swap_k = false;
    if (int rc = fill(a, probs, nprob, B, H, TILE * M, 1, &swap)) return rc;
    if (int rc = fill(ak, probs, nprob, B, H, TILE * M, 2, &swap_k)) return rc;
    a.scale = ak.scale = scale;
    for (int i = 0; i < nprob; ++i) {
      const cgvp_attn_problem& s = probs[i];
      if ((s.num_q > 0 && (!s.g_out || !s.g_q || !s.delta)) || (s.num_k > 0 && (!s.g_k || !s.g_v))) return CGVP_ERR_BAD_ARG;
    }
    Drop d;
    const int drop = check_rng ? drop_of(d, rng, nprob, H) : 0;
    if (drop < 0) return drop;
    if (B == 0) return 0;
    const int64_t uq = ((int64_t)a.p[0].units_q + a.p[1].units_q) * H;
    const int64_t uk = ((int64_t)a.p[0].units_k + a.p[1].units_k) * H;
    const dim3 gq((unsigned)((uq + WPB - 1) / WPB)), gk((unsigned)((uk + WPB - 1) / WPB));
    if (drop) {
      launch<attn_bwd_dq_kernel<true, M>>(gq, dim3(TPB), 0, st, a, ordered(d, swap));
      launch<attn_bwd_dkv_kernel<true, M>>(gk, dim3(TPB), 0, st, ak, ordered(d, swap_k));
    } else {
      launch<attn_bwd_dq_kernel<false, M>>(gq, dim3(TPB), 0, st, a, NoDrop{});
      launch<attn_bwd_dkv_kernel<false, M>>(gk, dim3(TPB), 0, st, ak, NoDrop{});
    }
    return launch_status();
  });
}

int attn_weights(const cgvp_attn_problem* probs, int nprob, int64_t B, int H, int head_dim, float scale, hipStream_t st) {
  return with_m(head_dim, [&](auto m) -> int {
    constexpr int M = decltype(m)::value;
    Args a;
    if (int rc = fill(a, probs, nprob, B, H, TILE * M)) return rc;
    a.scale = scale;
    for (int i = 0; i < nprob; ++i)
      if (!probs[i].weights || probs[i].weights_lq < 0 || probs[i].weights_lk < 0) return CGVP_ERR_BAD_ARG;
    if (B == 0) return 0;
    const int64_t tiles = (int64_t)a.p[0].units_q + a.p[1].units_q;
    launch<attn_weights_kernel<M>>(dim3((unsigned)((tiles + WPB - 1) / WPB)), dim3(TPB), 0, st, a);
    return launch_status();
  });
}

}  // namespace

extern "C" {

int cgvp_attn_fwd(const cgvp_attn_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads, float scale,
                  void* stream) {
  return attn_fwd(probs, num_problems, num_pairs, heads, 16, scale, nullptr, false, (hipStream_t)stream);
}

int cgvp_attn_weights(const cgvp_attn_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads, float scale,
                      void* stream) {
  return attn_weights(probs, num_problems, num_pairs, heads, 16, scale, (hipStream_t)stream);
}

int cgvp_attn_bwd(const cgvp_attn_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads, float scale,
                  void* stream) {
  return attn_bwd(probs, num_problems, num_pairs, heads, 16, scale, nullptr, false, (hipStream_t)stream);
}

// ---- include/caster_gvp_attndrop.h
int cgvp_attn_dropout_version(void) { return CGVP_ATTN_DROPOUT_VERSION; }

int cgvp_attn_fwd_dropout(const cgvp_attn_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads, float scale,
                          const cgvp_rng* rng, void* stream) {
  return attn_fwd(probs, num_problems, num_pairs, heads, 16, scale, rng, true, (hipStream_t)stream);
}

int cgvp_attn_bwd_dropout(const cgvp_attn_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads, float scale,
                          const cgvp_rng* rng, void* stream) {
  return attn_bwd(probs, num_problems, num_pairs, heads, 16, scale, rng, true, (hipStream_t)stream);
}

// ---- include/caster_gvp_attnhd.h: rng == NULL is cgvp_attn_fwd / cgvp_attn_bwd, anything else their _dropout forms
int cgvp_attn_hd_version(void) { return CGVP_ATTN_HD_VERSION; }

int cgvp_attn_fwd_hd(const cgvp_attn_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads, int32_t head_dim,
                     float scale, const cgvp_rng* rng, void* stream) {
  return attn_fwd(probs, num_problems, num_pairs, heads, head_dim, scale, rng, rng != nullptr, (hipStream_t)stream);
}

int cgvp_attn_bwd_hd(const cgvp_attn_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads, int32_t head_dim,
                     float scale, const cgvp_rng* rng, void* stream) {
  return attn_bwd(probs, num_problems, num_pairs, heads, head_dim, scale, rng, rng != nullptr, (hipStream_t)stream);
}

int cgvp_attn_weights_hd(const cgvp_attn_problem* probs, int32_t num_problems, int64_t num_pairs, int32_t heads,
                         int32_t head_dim, float scale, void* stream) {
  return attn_weights(probs, num_problems, num_pairs, heads, head_dim, scale, (hipStream_t)stream);
}

}  // extern "C"
