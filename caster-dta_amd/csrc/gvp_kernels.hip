// gvp_kernels.hip -- three parts of libcaster_gvp.so (declarations and reference citations: include/caster_gvp.h):
//   * the round-1 one-item-per-lane kernels (node_embed, conv_fwd, node_update, gine_conv): what the fine-grained forward
//     entry points run when the caller passes no fragment image;
//   * the dropout plumbing (cgvp_rng checks, rng_next_kernel, dropout_masks_kernel);
//   * the fine-grained C ABI: each entry point validates its arguments, then dispatches to the tile kernels behind
//     namespace quad (gvp_internal.h) or to the kernels of this file.
// The CSR build, source-order index, collate and zero fill: graph_index_kernels.hip.  Whole passes: pass_api.hip.
// Mapping of the one-item-per-lane kernels: one residue / one edge per lane, 64-lane workgroups.
//   * conv: a workgroup owns `npw` consecutive TARGET nodes (dst-sorted CSR), so the rows it reduces into are private:
//     messages go lane -> LDS, a segmented reduction over the sorted targets runs in LDS, and the finished [npw][28]
//     block is written with coalesced stores -- no atomics, no zero-fill, bitwise reproducible.  The raw edge features
//     stream through the edge-embedding GVP + LayerNorm in registers (never materialised).
//   * node kernels: row-per-lane, outputs transposed through LDS so global stores are contiguous.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>

#include <initializer_list>

#include "gvp_internal.h"

using namespace gvp;

namespace {

constexpr int WAVE = 64;

inline int check_dims(const cgvp_dims* d) {
  if (!d) return CGVP_ERR_BAD_ARG;
  if (d->node_in_s != NODE_IN_S || d->node_in_v != NODE_IN_V || d->edge_in_s != EDGE_IN_S ||
      d->edge_in_v != EDGE_IN_V || d->hidden_s != NS || d->hidden_v != NV ||
      d->edge_hidden_s != ES || d->edge_hidden_v != EV || d->out_s != OUT)
    return CGVP_ERR_UNSUPPORTED_DIMS;
  if (d->storage != CGVP_F32 && d->storage != CGVP_BF16) return CGVP_ERR_UNSUPPORTED_DIMS;
  if (d->layer_kind < CGVP_LAYER_GATED || d->layer_kind > CGVP_LAYER_LINEAR) return CGVP_ERR_UNSUPPORTED_DIMS;
  if (d->layer_kind != CGVP_LAYER_GATED && d->storage != CGVP_F32) return CGVP_ERR_UNSUPPORTED_DIMS;
  return 0;
}
// entry points that exist for CASTER-DTA's gated layers only (embeddings, head, fused layer, whole passes)
inline int check_dims_gated(const cgvp_dims* d) {
  if (int rc = check_dims(d)) return rc;
  return d->layer_kind == CGVP_LAYER_GATED ? 0 : CGVP_ERR_UNSUPPORTED_DIMS;
}
// tile policy index of the MFMA launchers (gvp_internal.h): storage type for the gated kind, else the layer kind
inline int policy_of(const cgvp_dims* d) {
  if (d->layer_kind == CGVP_LAYER_GVPDEF) return POLICY_GVPDEF;
  if (d->layer_kind == CGVP_LAYER_LINEAR) return POLICY_LINEAR;
  return d->storage == CGVP_BF16 ? POLICY_BF16 : POLICY_F32;
}

inline EncLayout cvt(const cgvp_layout& l) {
  EncLayout L;
  L.nt_node = l.nt_node; L.nt_edge = l.nt_edge; L.node_gvp = l.node_gvp; L.node_ln = l.node_ln;
  L.edge_gvp = l.edge_gvp; L.edge_ln = l.edge_ln; L.conv0 = l.conv0; L.conv_stride = l.conv_stride;
  L.ln_out = l.ln_out; L.head = l.head; L.total = l.total;
  return L;
}

// one of the pointers is not 16-byte aligned (float4 row accesses); NULL passes: most of these buffers are optional
inline bool misaligned16(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs) if ((uintptr_t)q & 15) return true;
  return false;
}

// float offsets of the layout's slices inside the fragment image
inline int image_offsets(const cgvp_layout& l, QuadOffsets* o) {
  return quad::offsets(l.nt_node, l.nt_edge, num_convs_of(l), o);
}
// what every fine-grained backward entry point looks up first: the image offsets and the slab row sizes of the layout
struct BwdLookup : QuadOffsets { quad::BwdBlocks blk; };
inline int bwd_lookup(const cgvp_layout& l, BwdLookup* o) {
  if (int rc = image_offsets(l, o)) return rc;
  return quad::bwd_block_sizes(l.nt_node, l.nt_edge, &o->blk);
}
// ... and what it ends with: the slab segments go to the caller (who reduces them with the rest of the pass) or are
// reduced into grad_params now
inline int emit_segments(const cgvp_segment* sg, int n, cgvp_segment* segs, int32_t* nsegs, float* grad_params,
                         hipStream_t st, int overwrite = 0, bool store_only = false) {
  if (segs && nsegs) { for (int k = 0; k < n; ++k) segs[k] = sg[k]; *nsegs = n; }
  else quad::reduce_segments(sg, n, grad_params, st, overwrite, store_only);
  return launch_status();
}

// Launder the arena pointer through an empty asm so the optimiser cannot hoist
// (loop-invariant) weight addresses / constant-space loads out of a loop body
// and then spill them: weights are re-read from the scalar cache per iteration.
__device__ __forceinline__ const float* opaque(const float* p) {
  asm volatile("" : "+s"(p));
  return p;
}

// ------------------------------------------------------------- row staging
// Coalesced copy of `count` floats global -> LDS rows of ROWLEN with stride RS.
template <int ROWLEN, int RS>
__device__ __forceinline__ void stage_in(const float* __restrict__ g, int count, float* lds, int lane) {
  for (int i = lane; i < count; i += WAVE) lds[(i / ROWLEN) * RS + (i % ROWLEN)] = g[i];
}
template <int ROWLEN, int RS>
__device__ __forceinline__ void stage_out(float* __restrict__ g, int count, const float* lds, int lane) {
  for (int i = lane; i < count; i += WAVE) g[i] = lds[(i / ROWLEN) * RS + (i % ROWLEN)];
}

__device__ __forceinline__ void load_row28(const float* __restrict__ base, int64_t row, float (&r)[ROW]) {
  const float4* p = reinterpret_cast<const float4*>(base + row * ROW);
#pragma unroll
  for (int i = 0; i < ROW / 4; ++i) {
    float4 q = p[i];
    r[4 * i] = q.x; r[4 * i + 1] = q.y; r[4 * i + 2] = q.z; r[4 * i + 3] = q.w;
  }
}

// ------------------------------------------------------------- node embed
struct NodeEmbedArgs {
  const float* params; EncLayout L; const float* x_s; const float* x_v; const int64_t* ntypes;
  int64_t N; float* h;
};

template <int NTN>
__global__ __launch_bounds__(WAVE) void node_embed_kernel(NodeEmbedArgs a) {
  constexpr int RS_S = NODE_IN_S;              // 17: odd stride, conflict-free
  constexpr int RS_V = 3 * NODE_IN_V;          // 9
  constexpr int RS_O = ROW + 1;                // 29
  __shared__ float lds[WAVE * RS_O];           // reused: inputs (17+9 per row) then outputs
  const int lane = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * WAVE;
  const int cnt = (int)((a.N - n0 < WAVE) ? (a.N - n0) : WAVE);
  float* lds_s = lds;
  float* lds_v = lds + WAVE * RS_S;
  stage_in<NODE_IN_S, RS_S>(a.x_s + n0 * NODE_IN_S, cnt * NODE_IN_S, lds_s, lane);
  stage_in<RS_V, RS_V>(a.x_v + n0 * RS_V, cnt * RS_V, lds_v, lane);
  __syncthreads();
  float row[ROW];
  if (lane < cnt) {
    float xs[NODE_IN_S], xv[NODE_IN_V][3];
#pragma unroll
    for (int k = 0; k < NODE_IN_S; ++k) xs[k] = lds_s[lane * RS_S + k];
#pragma unroll
    for (int i = 0; i < NODE_IN_V; ++i)
#pragma unroll
      for (int d = 0; d < 3; ++d) xv[i][d] = lds_v[lane * RS_V + 3 * i + d];
    int type = 0;
    if (NTN > 0) {
      type = (int)a.ntypes[n0 + lane];
      type = type < 0 ? 0 : (type >= NTN ? NTN - 1 : type);
    }
    node_embed_item<NTN>(a.params, a.L, type, xs, xv, row);
  }
  __syncthreads();
  if (lane < cnt) {
#pragma unroll
    for (int k = 0; k < ROW; ++k) lds[lane * RS_O + k] = row[k];
  }
  __syncthreads();
  stage_out<ROW, RS_O>(a.h + n0 * ROW, cnt * ROW, lds, lane);
}

// ------------------------------------------------------------- conv
struct ConvArgs {
  const float* params; EncLayout L; int layer;
  const float* h; const float* e_s; const float* e_v; const int64_t* etypes;
  const int32_t* rowptr; const int32_t* eperm; const int32_t* esrc; const int32_t* edst;
  int64_t N; int npw; int mean; float* dh;
};

template <int NTE>
__global__ __launch_bounds__(WAVE) void conv_fwd_kernel(ConvArgs a) {
  constexpr int RS = ROW + 1;                  // 29
  __shared__ float msg[WAVE * RS];
  __shared__ float acc[WAVE * ROW];
  __shared__ int dloc[WAVE];
  const int lane = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * a.npw;
  const int nn = (int)((a.N - n0 < a.npw) ? (a.N - n0) : a.npw);
  const int32_t e0 = a.rowptr[n0], e1 = a.rowptr[n0 + nn];
  for (int i = lane; i < nn * ROW; i += WAVE) acc[i] = 0.f;

  for (int32_t base = e0; base < e1; base += WAVE) {
    const int32_t p = base + lane;
    const bool active = p < e1;
    float m[ROW];
    int dl = -1;
    if (active) {
      const int32_t eid = a.eperm[p];
      const int32_t src = a.esrc[p];
      const int32_t dst = a.edst[p];
      dl = dst - (int)n0;
      float es_raw[EDGE_IN_S], ev_raw[EDGE_IN_V][3], xj[ROW], xi[ROW];
      const float4* pe = reinterpret_cast<const float4*>(a.e_s + (int64_t)eid * EDGE_IN_S);
#pragma unroll
      for (int i = 0; i < EDGE_IN_S / 4; ++i) {
        float4 q = pe[i];
        es_raw[4 * i] = q.x; es_raw[4 * i + 1] = q.y; es_raw[4 * i + 2] = q.z; es_raw[4 * i + 3] = q.w;
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) ev_raw[0][d] = a.e_v[(int64_t)eid * 3 + d];
      int et = 0;
      if (NTE > 0) {
        et = (int)a.etypes[eid];
        et = et < 0 ? 0 : (et >= NTE ? NTE - 1 : et);
      }
      load_row28(a.h, src, xj);
      load_row28(a.h, dst, xi);
      conv_message_item<NTE>(opaque(a.params), a.L, a.layer, et, es_raw, ev_raw, xj, xi, m);
    }
    __syncthreads();                           // previous chunk's reduction has drained msg[]
    if (active) {
#pragma unroll
      for (int k = 0; k < ROW; ++k) msg[lane * RS + k] = m[k];
    }
    dloc[lane] = dl;
    __syncthreads();
    // Segmented reduction over the (sorted) targets of this chunk.  Lanes 0..27
    // walk rows 0..31, lanes 32..59 walk rows 32..63, one channel each.  Only the
    // second half's FIRST segment can share a node with the first half, so it is
    // held back and added after a barrier; every other flush is exclusive.
    const int cntc = (e1 - base < WAVE) ? (e1 - base) : WAVE;
    const int half = lane >> 5, c = lane & 31;
    const int r0 = half * 32, r1 = (cntc < r0 + 32) ? cntc : r0 + 32;
    float first_run = 0.f;
    int first_cur = -1;
    if (c < ROW && r0 < r1) {
      int cur = dloc[r0];
      float run = 0.f;
      bool first = true;
      for (int r = r0; r < r1; ++r) {
        const int d = dloc[r];
        if (d != cur) {
          if (first && half == 1) { first_run = run; first_cur = cur; }
          else acc[cur * ROW + c] += run;
          first = false;
          run = 0.f;
          cur = d;
        }
        run += msg[r * RS + c];
      }
      if (first && half == 1) { first_run = run; first_cur = cur; }
      else acc[cur * ROW + c] += run;
    }
    __syncthreads();
    if (first_cur >= 0) acc[first_cur * ROW + c] += first_run;
  }
  __syncthreads();
  float* out = a.dh + n0 * ROW;
  for (int i = lane; i < nn * ROW; i += WAVE) {
    float v = acc[i];
    if (a.mean) {
      const int nd = i / ROW;
      const int deg = a.rowptr[n0 + nd + 1] - a.rowptr[n0 + nd];
      v = v / (float)(deg > 1 ? deg : 1);
    }
    out[i] = v;
  }
}

// ------------------------------------------------------------- node update
struct NodeUpdateArgs {
  const float* params; EncLayout L; int layer;
  const float* h; const float* dh; int64_t N; float* h_out; float* out;
};

template <bool HEAD>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(1, 1)))
void node_update_kernel(NodeUpdateArgs a) {
  constexpr int RS = HEAD ? (OUT + 1) : (ROW + 1);
  __shared__ float lds[WAVE * RS];
  const int lane = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * WAVE;
  const int cnt = (int)((a.N - n0 < WAVE) ? (a.N - n0) : WAVE);
  float row_keep[HEAD ? ROW : 1];
  if (lane < cnt) {
    float x[ROW], dh[ROW], row[ROW], out[OUT];
    load_row28(a.h, n0 + lane, x);
    load_row28(a.dh, n0 + lane, dh);
    node_update_item<HEAD>(a.params, a.L, a.layer, x, dh, row, out);
    if (HEAD) {
#pragma unroll
      for (int k = 0; k < ROW; ++k) row_keep[k] = row[k];
#pragma unroll
      for (int k = 0; k < OUT; ++k) lds[lane * RS + k] = out[k];
    } else {
#pragma unroll
      for (int k = 0; k < ROW; ++k) lds[lane * RS + k] = row[k];
    }
  }
  __syncthreads();
  if (HEAD) stage_out<OUT, RS>(a.out + n0 * OUT, cnt * OUT, lds, lane);
  else stage_out<ROW, RS>(a.h_out + n0 * ROW, cnt * ROW, lds, lane);
  if (HEAD && a.h_out) {                      // optional with the head: the head's input, kept for a backward pass
    __syncthreads();
    if (lane < cnt) {
#pragma unroll
      for (int k = 0; k < ROW; ++k) lds[lane * RS + k] = row_keep[k];
    }
    __syncthreads();
    stage_out<ROW, RS>(a.h_out + n0 * ROW, cnt * ROW, lds, lane);
  }
}

// ------------------------------------------------------------- GINE
struct GineArgs {
  const float* x; const int64_t* ntypes; int nt; const float* eattr; const int64_t* etypes;
  int net; int ed; const int32_t* rowptr; const int32_t* eperm; const int32_t* esrc;
  int64_t N; int cin; int chid; int cout;
  const float* eps; const float* we; const float* be; const float* w0; const float* b0;
  const float* w1; const float* b1; float slope; float* out;
  const float* mask;     // optional [N][cout] dropout factors applied after the activation
  gvp::RngArgs rng;      // ... or generated in the kernel (mask == NULL, rng.seed != NULL)
};

constexpr int GINE_APB = 4;   // atoms (waves) per block
constexpr int GINE_MAXKE = 16;

// One wave per target atom, one lane per channel.  The two MLP matrices are
// staged once per workgroup in LDS with odd row strides (cin+1 / chid+1), so the
// "lane o reads row o" pattern of the mat-vecs is bank-conflict free instead of a
// 64-cache-line gather from global memory per k.
__global__ __launch_bounds__(WAVE * GINE_APB) void gine_conv_kernel(GineArgs a) {
  extern __shared__ float gsm[];
  const int s0 = a.cin + 1, s1 = a.chid + 1;
  float* w0s = gsm;                                   // [chid][cin + 1]
  float* w1s = w0s + a.chid * s0;                     // [cout][chid + 1]
  float (*hbuf)[WAVE] = reinterpret_cast<float (*)[WAVE]>(w1s + a.cout * s1);
  float (*tbuf)[WAVE] = hbuf + GINE_APB;
  for (int k = threadIdx.x; k < a.chid * a.cin; k += WAVE * GINE_APB) w0s[(k / a.cin) * s0 + k % a.cin] = a.w0[k];
  for (int k = threadIdx.x; k < a.cout * a.chid; k += WAVE * GINE_APB) w1s[(k / a.chid) * s1 + k % a.chid] = a.w1[k];
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * GINE_APB + w;
  const bool valid = i < a.N;
  const int ke = a.net + a.ed;
  const int xw = a.cin - a.nt;                  // raw feature width
  float hval = 0.f;
  // The atom's edge metadata is fetched lane-parallel (lane q <- q-th incoming edge) and handed to the
  // channel lanes by readlane, so an atom costs three dependent memory hops (rowptr -> eperm/esrc ->
  // bond features / source row) instead of three per edge.
  int32_t p0 = 0, p1 = 0;
  if (valid) { p0 = a.rowptr[i]; p1 = a.rowptr[i + 1]; }
  p0 = __builtin_amdgcn_readfirstlane(p0);
  p1 = __builtin_amdgcn_readfirstlane(p1);
  float wa[GINE_MAXKE];                          // this channel's W_e columns for the bond features
  float bias = 0.f;
  if (lane < a.cin) {
#pragma unroll
    for (int k = 0; k < GINE_MAXKE; ++k) wa[k] = (k < a.ed) ? a.we[lane * ke + a.net + k] : 0.f;
    bias = a.be[lane];
  }
  auto xcat = [&](int64_t n) -> float {
    if (lane < a.nt) return ((int)a.ntypes[n] == lane) ? 1.f : 0.f;
    return a.x[n * xw + (lane - a.nt)];
  };
  float agg = 0.f;
  for (int32_t c0 = p0; c0 < p1; c0 += WAVE) {
    const int n = (p1 - c0 < WAVE) ? (p1 - c0) : WAVE;
    int32_t m_eid = 0, m_src = 0, m_et = 0;
    if (lane < n) {
      m_eid = a.eperm[c0 + lane];
      m_src = a.esrc[c0 + lane];
      if (a.net > 0) {                            // one-hot bond type = column lookup
        m_et = (int)a.etypes[m_eid];
        m_et = m_et < 0 ? 0 : (m_et >= a.net ? a.net - 1 : m_et);
      }
    }
#pragma unroll 4
    for (int q = 0; q < n; ++q) {
      const int32_t eid = __builtin_amdgcn_readlane(m_eid, q);
      const int32_t j = __builtin_amdgcn_readlane(m_src, q);
      const int32_t et = __builtin_amdgcn_readlane(m_et, q);
      if (lane < a.cin) {
        float e = bias;
        if (a.net > 0) e += a.we[lane * ke + et];
        const float* ea = a.eattr + (int64_t)eid * a.ed;
#pragma unroll
        for (int k = 0; k < GINE_MAXKE; ++k)
          if (k < a.ed) e = fmaf(wa[k], ea[k], e);
        const float mj = xcat(j) + e;
        agg += mj > 0.f ? mj : 0.f;
      }
    }
  }
  if (valid && lane < a.cin) hval = fmaf(1.0f + a.eps[0], xcat(i), agg);
  hbuf[w][lane] = hval;
  __syncthreads();
  float t = 0.f;
  if (valid && lane < a.chid) {
    t = a.b0[lane];
    const float* wr = w0s + lane * s0;
    for (int k = 0; k < a.cin; ++k) t = fmaf(wr[k], hbuf[w][k], t);
    t = t > 0.f ? t : t * a.slope;
  }
  tbuf[w][lane] = t;
  __syncthreads();
  if (valid && lane < a.cout) {
    float y = a.b1[lane];
    const float* wr = w1s + lane * s1;
    for (int k = 0; k < a.chid; ++k) y = fmaf(wr[k], tbuf[w][k], y);
    y = y > 0.f ? y : y * a.slope;
    if (a.mask) y *= a.mask[i * a.cout + lane];
    else if (a.rng.seed) {
      float f[4];
      gvp::dropout4(a.rng.seed[0], a.rng.seed[1], a.rng.stream, i, lane >> 2, a.rng.p, f);
      y *= f[lane & 3];
    }
    a.out[i * a.cout + lane] = y;
  }
}

// ------------------------------------------------------------- GINE backward
// Runs on 16-atom MFMA tiles: gine_quad_kernels.hip.  The layer's gradient block is in state_dict
// order  eps | nn.lins.0.weight | nn.lins.0.bias | nn.lins.1.weight | nn.lins.1.bias | lin.weight | lin.bias
// (gine_layer_floats, gvp_internal.h).

}  // namespace

// ------------------------------------------------------------- dropout plumbing
static int check_rng(const cgvp_rng* rng) {
  if (!rng || !rng->seed) return 0;
  if (!(rng->p >= 0.f && rng->p < 1.f) || rng->stream < 0 || ((uintptr_t)rng->seed & 7)) return CGVP_ERR_BAD_ARG;
  return 0;
}
// kernel-argument form
static gvp::RngArgs rng_args(const cgvp_rng* rng) {
  if (!rng || !rng->seed) return gvp::RngArgs{nullptr, 0.f, 0};
  return gvp::RngArgs{reinterpret_cast<const unsigned long long*>(rng->seed), rng->p, rng->stream};
}

__global__ void rng_next_kernel(unsigned long long* state, unsigned long long* out) {
  const unsigned long long off = state[1] + 1;
  state[1] = off;
  out[0] = state[0];
  out[1] = off;
}
// cgvp_rng_next without its checks (the CSR build calls it when it has no count launch to advance the generator in)
int quad::rng_next(unsigned long long* state, unsigned long long* out, hipStream_t st) {
  return launch<rng_next_kernel>(dim3(1), dim3(1), 0, st, state, out);
}

struct MaskArgs { gvp::RngArgs rng; int num_masks; int64_t N; int width; float* out; };
__global__ __launch_bounds__(256) void dropout_masks_kernel(MaskArgs a) {
  const int64_t per = a.N * (a.width / 4), total = per * a.num_masks;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(t / per);
    const int64_t r = t - (int64_t)m * per, n = r / (a.width / 4);
    const int blk = (int)(r - n * (a.width / 4));
    float* row = a.out + ((int64_t)m * a.N + n) * a.width;
    if (a.width == 20) {                 // protein row: quarter g = blk of [16 scalar | 4 vector-channel] (blk 4 is covered by 0..3)
      if (blk < 4) {
        float fs[4], fv;
        gvp::dropout_row20(a.rng.seed[0], a.rng.seed[1], a.rng.stream + m, n, blk, a.rng.p, fs, fv);
        row[4 * blk] = fs[0]; row[4 * blk + 1] = fs[1]; row[4 * blk + 2] = fs[2]; row[4 * blk + 3] = fs[3];
        row[16 + blk] = fv;
      }
    } else {
      float f[4];
      gvp::dropout4(a.rng.seed[0], a.rng.seed[1], a.rng.stream + m, n, blk, a.rng.p, f);
      row[4 * blk] = f[0]; row[4 * blk + 1] = f[1]; row[4 * blk + 2] = f[2]; row[4 * blk + 3] = f[3];
    }
  }
}

bool quad::deterministic_env() {
  static const bool v = [] { const char* e = getenv("CGVP_DETERMINISTIC"); return e && e[0] == '1'; }();
  return v;
}

// ===================================================================== C ABI
extern "C" {

int cgvp_abi_version(void) { return CGVP_ABI_VERSION; }
const char* cgvp_build_info(void) { return "libcaster_gvp gfx950 (HIP, wave64), built " __DATE__ " " __TIME__; }

int cgvp_deterministic_forced(void) { return quad::deterministic_env() ? 1 : 0; }

int cgvp_lba_layout(const cgvp_dims* dims, int32_t num_ntypes, int32_t num_etypes, int32_t num_convs,
                    cgvp_layout* out) {
  if (int rc = check_dims(dims)) return rc;
  if (!out || num_ntypes < 0 || num_etypes < 0 || num_convs < 0) return CGVP_ERR_BAD_ARG;
  const EncLayout L = make_layout(num_ntypes, num_etypes, num_convs);
  out->nt_node = L.nt_node; out->nt_edge = L.nt_edge; out->node_gvp = L.node_gvp; out->node_ln = L.node_ln;
  out->edge_gvp = L.edge_gvp; out->edge_ln = L.edge_ln; out->conv0 = L.conv0;
  out->conv_stride = L.conv_stride; out->ln_out = L.ln_out; out->head = L.head; out->total = L.total;
  return 0;
}

int64_t cgvp_lba_image_floats(const cgvp_dims* dims, const cgvp_layout* layout) {
  if (int rc = check_dims(dims)) return rc;
  if (!layout) return CGVP_ERR_BAD_ARG;
  QuadOffsets o;
  if (int rc = image_offsets(*layout, &o)) return rc;
  return o.total;
}

int cgvp_lba_prepare(const cgvp_dims* dims, const cgvp_layout* layout, const float* params, float* image,
                     void* stream) {
  if (int rc = check_dims(dims)) return rc;
  if (!layout || !params || !image) return CGVP_ERR_BAD_ARG;
  // bf16 storage: the fragments of every GEMM with K > 4 are packed as bf16 for v_mfma_f32_16x16x16_bf16 (gvp_quad.h)
  if (int rc = quad::prepare(cvt(*layout), num_convs_of(*layout), policy_of(dims) == POLICY_BF16 ? 1 : 0, params, image, (hipStream_t)stream)) return rc;
  return launch_status();
}

int cgvp_lba_pass_begin(const cgvp_dims* dims, const cgvp_layout* layout, const float* params, float* image,
                        const float* x_s, const float* x_v, const int64_t* ntypes, int64_t N, float* h,
                        uint64_t* rng_state, uint64_t* rng_out, const int64_t* edge_index, int64_t E,
                        int32_t* csr_counters, void* stream) {
  if (int rc = check_dims_gated(dims)) return rc;
  if (N < 0 || E < 0 || !layout || !params || !image || (layout->nt_node > 0 && N > 0 && !ntypes)) return CGVP_ERR_BAD_ARG;
  if ((rng_state != nullptr) != (rng_out != nullptr)) return CGVP_ERR_BAD_ARG;
  if (((uintptr_t)rng_state & 7) || ((uintptr_t)rng_out & 7) || misaligned16({h, image})) return CGVP_ERR_BAD_ARG;
  if ((edge_index != nullptr) != (csr_counters != nullptr)) return CGVP_ERR_BAD_ARG;
  if (N > 0 && (!x_s || !x_v || !h)) return CGVP_ERR_BAD_ARG;
  if (N >= (int64_t)1 << 31 || E >= (int64_t)1 << 31) return CGVP_ERR_BAD_ARG;
  if (N == 0 && rng_state)           // no embedding block exists to do the hand-off
    if (int rc = cgvp_rng_next(rng_state, rng_out, stream)) return rc;
  if (int rc = quad::pass_begin(cvt(*layout), num_convs_of(*layout), policy_of(dims), params, image, x_s, x_v, ntypes, N, h,
                                reinterpret_cast<unsigned long long*>(rng_state), reinterpret_cast<unsigned long long*>(rng_out),
                                edge_index, E, csr_counters, (hipStream_t)stream)) return rc;
  return launch_status();
}

int cgvp_node_embed_fwd(const cgvp_dims* dims, const cgvp_layout* layout, const float* params,
                        const float* image, const float* x_s, const float* x_v, const int64_t* ntypes,
                        int64_t N, float* h, uint64_t* rng_state, uint64_t* rng_out, void* stream) {
  if (int rc = check_dims_gated(dims)) return rc;
  if (N < 0 || !layout || !params || (layout->nt_node > 0 && N > 0 && !ntypes)) return CGVP_ERR_BAD_ARG;
  if ((rng_state != nullptr) != (rng_out != nullptr) || (rng_state && !image)) return CGVP_ERR_BAD_ARG;
  if (((uintptr_t)rng_state & 7) || ((uintptr_t)rng_out & 7)) return CGVP_ERR_BAD_ARG;
  if (N == 0) return rng_state ? cgvp_rng_next(rng_state, rng_out, stream) : 0;
  if (!x_s || !x_v || !h) return CGVP_ERR_BAD_ARG;
  if (image) {
    if (misaligned16({h})) return CGVP_ERR_BAD_ARG;
    QuadOffsets o;
    if (int rc = image_offsets(*layout, &o)) return rc;
    if (int rc = quad::node_embed(layout->nt_node, image + o.emb, x_s, x_v, ntypes, N, h,
                                  reinterpret_cast<unsigned long long*>(rng_state),
                                  reinterpret_cast<unsigned long long*>(rng_out), policy_of(dims), (hipStream_t)stream)) return rc;
    return launch_status();
  }
  if (policy_of(dims)) return CGVP_ERR_UNSUPPORTED_DIMS;      // bf16 storage is a feature of the MFMA kernels
  NodeEmbedArgs a{params, cvt(*layout), x_s, x_v, ntypes, N, h};
  const dim3 grid((unsigned)((N + WAVE - 1) / WAVE));
  hipStream_t st = (hipStream_t)stream;
  switch (layout->nt_node) {   // one-hot width is a compile-time constant of the kernel
    case 0: launch<node_embed_kernel<0>>(grid, dim3(WAVE), 0, st, a); break;
    case 20: launch<node_embed_kernel<20>>(grid, dim3(WAVE), 0, st, a); break;
    case 21: launch<node_embed_kernel<21>>(grid, dim3(WAVE), 0, st, a); break;
    default: return CGVP_ERR_UNSUPPORTED_DIMS;
  }
  return launch_status();
}

int cgvp_conv_fwd(const cgvp_dims* dims, const cgvp_layout* layout, const float* params,
                  const float* image, int32_t layer,
                  const float* h, const float* e_s, const float* e_v, const int64_t* etypes,
                  const int32_t* rowptr, const int32_t* eperm, const int32_t* esrc,
                  const int32_t* edst, int64_t N, int64_t E, int32_t aggr_mean, const float* e_in,
                  float* e_out, float* dh, void* stream) {
  if (int rc = check_dims(dims)) return rc;
  if (N < 0 || E < 0 || !layout || !params) return CGVP_ERR_BAD_ARG;
  if (layer < 0 || layer >= num_convs_of(*layout)) return CGVP_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!h || !dh || !rowptr) return CGVP_ERR_BAD_ARG;
  if (!image && (e_in || e_out)) return CGVP_ERR_BAD_ARG;      // the stored edge embedding is a feature of the MFMA kernels
  if (E > 0 && (!esrc || !edst)) return CGVP_ERR_BAD_ARG;
  if (E > 0 && !e_in && (!e_s || !e_v || !eperm || (layout->nt_edge > 0 && !etypes))) return CGVP_ERR_BAD_ARG;
  if (misaligned16({h, e_s, e_in, e_out})) return CGVP_ERR_BAD_ARG;   // float4 row loads
  if (image) {
    QuadOffsets o;
    if (int rc = image_offsets(*layout, &o)) return rc;
    if (int rc = quad::conv(layout->nt_edge, image + o.conv0 + layer * o.layer_stride, h, e_s, e_v, etypes, rowptr,
                            eperm, esrc, edst, N, E, aggr_mean ? 1 : 0, dh, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, gvp::RngArgs{nullptr, 0.f, 0}, e_in, e_in ? nullptr : e_out, policy_of(dims),
                            (hipStream_t)stream)) return rc;
    return launch_status();
  }
  if (policy_of(dims)) return CGVP_ERR_UNSUPPORTED_DIMS;
  // target nodes per workgroup: aim at ~48 of the 64 edge lanes per chunk
  int64_t deg = (E + N - 1) / N;
  if (deg < 1) deg = 1;
  int npw = (int)(48 / deg);
  npw = npw < 1 ? 1 : (npw > WAVE ? WAVE : npw);
  ConvArgs a{params, cvt(*layout), layer, h, e_s, e_v, etypes, rowptr, eperm, esrc, edst, N, npw,
             aggr_mean ? 1 : 0, dh};
  const dim3 grid((unsigned)((N + npw - 1) / npw));
  hipStream_t st = (hipStream_t)stream;
  switch (layout->nt_edge) {
    case 0: launch<conv_fwd_kernel<0>>(grid, dim3(WAVE), 0, st, a); break;
    case 1: launch<conv_fwd_kernel<1>>(grid, dim3(WAVE), 0, st, a); break;
    default: return CGVP_ERR_UNSUPPORTED_DIMS;
  }
  return launch_status();
}

int cgvp_conv_layer_fwd(const cgvp_dims* dims, const cgvp_layout* layout, const float* image, int32_t layer,
                        const float* h, const float* e_s, const float* e_v, const int64_t* etypes,
                        const int32_t* rowptr, const int32_t* eperm, const int32_t* esrc, const int32_t* edst,
                        int64_t N, int64_t E, int32_t aggr_mean, const float* mask0, const float* mask1,
                        const cgvp_rng* rng, int32_t with_head, const float* e_in, float* e_out, float* dh,
                        float* h_out, float* out, void* stream) {
  if (int rc = check_dims_gated(dims)) return rc;
  if (int rc = check_rng(rng)) return rc;
  if (N < 0 || E < 0 || !layout || !image) return CGVP_ERR_BAD_ARG;
  if (layer < 0 || layer >= num_convs_of(*layout)) return CGVP_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!h || !rowptr || (with_head ? !out : !h_out)) return CGVP_ERR_BAD_ARG;
  if (E > 0 && (!esrc || !edst)) return CGVP_ERR_BAD_ARG;
  if (E > 0 && !e_in && (!e_s || !e_v || !eperm || (layout->nt_edge > 0 && !etypes))) return CGVP_ERR_BAD_ARG;
  if (misaligned16({h, e_s, dh, h_out, out, mask0, mask1, e_in, e_out})) return CGVP_ERR_BAD_ARG;
  QuadOffsets o;
  if (int rc = image_offsets(*layout, &o)) return rc;
  if (int rc = quad::conv(layout->nt_edge, image + o.conv0 + layer * o.layer_stride, h, e_s, e_v, etypes, rowptr, eperm,
                          esrc, edst, N, E, aggr_mean ? 1 : 0, dh, with_head ? 2 : 1,
                          image + o.node0 + layer * o.layer_stride, image + o.head, h_out, out, mask0, mask1,
                          rng_args(rng), e_in, e_in ? nullptr : e_out, policy_of(dims), (hipStream_t)stream)) return rc;
  return launch_status();
}

int cgvp_node_update_fwd(const cgvp_dims* dims, const cgvp_layout* layout, const float* params,
                         const float* image, int32_t layer, const float* h, const float* dh, int64_t N,
                         int32_t with_head, float* h_out, float* out, void* stream) {
  if (int rc = check_dims(dims)) return rc;
  if (N < 0 || !layout || !params) return CGVP_ERR_BAD_ARG;
  if (layer < 0 || layer >= num_convs_of(*layout)) return CGVP_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!h || !dh || (with_head ? !out : !h_out)) return CGVP_ERR_BAD_ARG;
  if (misaligned16({h, dh})) return CGVP_ERR_BAD_ARG;
  if (image) {
    if (misaligned16({h_out, out})) return CGVP_ERR_BAD_ARG;
    QuadOffsets o;
    if (int rc = image_offsets(*layout, &o)) return rc;
    if (int rc = quad::node_update(image + o.node0 + layer * o.layer_stride, image + o.head, h, dh, N,
                                   with_head ? 1 : 0, h_out, out, nullptr, nullptr, gvp::RngArgs{nullptr, 0.f, 0},
                                   policy_of(dims), (hipStream_t)stream)) return rc;
    return launch_status();
  }
  if (policy_of(dims)) return CGVP_ERR_UNSUPPORTED_DIMS;
  NodeUpdateArgs a{params, cvt(*layout), layer, h, dh, N, h_out, out};
  dim3 grid((unsigned)((N + WAVE - 1) / WAVE));
  if (with_head) launch<node_update_kernel<true>>(grid, dim3(WAVE), 0, (hipStream_t)stream, a);
  else launch<node_update_kernel<false>>(grid, dim3(WAVE), 0, (hipStream_t)stream, a);
  return launch_status();
}

int cgvp_node_update_fwd_train(const cgvp_dims* dims, const cgvp_layout* layout, const float* image,
                               int32_t layer, const float* h, const float* dh, const float* mask0,
                               const float* mask1, const cgvp_rng* rng, int64_t N, int32_t with_head, float* h_out,
                               float* out, void* stream) {
  if (int rc = check_dims(dims)) return rc;
  if (int rc = check_rng(rng)) return rc;
  if (N < 0 || !layout || !image) return CGVP_ERR_BAD_ARG;
  if (layer < 0 || layer >= num_convs_of(*layout)) return CGVP_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!h || !dh || (with_head ? !out : !h_out)) return CGVP_ERR_BAD_ARG;
  if (misaligned16({h, dh, h_out, out, mask0, mask1})) return CGVP_ERR_BAD_ARG;
  QuadOffsets o;
  if (int rc = image_offsets(*layout, &o)) return rc;
  if (int rc = quad::node_update(image + o.node0 + layer * o.layer_stride, image + o.head, h, dh, N,
                                 with_head ? 1 : 0, h_out, out, mask0, mask1, rng_args(rng),
                                 policy_of(dims), (hipStream_t)stream)) return rc;
  return launch_status();
}

int64_t cgvp_bwd_workspace_floats(const cgvp_dims* dims, const cgvp_layout* layout) {
  if (int rc = check_dims(dims)) return rc;
  if (!layout) return CGVP_ERR_BAD_ARG;
  quad::BwdBlocks b;
  if (int rc = quad::bwd_block_sizes(layout->nt_node, layout->nt_edge, &b)) return rc;
  int mx = b.emb > b.conv_total ? b.emb : b.conv_total;
  mx = mx > b.node + b.head ? mx : b.node + b.head;
  mx = mx > 2 * b.conv_edge ? mx : 2 * b.conv_edge;            // the edge stage runs two workgroups per CU (2 x kBwdMaxGrid slab rows)
  return (int64_t)kBwdMaxGrid * mx;
}

int cgvp_node_update_bwd(const cgvp_dims* dims, const cgvp_layout* layout, const float* image, int32_t layer,
                         const float* h, const float* dh, const float* mask0, const float* mask1,
                         const cgvp_rng* rng, const float* h_out, const float* g_out, const float* g_up0, const float* g_up1,
                         const float* g_up2, int64_t N, int32_t with_head, float* g_dh, float* g_h,
                         float* zero_out, float* grad_params, float* workspace, cgvp_segment* segs, int32_t* nsegs,
                         void* stream) {
  if (int rc = check_dims(dims)) return rc;
  if (int rc = check_rng(rng)) return rc;
  if (N < 0 || !layout || !image || !grad_params || !workspace) return CGVP_ERR_BAD_ARG;
  const int nc = num_convs_of(*layout);
  if (layer < 0 || layer >= nc) return CGVP_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!h || !dh || !g_dh || (with_head && (!g_out || !h_out))) return CGVP_ERR_BAD_ARG;
  if (with_head && dims->layer_kind != CGVP_LAYER_GATED) return CGVP_ERR_UNSUPPORTED_DIMS;     // the head is CASTER-DTA's
  if (misaligned16({h, dh, mask0, mask1, h_out, g_out, g_up0, g_up1, g_up2, g_dh, g_h, zero_out})) return CGVP_ERR_BAD_ARG;
  BwdLookup o;
  if (int rc = bwd_lookup(*layout, &o)) return rc;
  int grid = 0, hgrid = 0;
  hipStream_t st = (hipStream_t)stream;
  float* head_slab = workspace + (size_t)kBwdMaxGrid * o.blk.node;
  // CGVP_SPLIT_HEAD_BWD=1 keeps the head stage in a launch of its own (A/B switch; the results are the same)
  static const bool split_head = [] { const char* e = getenv("CGVP_SPLIT_HEAD_BWD"); return e && e[0] == '1'; }();
  if (with_head && !split_head) {
    // the head's d h_out lands in g_dh and is consumed in place as the node stage's upstream, inside ONE launch
    if (int rc = quad::node_head_bwd(image + o.head, image + o.headT, h_out, g_out, g_dh, head_slab,
                                     image + o.node0 + layer * o.layer_stride, image + o.nodeT0 + layer * o.layerT_stride,
                                     h, dh, mask0, mask1, rng_args(rng), N, g_dh, g_h, zero_out, workspace, &grid,
                                     policy_of(dims), st)) return rc;
    hgrid = grid;
  } else {
  if (with_head) {
    if (int rc = quad::head_bwd(image + o.head, image + o.headT, h_out, g_out, N, g_dh, head_slab, &hgrid, policy_of(dims), st)) return rc;
    g_up0 = g_dh; g_up1 = nullptr; g_up2 = nullptr;
  }
  if (int rc = quad::node_update_bwd(image + o.node0 + layer * o.layer_stride, image + o.nodeT0 + layer * o.layerT_stride,
                                     h, dh, mask0, mask1, rng_args(rng), g_up0, g_up1, g_up2, N, g_dh, g_h, zero_out,
                                     workspace, &grid, policy_of(dims), st)) return rc;
  }
  const int node_len = conv_ff1() + LFf1::size(0) - conv_ln0();          // norm.0 .. end of ff_func.1
  cgvp_segment sg[2] = {{workspace, grid, o.blk.node, 0, node_len, layout->conv0 + layer * layout->conv_stride + conv_ln0()},
                        {head_slab, hgrid, o.blk.head, 0, layout->total - layout->ln_out, layout->ln_out}};
  return emit_segments(sg, with_head ? 2 : 1, segs, nsegs, grad_params, st);
}

int cgvp_conv_bwd(const cgvp_dims* dims, const cgvp_layout* layout, const float* image, int32_t layer,
                  const float* h, const float* e_emb, const int32_t* rowptr, const int32_t* esrc,
                  const int32_t* edst, int64_t N, int64_t E, int32_t aggr_mean, const float* g_dh, float* g_src,
                  int32_t g_src_zeroed, float* g_dst, float* g_e, float* grad_params, float* workspace,
                  cgvp_segment* segs, int32_t* nsegs, void* stream) {
  if (quad::deterministic_env()) return CGVP_ERR_NONDETERMINISTIC;     // d h[src] by float atomics
  return quad::conv_bwd_entry(dims, layout, image, layer, h, e_emb, rowptr, esrc, edst, N, E, aggr_mean, g_dh, g_src,
                              g_src_zeroed, g_dst, g_e, grad_params, workspace, segs, nsegs, stream, nullptr);
}
}  // extern "C"

// cgvp_conv_bwd; det != NULL: the deterministic mode (store d h[src] rows, then one per-source sum launch into g_src,
// which needs no zero fill)
int quad::conv_bwd_entry(const cgvp_dims* dims, const cgvp_layout* layout, const float* image, int32_t layer,
                         const float* h, const float* e_emb, const int32_t* rowptr, const int32_t* esrc,
                         const int32_t* edst, int64_t N, int64_t E, int32_t aggr_mean, const float* g_dh, float* g_src,
                         int32_t g_src_zeroed, float* g_dst, float* g_e, float* grad_params, float* workspace,
                         cgvp_segment* segs, int32_t* nsegs, void* stream, const quad::DetBufs* det) {
  if (int rc = check_dims(dims)) return rc;
  if (N < 0 || E < 0 || !layout || !image || !grad_params || !workspace) return CGVP_ERR_BAD_ARG;
  const int nc = num_convs_of(*layout);
  if (layer < 0 || layer >= nc) return CGVP_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!h || !g_dh || !g_src || !g_dst || !rowptr) return CGVP_ERR_BAD_ARG;
  if (E > 0 && (!e_emb || !g_e || !esrc || !edst)) return CGVP_ERR_BAD_ARG;
  if (misaligned16({h, e_emb, g_dh, g_src, g_dst, g_e})) return CGVP_ERR_BAD_ARG;
  BwdLookup o;
  if (int rc = bwd_lookup(*layout, &o)) return rc;
  int grid = 0;
  hipStream_t st = (hipStream_t)stream;
  if (!g_src_zeroed && !det) quad::zero_words(g_src, (size_t)N * ROW, st);
  if (int rc = quad::conv_bwd(layout->nt_edge, image + o.conv0 + layer * o.layer_stride,
                              image + o.convT0 + layer * o.layerT_stride, h, e_emb, rowptr, esrc, edst, N, E,
                              aggr_mean ? 1 : 0, g_dh, g_src, g_dst, g_e, workspace, &grid, policy_of(dims), st,
                              det ? det->rows : nullptr, det ? det->slot : nullptr)) return rc;
  if (det)
    if (int rc = quad::src_sum(ROW, det->rows, nullptr, det->sptr, det->spos, rowptr, det->slot, (int64_t)grid * 8, N, g_src, st))
      return rc;
  const cgvp_segment sg{workspace, grid, o.blk.conv_total, 0, conv_ln0(), layout->conv0 + layer * layout->conv_stride};
  return emit_segments(&sg, 1, segs, nsegs, grad_params, st, det ? 1 : 0, det != nullptr);
}

extern "C" {

int64_t cgvp_conv_bwd_det_floats(int64_t num_nodes, int64_t num_edges) {
  if (num_nodes < 0 || num_edges < 0) return CGVP_ERR_BAD_ARG;
  return (num_edges > 0 ? num_edges : 1) * ROW + (int64_t)quad::conv_bwd_max_waves() * ROW;
}

int cgvp_conv_bwd_ex(const cgvp_dims* dims, const cgvp_layout* layout, const float* image, int32_t layer,
                     const float* h, const float* e_emb, const int32_t* rowptr, const int32_t* esrc,
                     const int32_t* edst, int64_t N, int64_t E, int32_t aggr_mean, const float* g_dh, float* g_src,
                     int32_t g_src_zeroed, float* g_dst, float* g_e, float* grad_params, float* workspace,
                     cgvp_segment* segs, int32_t* nsegs, const int32_t* sptr, const int32_t* spos, float* det_scratch,
                     int32_t flags, void* stream) {
  if (!((flags & CGVP_BWD_DETERMINISTIC) || quad::deterministic_env()))
    return quad::conv_bwd_entry(dims, layout, image, layer, h, e_emb, rowptr, esrc, edst, N, E, aggr_mean, g_dh, g_src,
                                g_src_zeroed, g_dst, g_e, grad_params, workspace, segs, nsegs, stream, nullptr);
  if (!sptr || !det_scratch || (E > 0 && !spos) || misaligned16({det_scratch})) return CGVP_ERR_BAD_ARG;
  const quad::DetBufs db{sptr, spos, det_scratch, det_scratch + (E > 0 ? E : 1) * ROW};
  return quad::conv_bwd_entry(dims, layout, image, layer, h, e_emb, rowptr, esrc, edst, N, E, aggr_mean, g_dh, g_src,
                              g_src_zeroed, g_dst, g_e, grad_params, workspace, segs, nsegs, stream, &db);
}

int cgvp_edge_embed_bwd(const cgvp_dims* dims, const cgvp_layout* layout, const float* image, const float* e_s,
                        const float* e_v, const int64_t* etypes, const int32_t* eperm, int64_t E,
                        const float* const* g_e, int32_t num_g, float* g_e_s, float* g_e_v, float* grad_params,
                        float* workspace, cgvp_segment* segs, int32_t* nsegs, void* stream) {
  if (int rc = check_dims_gated(dims)) return rc;
  if (E < 0 || !layout || !image || !grad_params || !workspace || !g_e || num_g < 1) return CGVP_ERR_BAD_ARG;
  if ((g_e_s == nullptr) != (g_e_v == nullptr) || misaligned16({g_e_s})) return CGVP_ERR_BAD_ARG;
  if (segs && nsegs) *nsegs = 0;
  if (E == 0) return 0;
  if (!e_s || !e_v || !eperm || (layout->nt_edge > 0 && !etypes)) return CGVP_ERR_BAD_ARG;
  if (misaligned16({e_s})) return CGVP_ERR_BAD_ARG;
  for (int l = 0; l < num_g; ++l) if (!g_e[l] || misaligned16({g_e[l]})) return CGVP_ERR_BAD_ARG;
  BwdLookup o;
  if (int rc = bwd_lookup(*layout, &o)) return rc;
  int grid = 0;
  hipStream_t st = (hipStream_t)stream;
  if (g_e_s) {        // edges the CSR build dropped (endpoint out of range) are in no tile: their rows stay zero
    quad::zero_words(g_e_s, (size_t)E * EDGE_IN_S, st);
    quad::zero_words(g_e_v, (size_t)E * EDGE_IN_V * 3, st);
  }
  // gvp_edge's fragments are the head of every conv slice (identical in all layers): layer 0's is used
  if (int rc = quad::edge_embed_bwd(layout->nt_edge, image + o.conv0, image + o.convT0, e_s, e_v, etypes, eperm, E, g_e,
                                    num_g, g_e_s, g_e_v, workspace, &grid, policy_of(dims), st)) return rc;
  const cgvp_segment sg{workspace, grid, o.blk.conv_edge, 0, layout->conv0 - layout->edge_gvp, layout->edge_gvp};
  return emit_segments(&sg, 1, segs, nsegs, grad_params, st);
}

int cgvp_node_embed_bwd(const cgvp_dims* dims, const cgvp_layout* layout, const float* image, const float* x_s,
                        const float* x_v, const int64_t* ntypes, int64_t N, const float* g_up0,
                        const float* g_up1, const float* g_up2, float* g_x_s, float* g_x_v, float* grad_params,
                        float* workspace, cgvp_segment* segs, int32_t* nsegs, void* stream) {
  if (int rc = check_dims_gated(dims)) return rc;
  if (N < 0 || !layout || !image || !grad_params || !workspace) return CGVP_ERR_BAD_ARG;
  if (N == 0) return 0;
  if (!x_s || !x_v || (layout->nt_node > 0 && !ntypes) || ((g_x_s == nullptr) != (g_x_v == nullptr))) return CGVP_ERR_BAD_ARG;
  if (misaligned16({g_up0, g_up1, g_up2})) return CGVP_ERR_BAD_ARG;
  BwdLookup o;
  if (int rc = bwd_lookup(*layout, &o)) return rc;
  int grid = 0;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = quad::node_embed_bwd(layout->nt_node, image + o.emb, image + o.embT, x_s, x_v, ntypes, N, g_up0, g_up1,
                                    g_up2, g_x_s, g_x_v, workspace, &grid, policy_of(dims), st)) return rc;
  const cgvp_segment sg{workspace, grid, o.blk.emb, 0, layout->edge_gvp - layout->node_gvp, layout->node_gvp};
  return emit_segments(&sg, 1, segs, nsegs, grad_params, st);
}

int cgvp_gine_conv_fwd(const float* x, const int64_t* ntypes, int32_t num_ntypes, const float* eattr,
                       const int64_t* etypes, int32_t num_etypes, int32_t edge_dim,
                       const int32_t* rowptr, const int32_t* eperm, const int32_t* esrc, const int32_t* edst,
                       int64_t N, int64_t E, int32_t cin, int32_t chid, int32_t cout, const cgvp_gine_w* w,
                       float act_slope, const float* mask, const cgvp_rng* rng, int32_t variant, float* out,
                       void* stream) {
  if (N < 0 || E < 0 || !w) return CGVP_ERR_BAD_ARG;
  if (int rc = check_rng(rng)) return rc;
  const gvp::RngArgs ra = rng_args(rng);
  if (num_ntypes < 0 || num_etypes < 0 || edge_dim < 0 || cin <= num_ntypes) return CGVP_ERR_BAD_ARG;
  if (cin > WAVE || chid > WAVE || cout > WAVE || chid < 1 || cout < 1 || num_etypes + edge_dim > GINE_MAXKE)
    return CGVP_ERR_UNSUPPORTED_DIMS;
  if (N == 0) return 0;
  if (!x || !out || !rowptr || (num_ntypes > 0 && !ntypes)) return CGVP_ERR_BAD_ARG;
  if (E > 0 && (!eperm || !esrc || (edge_dim > 0 && !eattr) || (num_etypes > 0 && !etypes))) return CGVP_ERR_BAD_ARG;
  // variant 0: 16-atom MFMA tiles when the layer shape is compiled (needs edst and 16-B aligned
  // out / mask); variant 1 or any other shape: generic one-wave-per-atom kernel
  if (variant == 0 && edst && !misaligned16({out, mask})) {
    const int rc = quad::gine_fwd(cin, chid, cout, num_ntypes, num_etypes, edge_dim, x, ntypes, eattr, etypes, rowptr,
                                  eperm, esrc, edst, N, w, act_slope, mask, ra, out, nullptr, nullptr, (hipStream_t)stream);
    if (rc <= 0) return rc < 0 ? rc : launch_status();
  }
  GineArgs a{x, ntypes, num_ntypes, eattr, etypes, num_etypes, edge_dim, rowptr, eperm, esrc, N, cin,
             chid, cout, w->eps, w->we, w->be, w->w0, w->b0, w->w1, w->b1, act_slope, out, mask, ra};
  const size_t lds = (size_t)(chid * (cin + 1) + cout * (chid + 1) + 2 * GINE_APB * WAVE) * sizeof(float);
  launch<gine_conv_kernel>(dim3((unsigned)((N + GINE_APB - 1) / GINE_APB)),
                           dim3(WAVE * GINE_APB), lds, (hipStream_t)stream, a);
  return launch_status();
}

int cgvp_rng_next(uint64_t* state, uint64_t* out, void* stream) {
  if (!state || !out || ((uintptr_t)state & 7) || ((uintptr_t)out & 7)) return CGVP_ERR_BAD_ARG;
  quad::rng_next(reinterpret_cast<unsigned long long*>(state), reinterpret_cast<unsigned long long*>(out), (hipStream_t)stream);
  return launch_status();
}

int cgvp_dropout_masks(const cgvp_rng* rng, int32_t num_masks, int64_t N, int32_t width, float* out, void* stream) {
  if (!rng || !rng->seed || !out || num_masks < 1 || N < 0 || width < 4 || (width & 3)) return CGVP_ERR_BAD_ARG;
  if (int rc = check_rng(rng)) return rc;
  if (N == 0) return 0;
  MaskArgs a{rng_args(rng), num_masks, N, width, out};
  const int64_t total = (int64_t)num_masks * N * (width / 4);
  launch<dropout_masks_kernel>(dim3((unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256)), dim3(256), 0,
                               (hipStream_t)stream, a);
  return launch_status();
}

int cgvp_bwd_reduce(const cgvp_segment* segs, int32_t nsegs, float* grad_params, int32_t overwrite, void* stream) {
  if (!segs || nsegs < 0 || nsegs > CGVP_MAX_SEGS || !grad_params) return CGVP_ERR_BAD_ARG;
  quad::reduce_segments(segs, nsegs, grad_params, (hipStream_t)stream, overwrite ? 1 : 0);
  return launch_status();
}

int64_t cgvp_gine_bwd_workspace_floats(void) { return (int64_t)quad::kGineBwdMaxGrid * quad::gine_max_slab_row(); }   // the largest compiled layer: (64,64,64)

int cgvp_gine_conv_bwd(const float* x, const int64_t* ntypes, int32_t num_ntypes, const float* eattr,
                       const int64_t* etypes, int32_t num_etypes, int32_t edge_dim, const int32_t* rowptr,
                       const int32_t* eperm, const int32_t* esrc, const int32_t* edst, int64_t N, int64_t E,
                       int32_t cin, int32_t chid, int32_t cout, const cgvp_gine_w* w, float act_slope,
                       const float* mask, const cgvp_rng* rng, const float* g_out, float* g_x, float* grad_layer,
                       float* workspace, int32_t max_workgroups, void* stream) {
  if (N < 0 || E < 0 || !w || !grad_layer || !workspace) return CGVP_ERR_BAD_ARG;
  if (int rc = check_rng(rng)) return rc;
  if (quad::deterministic_env() && g_x) return CGVP_ERR_NONDETERMINISTIC;     // d x by float atomics
  if (N == 0) return 0;
  if (!x || !g_out || !rowptr || (num_ntypes > 0 && !ntypes)) return CGVP_ERR_BAD_ARG;
  if (E > 0 && (!eperm || !esrc || !edst || (edge_dim > 0 && !eattr) || (num_etypes > 0 && !etypes))) return CGVP_ERR_BAD_ARG;
  if (misaligned16({g_out, mask})) return CGVP_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (g_x) quad::zero_words(g_x, (size_t)N * (cin - num_ntypes), st);
  int rows = 0, row_len = 0;
  if (int rc = quad::gine_bwd(cin, chid, cout, num_ntypes, num_etypes, edge_dim, x, ntypes, eattr, etypes, rowptr, eperm,
                              esrc, edst, N, w, act_slope, mask, rng_args(rng), g_out, g_x, workspace, max_workgroups, &rows, &row_len, st)) return rc;
  quad::reduce_slab(workspace, rows, row_len, 0, row_len, grad_layer, st);
  return launch_status();
}

}  // extern "C"
