// Internal declarations shared by the translation units of libcaster_gvp.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gvp_host.h"
#include "gvp_math.h"
#include "gvp_rng.h"

// Tile policy index the launchers in namespace quad take: activation storage type x layer kind (cgvp_dims.storage /
// cgvp_dims.layer_kind; gvp_quad.h LayerKind).  bf16 storage exists for CASTER-DTA's layers only.
constexpr int POLICY_F32 = 0, POLICY_BF16 = 1, POLICY_GVPDEF = 2, POLICY_LINEAR = 3;

// Small host helpers of the entry points.
inline int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline int num_convs_of(const cgvp_layout& l) { return l.conv_stride > 0 ? (l.ln_out - l.conv0) / l.conv_stride : 0; }
// floats of a GINE layer's parameters / gradient block, state_dict order:
// eps | nn.lins.0.weight | nn.lins.0.bias | nn.lins.1.weight | nn.lins.1.bias | lin.weight | lin.bias
constexpr int gine_layer_floats(int cin, int chid, int cout, int ke) {
  return 1 + chid * cin + chid + cout * chid + cout + cin * ke + cin;
}

// Float offsets of the per-kernel slices inside the fragment image.
struct QuadOffsets {
  int emb, conv0, node0, layer_stride, head, total;
  int embT, convT0, nodeT0, layerT_stride, headT;     // transposed slices (backward)
};

#ifndef CGVP_BWD_MAX_GRID
#define CGVP_BWD_MAX_GRID 240       // of 256 CUs: the rest is left to the drug-side backward running beside it
#endif
constexpr int kBwdMaxGrid = CGVP_BWD_MAX_GRID;    // persistent workgroups of the backward kernels (one per CU) = slab rows per stage

#include <type_traits>

// Runtime value -> compile-time tag of a generic lambda, so that every combination of kernel template flags is written once.
// with_policy: `f(Tag<ST>{})` for the storage tag type ST of a tile policy index; KINDS says whether the two layer-kind
// policies exist for the kernel (they are not instantiated otherwise).  with_flag: `f(std::bool_constant<b>{})`.
namespace gq { struct bf16s; struct f32_gvpdef; struct f32_linear; }
template <class T> struct Tag { using type = T; };
template <class ST> constexpr bool is_layer_kind = std::is_same_v<ST, gq::f32_gvpdef> || std::is_same_v<ST, gq::f32_linear>;
template <bool KINDS, class F>
int with_policy(int policy, F&& f) {
  if (policy == POLICY_F32) return f(Tag<float>{});
  if (policy == POLICY_BF16) return f(Tag<gq::bf16s>{});
  if constexpr (KINDS) {
    if (policy == POLICY_GVPDEF) return f(Tag<gq::f32_gvpdef>{});
    if (policy == POLICY_LINEAR) return f(Tag<gq::f32_linear>{});
  }
  return CGVP_ERR_UNSUPPORTED_DIMS;
}
template <class F>
int with_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

namespace quad {
int offsets(int nt_node, int nt_edge, int num_convs, QuadOffsets* o);
int prepare(const gvp::EncLayout& L, int num_convs, int packed_bf16, const float* params, float* image, hipStream_t st);
int node_embed(int nt_node, const float* img, const float* x_s, const float* x_v, const int64_t* ntypes,
               int64_t N, float* h, unsigned long long* rng_state, unsigned long long* rng_out, int policy, hipStream_t st);
int pass_begin(const gvp::EncLayout& L, int num_convs, int policy, const float* params, float* image, const float* x_s,
               const float* x_v, const int64_t* ntypes, int64_t N, float* h, unsigned long long* rng_state,
               unsigned long long* rng_out, const int64_t* edge_index, int64_t E, int32_t* counters, hipStream_t st);
int conv(int nt_edge, const float* img, const float* h, const float* e_s, const float* e_v,
         const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm, const int32_t* esrc,
         const int32_t* edst, int64_t N, int64_t E, int mean, float* dh, int fuse, const float* img_node,
         const float* img_head, float* h_out, float* out, const float* mask0, const float* mask1, gvp::RngArgs rng,
         const float* e_in, float* e_out, int policy, hipStream_t st);
int node_update(const float* img_node, const float* img_head, const float* h, const float* dh, int64_t N,
                int with_head, float* h_out, float* out, const float* mask0, const float* mask1, gvp::RngArgs rng,
                int policy, hipStream_t st);

// ---- backward (gvp_quad_bwd_kernels.hip).  Weight gradients are written as one
// partial block per workgroup into `slab` ([grid][block floats]); `grid` returns
// the number of rows to reduce.
int node_update_bwd(const float* img_node, const float* imgT_node, const float* h, const float* dh,
                    const float* mask0, const float* mask1, gvp::RngArgs rng, const float* g_up0, const float* g_up1,
                    const float* g_up2, int64_t N, float* g_dh, float* g_h, float* zero_rows, float* slab, int* grid,
                    int policy, hipStream_t st);
int head_bwd(const float* img_head, const float* imgT_head, const float* h_out, const float* g_out, int64_t N,
             float* g_h_out, float* slab, int* grid, int policy, hipStream_t st);
// head_bwd + node_update_bwd of the last layer as ONE launch (g_h_out doubles as the node stage's upstream gradient)
int node_head_bwd(const float* img_head, const float* imgT_head, const float* h_out, const float* g_out, float* g_h_out,
                  float* head_slab, const float* img_node, const float* imgT_node, const float* h, const float* dh,
                  const float* mask0, const float* mask1, gvp::RngArgs rng, int64_t N, float* g_dh, float* g_h,
                  float* zero_rows, float* slab, int* grid, int policy, hipStream_t st);
int conv_bwd(int nt_edge, const float* img, const float* imgT, const float* h, const float* e_emb,
             const int32_t* rowptr, const int32_t* esrc, const int32_t* edst, int64_t N, int64_t E, int mean,
             const float* g_dh, float* g_src, float* g_dst, float* g_e, float* slab, int* grid, int policy, hipStream_t st,
             float* g_edge = nullptr, float* slot = nullptr);
// ---- deterministic mode (CGVP_BWD_DETERMINISTIC): store-then-sum instead of float atomics
// conv_bwd with g_edge / slot: d h[src] rows -> g_edge [E][28] at their sorted positions, boundary rows -> slot
// [conv_bwd_max_waves()][28]; g_src is not touched (src_sum fills it).  The waves of the launch are *grid x 8.
int conv_bwd_max_waves();
// out [N][width] = self (optional) + rows[p] over the source's positions (+ slot rows of conv_bwd's boundary targets)
int src_sum(int width, const float* rows, const float* self, const int32_t* sptr, const int32_t* spos,
            const int32_t* rowptr, const float* slot, int64_t waves, int64_t N, float* out, hipStream_t st);
struct DetBufs { const int32_t* sptr; const int32_t* spos; float* rows; float* slot; };
int conv_bwd_entry(const cgvp_dims* dims, const cgvp_layout* layout, const float* image, int32_t layer,
                   const float* h, const float* e_emb, const int32_t* rowptr, const int32_t* esrc,
                   const int32_t* edst, int64_t N, int64_t E, int32_t aggr_mean, const float* g_dh, float* g_src,
                   int32_t g_src_zeroed, float* g_dst, float* g_e, float* grad_params, float* workspace,
                   cgvp_segment* segs, int32_t* nsegs, void* stream, const DetBufs* det);
// CGVP_DETERMINISTIC=1 in the environment (read once): every backward runs in the deterministic mode
bool deterministic_env();
// backward of gvp_edge + LayerNorm from the summed d(edge embedding) of the conv layers (weight gradients only)
int edge_embed_bwd(int nt_edge, const float* img, const float* imgT, const float* e_s, const float* e_v,
                   const int64_t* etypes, const int32_t* eperm, int64_t E, const float* const* g_e, int n_g,
                   float* g_e_s, float* g_e_v, float* slab, int* grid, int policy, hipStream_t st);
constexpr int kEdgeRow = 36;              // floats per edge of the stored edge embedding: [e_s 32 | e_v 3 | pad]
int node_embed_bwd(int nt_node, const float* img, const float* imgT, const float* x_s, const float* x_v,
                   const int64_t* ntypes, int64_t N, const float* g_up0, const float* g_up1, const float* g_up2,
                   float* g_x_s, float* g_x_v, float* slab, int* grid, int policy, hipStream_t st);
// GINE layer backward on 16-atom MFMA tiles (gine_quad_kernels.hip): one slab row per workgroup
// (`rows` x `row_len` floats, state_dict order of the layer).
constexpr int kGineBwdMaxGrid = 256;      // upper bound (workspace sizing)
constexpr int kGineBwdDefaultGrid = 16;   // the CUs the protein backward (kBwdMaxGrid workgroups, one per CU) leaves free
int gine_bwd(int cin, int chid, int cout, int nt, int net, int ed, const float* x, const int64_t* ntypes,
             const float* eattr, const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm,
             const int32_t* esrc, const int32_t* edst, int64_t N, const cgvp_gine_w* w, float slope,
             const float* mask, gvp::RngArgs rng, const float* g_out, float* g_x, float* slab, int max_workgroups, int* rows,
             int* row_len, hipStream_t st, const float* agg_in = nullptr, const uint16_t* pos_in = nullptr,
             float* g_edge = nullptr, float* g_self = nullptr,
             // d eattr [E][ed] at the original edge ids, or NULL; eattr_accum: 0 = store the rows, 1 = add to them
             float* g_eattr = nullptr, int eattr_accum = 0);
int gine_fwd(int cin, int chid, int cout, int nt, int net, int ed, const float* x, const int64_t* ntypes,
             const float* eattr, const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm,
             const int32_t* esrc, const int32_t* edst, int64_t N, const cgvp_gine_w* w, float slope,
             const float* mask, gvp::RngArgs rng, float* out, float* agg_out, uint16_t* pos_out, hipStream_t st);
// the same two over the shapes of gine_quad_wide_kernels.hip / gine_quad_wide64_kernels.hip (what gine_bwd / gine_fwd try
// after their own table; same returns)
int gine_bwd_wide(int cin, int chid, int cout, int nt, int net, int ed, const float* x, const int64_t* ntypes,
                  const float* eattr, const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm,
                  const int32_t* esrc, const int32_t* edst, int64_t N, const cgvp_gine_w* w, float slope,
                  const float* mask, gvp::RngArgs rng, const float* g_out, float* g_x, float* slab, int max_workgroups,
                  int* rows, int* row_len, hipStream_t st, const float* agg_in, const uint16_t* pos_in, float* g_edge,
                  float* g_self, float* g_eattr, int eattr_accum);
int gine_fwd_wide(int cin, int chid, int cout, int nt, int net, int ed, const float* x, const int64_t* ntypes,
                  const float* eattr, const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm,
                  const int32_t* esrc, const int32_t* edst, int64_t N, const cgvp_gine_w* w, float slope,
                  const float* mask, gvp::RngArgs rng, float* out, float* agg_out, uint16_t* pos_out, hipStream_t st);
int gine_bwd_wide64(int cin, int chid, int cout, int nt, int net, int ed, const float* x, const int64_t* ntypes,
                  const float* eattr, const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm,
                  const int32_t* esrc, const int32_t* edst, int64_t N, const cgvp_gine_w* w, float slope,
                  const float* mask, gvp::RngArgs rng, const float* g_out, float* g_x, float* slab, int max_workgroups,
                  int* rows, int* row_len, hipStream_t st, const float* agg_in, const uint16_t* pos_in, float* g_edge,
                  float* g_self, float* g_eattr, int eattr_accum);
int gine_fwd_wide64(int cin, int chid, int cout, int nt, int net, int ed, const float* x, const int64_t* ntypes,
                  const float* eattr, const int64_t* etypes, const int32_t* rowptr, const int32_t* eperm,
                  const int32_t* esrc, const int32_t* edst, int64_t N, const cgvp_gine_w* w, float slope,
                  const float* mask, gvp::RngArgs rng, float* out, float* agg_out, uint16_t* pos_out, hipStream_t st);
bool gine_shape_compiled(int cin, int chid, int cout, int nt, int net, int ed);   // the tile kernels exist for the layer
int gine_max_slab_row();                  // floats of the largest compiled layer's gradient block
int reduce_slab(const float* slab, int rows, int stride, int col0, int len, float* dst, hipStream_t st);
int reduce_segments(const cgvp_segment* segs, int nsegs, float* grad_params, hipStream_t st, int overwrite = 0,
                    bool store_only = false);
// floats of one slab row (= one workgroup's weight-gradient block) of each backward stage
struct BwdBlocks { int emb, conv_edge, conv_total, node, head; };
int bwd_block_sizes(int nt_node, int nt_edge, BwdBlocks* b);
// ---- graph_index_kernels.hip: zero fill, dst-sorted CSR build, source-order index
void zero_words(void* p, size_t words, hipStream_t s);     // the library's own zero fill (never hipMemsetAsync: see that file)
int csr_build(const int64_t* edge_index, int64_t N, int64_t E, int32_t* rowptr, int32_t* eperm, int32_t* esrc,
              int32_t* edst, int32_t* work, int work_is_zero, int32_t* ids_scratch, unsigned long long* rng_state,
              unsigned long long* rng_out, hipStream_t stream);
// source-order index of a dst-sorted CSR: sptr [N+1], spos [E]: the sorted positions p < rowptr[N] of every source in
// increasing p.  work: src_index_work_ints(N, E) ints, 16-B aligned, any content.  Five launches.
int64_t src_index_work_ints(int64_t N, int64_t E);
int src_index(const int32_t* rowptr, const int32_t* esrc, int64_t N, int64_t E, int32_t* sptr, int32_t* spos,
              int32_t* work, hipStream_t st);
// ---- gvp_kernels.hip: cgvp_rng_next without its checks (csr_build's, when it has no count launch to advance the generator in)
int rng_next(unsigned long long* state, unsigned long long* out, hipStream_t st);
}  // namespace quad
