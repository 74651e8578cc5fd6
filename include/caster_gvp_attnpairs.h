/*
 * caster_gvp_attnpairs.h -- the varlen cross attention over a LIST OF PAIRS of unique graphs, forward only.
 *
 * cgvp_attn_fwd ties pair b to rows ptr[b] .. ptr[b+1] of q, k, v and out alike: to score one protein against 1,024
 * drugs its caller collates (and encodes, norms, projects) the same protein 1,024 times.  Nothing before
 * softmax(Q K^T) V depends on the partner.  The entry points below read the projected rows of every UNIQUE graph once
 * and take the pairing as two index tables: pair b uses query graph q_graph[b] and key graph k_graph[b], and owns rows
 * out_ptr[b] .. out_ptr[b+1] of the output.  Inference only: no dropout, no backward, no weights.
 *
 * A header of its own beside caster_gvp.h, as caster_gvp_attnscore.h and caster_gvp_attnhd.h are: the entry points
 * live in the same libcaster_gvp.so, follow the same conventions (caller-owned DEVICE pointers, nothing allocated or
 * retained, an explicit hipStream_t, asynchronous launches, 0 = launched / >0 = hipError_t / <0 = CGVP_ERR_* from
 * caster_gvp.h, re-entrant, no state), and carry a version of their own, so the main C ABI does not move.
 */
#ifndef CASTER_GVP_ATTNPAIRS_H
#define CASTER_GVP_ATTNPAIRS_H

#include <stdint.h>

#include "caster_gvp.h" /* CGVP_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_ATTN_PAIRS_VERSION 1

int cgvp_attn_pairs_version(void);

/* One direction of the cross attention over a pair list.  E = heads * head_dim. */
typedef struct {
  const float* q;           /* [num_q][E] query rows of the UNIQUE query graphs, 16-byte aligned                   */
  const float* k;           /* [num_k][E] key rows of the UNIQUE key graphs, 16-byte aligned                       */
  const float* v;           /* [num_k][E] value rows, 16-byte aligned                                              */
  const int64_t* q_ptr;     /* [num_q_graphs + 1] ascending row offsets, q_ptr[num_q_graphs] <= num_q              */
  const int64_t* k_ptr;     /* [num_k_graphs + 1] ascending row offsets, k_ptr[num_k_graphs] <= num_k              */
  int64_t num_q_graphs, num_k_graphs, num_q, num_k;
  const int64_t* q_graph;   /* [num_pairs] in 0 .. num_q_graphs - 1: the query graph of pair b                     */
  const int64_t* k_graph;   /* [num_pairs] in 0 .. num_k_graphs - 1: the key graph of pair b                       */
  const int64_t* out_ptr;   /* [num_pairs + 1] ascending offsets of the pairs' rows in out:
                               out_ptr[b+1] - out_ptr[b] == q_ptr[q_graph[b]+1] - q_ptr[q_graph[b]]                */
  int64_t num_out;          /* rows of out; out_ptr[num_pairs] <= num_out                                          */
  float* out;               /* [num_out][E], 16-byte aligned                                                       */
  float* lse;               /* [num_out][heads] log sum_k exp(scale q.k) per output row and head, or NULL          */
} cgvp_attn_pairs_problem;

/* For every pair b, head h and row r of the pair's query graph, with qg = q_graph[b], kg = k_graph[b] and the keys /
 * values rows k_ptr[kg] .. k_ptr[kg+1]:
 *
 *   out[out_ptr[b] + r] = softmax_k(scale * q[q_ptr[qg] + r] . k[.]) v[.]
 *
 * The arithmetic of a pair is that of cgvp_attn_fwd_hd without dropout (caster_gvp_attnhd.h), instruction for
 * instruction: the same rows give the same bits wherever they lie.  No atomics.  A pair without keys gets zero rows and
 * an lse of -inf; a pair without queries writes nothing.  Up to two problems (the two directions of the module) go in
 * one launch when they share heads and head_dim; directions of different widths take one call each.
 *
 * The index tables are DEVICE memory: the entry point cannot look at them.  The caller guarantees what the struct's
 * comments say (the Python layer checks them on the host before it launches).
 *
 * head_dim must be 16, 32 or 64: anything else returns CGVP_ERR_UNSUPPORTED_DIMS before every other check.
 * CGVP_ERR_BAD_ARG, before anything is launched (and before the num_pairs == 0 return, which launches nothing and
 * returns 0): problems NULL, num_problems outside 1..2, num_pairs < 0 or >= 2^30, heads < 1, a negative graph or row
 * count, (rows + 16) * heads * head_dim >= 2^31 for num_q, num_k or num_out (rows are addressed with 32-bit element
 * offsets), a NULL q_ptr / k_ptr / q_graph / k_graph / out_ptr, q NULL with num_q > 0, k or v NULL with num_k > 0,
 * out NULL with num_out > 0, a row array that is not 16-byte aligned, an index table that is not 8-byte aligned, an
 * lse that is not 4-byte aligned. */
int cgvp_attn_fwd_pairs(const cgvp_attn_pairs_problem* problems, int32_t num_problems /* 1 or 2 */, int64_t num_pairs,
                        int32_t heads, int32_t head_dim /* 16, 32, 64 */, float scale, void* stream);

/* out[out_ptr[b] + r] = src[src_ptr[graph[b]] + r] for every pair b and row r < out_ptr[b+1] - out_ptr[b] (the length of
 * graph[b]): the per-pair copy of the unique graphs' rows, what the residual stream of the first cross-attention layer
 * starts from.  batch_out, when given, receives the pair of every row: batch_out[out_ptr[b] + r] = b (the `batch`
 * vector of the expanded rows).  Rows of `width` floats, moved as float4.  A pair of length 0 contributes nothing; rows
 * of out behind out_ptr[num_pairs] are not written.
 *
 * CGVP_ERR_BAD_ARG, before anything is launched (and before the num_pairs == 0 return): num_pairs < 0 or >= 2^30,
 * num_out < 0 or >= 2^33, width < 4 or no multiple of 4, a NULL src_ptr / graph / out_ptr, src or out NULL with
 * num_out > 0, src or out not 16-byte aligned, a table or batch_out not 8-byte aligned. */
int cgvp_expand_rows(const float* src, const int64_t* src_ptr, const int64_t* graph, const int64_t* out_ptr,
                     int64_t num_pairs, int64_t num_out, int32_t width /* multiple of 4 */, float* out,
                     int64_t* batch_out /* [num_out] = pair of the row, or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_ATTNPAIRS_H */
