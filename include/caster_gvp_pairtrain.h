/*
 * caster_gvp_pairtrain.h -- TRAINING on a list of pairs of unique graphs: the backward of cgvp_attn_fwd_pairs and of
 * cgvp_expand_rows (caster_gvp_attnpairs.h).
 *
 * A batch of 8 proteins x 8 drugs = 64 pairs holds 8 protein graphs: with the forward of caster_gvp_attnpairs.h every
 * unique graph is encoded, normed and projected once, and the gradient of a unique row is the sum over all the pairs
 * that reference its graph.  That sum is an ORDERED one here, never a scatter of float atomics: the attention backward
 * writes per-pair partial gradients with plain stores, and cgvp_reduce_rows adds, for every unique graph, the partial
 * rows of its pairs in ascending pair order, through an inverse table of the pair list.  The summation order is a
 * function of the tables alone: two runs give bitwise equal gradients, in every mode (there is no deterministic
 * switch because there is no other form).
 *
 * A header and a version of its own (CGVP_ATTN_PAIRS_VERSION and the symbols of caster_gvp_attnpairs.h do not move).
 * Same library, same conventions: caller-owned DEVICE pointers, nothing allocated or retained (the workspace is the
 * caller's, sized by a query function), an explicit hipStream_t, asynchronous launches, 0 = launched / >0 =
 * hipError_t / <0 = CGVP_ERR_* from caster_gvp.h, re-entrant, no state.
 */
#ifndef CASTER_GVP_PAIRTRAIN_H
#define CASTER_GVP_PAIRTRAIN_H

#include <stdint.h>

#include "caster_gvp.h" /* CGVP_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_PAIR_TRAIN_VERSION 1

int cgvp_pair_train_version(void);

/* One direction of the cross attention over a pair list, for its backward.  E = heads * head_dim.  The first block of
 * fields is the forward's problem (cgvp_attn_pairs_problem) with `out` and `lse` as the forward wrote them. */
typedef struct {
  const float* q;             /* [num_q][E] query rows of the UNIQUE query graphs, 16-byte aligned                 */
  const float* k;             /* [num_k][E] key rows of the UNIQUE key graphs, 16-byte aligned                     */
  const float* v;             /* [num_k][E] value rows, 16-byte aligned                                            */
  const int64_t* q_ptr;       /* [num_q_graphs + 1] ascending row offsets, q_ptr[num_q_graphs] <= num_q            */
  const int64_t* k_ptr;       /* [num_k_graphs + 1] ascending row offsets, k_ptr[num_k_graphs] <= num_k            */
  int64_t num_q_graphs, num_k_graphs, num_q, num_k;
  const int64_t* q_graph;     /* [num_pairs] in 0 .. num_q_graphs - 1                                              */
  const int64_t* k_graph;     /* [num_pairs] in 0 .. num_k_graphs - 1                                              */
  const int64_t* out_ptr;     /* [num_pairs + 1] offsets of the pairs' QUERY rows in out / lse / g_out             */
  int64_t num_out;            /* rows of out, lse and g_out; out_ptr[num_pairs] <= num_out                         */
  const float* out;           /* [num_out][E] the forward's output, 16-byte aligned                                */
  const float* lse;           /* [num_out][heads] the forward's log-sum-exp                                        */
  const float* g_out;         /* [num_out][E] gradient of out, 16-byte aligned                                     */
  const int64_t* kout_ptr;    /* [num_pairs + 1] offsets of the pairs' KEY rows in the per-pair partials:
                                 kout_ptr[b+1] - kout_ptr[b] == k_ptr[k_graph[b]+1] - k_ptr[k_graph[b]]
                                 (the out_ptr of the other direction)                                              */
  int64_t num_kout;           /* kout_ptr[num_pairs] <= num_kout                                                   */
  const int64_t* q_inv_ptr;   /* [num_q_graphs + 1] inverse of q_graph: the pairs of query graph g are             */
  const int64_t* q_inv_pairs; /* [num_pairs]        q_inv_pairs[q_inv_ptr[g] .. q_inv_ptr[g+1]-1], ascending       */
  const int64_t* k_inv_ptr;   /* [num_k_graphs + 1] the same for k_graph                                           */
  const int64_t* k_inv_pairs; /* [num_pairs]                                                                       */
  float* g_q;                 /* [num_q][E] gradient of q, 16-byte aligned                                         */
  float* g_k;                 /* [num_k][E] gradient of k                                                          */
  float* g_v;                 /* [num_k][E] gradient of v                                                          */
} cgvp_attn_pairs_bwd_problem;

/* Floats of workspace cgvp_attn_bwd_pairs needs for these problems (the per-pair partial gradients d Q [num_out][E],
 * d K and d V [num_kout][E] and delta [num_out][heads] of every problem; a multiple of 4), or a negative CGVP_ERR_*:
 * CGVP_ERR_UNSUPPORTED_DIMS for a head_dim outside 16 / 32 / 64, CGVP_ERR_BAD_ARG for problems NULL, num_problems
 * outside 1..2, heads < 1 or a negative num_out / num_kout.  Only the counts are read. */
int64_t cgvp_attn_bwd_pairs_floats(const cgvp_attn_pairs_bwd_problem* problems, int32_t num_problems, int32_t heads,
                                   int32_t head_dim);

/* The backward of cgvp_attn_fwd_pairs: g_q, g_k, g_v of the UNIQUE rows from the per-pair g_out.
 *
 * Three stages on `stream`, no atomics: (1) one wave per 16-row tile of a pair's query rows and head recomputes
 * P = exp(scale q.k - lse) and writes delta = sum_d g_out . out and the pair's d Q at its out_ptr rows of the
 * workspace; (2) one wave per 16-key tile of a pair's key rows (kout_ptr) and head loops over the pair's queries and
 * writes the pair's d K and d V; (3) cgvp_reduce_rows's kernel, one launch for all gradients of the call, adds for
 * every unique graph the partial rows of the pairs that reference it, in ascending pair order.  The arithmetic of (1)
 * and (2) is that of cgvp_attn_bwd_hd without dropout on the pair's rows.
 *
 * A pair without keys (lse = -inf, zero output rows) contributes exactly zero to every gradient, never a NaN.  A
 * unique graph that no pair references gets zero rows, written here: the caller does not pre-zero.  A unique graph
 * without rows is legal on either side.  With num_pairs == 0 stage (3) alone runs and every graph's rows become zero
 * (without a graph or a row on any side nothing is launched and the call returns 0 once its arguments have passed).
 * Rows of g_q / g_k / g_v behind q_ptr[num_q_graphs] / k_ptr[num_k_graphs] belong to no graph and are not written.
 *
 * The tables are DEVICE memory the entry point cannot look at: the caller guarantees what the struct's comments say.
 *
 * head_dim must be 16, 32 or 64: anything else returns CGVP_ERR_UNSUPPORTED_DIMS before every other check.
 * CGVP_ERR_BAD_ARG, before anything is launched: problems NULL, num_problems outside 1..2, num_pairs < 0 or >= 2^30,
 * heads < 1, a negative graph or row count, (rows + 16) * heads * head_dim >= 2^31 for num_q, num_k, num_out or
 * num_kout (rows are addressed with 32-bit element offsets), a NULL table, q or g_q NULL with num_q > 0, k, v, g_k or
 * g_v NULL with num_k > 0, out, lse or g_out NULL with num_out > 0, a row array that is not 16-byte aligned, a table
 * that is not 8-byte aligned, an lse that is not 4-byte aligned, a workspace that is NULL (with a non-zero need), not
 * 16-byte aligned or smaller than cgvp_attn_bwd_pairs_floats says. */
int cgvp_attn_bwd_pairs(const cgvp_attn_pairs_bwd_problem* problems, int32_t num_problems /* 1 or 2 */,
                        int64_t num_pairs, int32_t heads, int32_t head_dim /* 16, 32, 64 */, float scale,
                        float* workspace, int64_t workspace_floats, void* stream);

/* The transpose of cgvp_expand_rows: for every unique graph g and row r < src_ptr[g+1] - src_ptr[g]
 *
 *   dst[src_ptr[g] + r] = sum over j = inv_ptr[g] .. inv_ptr[g+1]-1, in increasing j, of part[optr[inv_pairs[j]] + r]
 *
 * (inv_pairs[inv_ptr[g] ..] lists the pairs b with graph[b] == g; optr is the out_ptr of the expansion).  Rows of
 * `width` floats, read as float4; every output row has one owner (one wave per 16-row tile of a graph), no atomics.
 * A graph that no pair references gets zero rows.  Rows of dst behind src_ptr[num_graphs] are not written.
 *
 * CGVP_ERR_BAD_ARG, before anything is launched (and before the num_graphs == 0 return): num_graphs < 0 or >= 2^30,
 * num_pairs < 0 or >= 2^30, num_part or num_dst < 0 or >= 2^33, width < 4 or no multiple of 4, a NULL optr / inv_ptr /
 * inv_pairs / src_ptr, part NULL with num_part > 0, dst NULL with num_dst > 0, part or dst not 16-byte aligned, a
 * table not 8-byte aligned. */
int cgvp_reduce_rows(const float* part, const int64_t* optr, const int64_t* inv_ptr, const int64_t* inv_pairs,
                     const int64_t* src_ptr, int64_t num_graphs, int64_t num_pairs, int64_t num_part, int64_t num_dst,
                     int32_t width /* multiple of 4 */, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_PAIRTRAIN_H */
