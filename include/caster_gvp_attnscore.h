/*
 * caster_gvp_attnscore.h -- per-node attention scores of the varlen cross attention: what the reference's evaluation
 * keeps of the attention weights (inference/evaluation.py:54-66, 97-102: the head-averaged weight matrix of every
 * pair, cut to [:dlen, :plen] and [:plen, :dlen], then the column MEAN and the column MAX of each), computed straight
 * from the compact rows the attention kernels work on.  No dense [B, Lq_max, Lk_max] tensor is written, no length
 * maximum is needed, nothing is read back: the call can sit inside a captured step.
 *
 * A header of its own beside caster_gvp.h, as caster_gvp_metrics.h is: the entry points below live in the same
 * libcaster_gvp.so, follow the same conventions (caller-owned DEVICE pointers, nothing allocated or retained, an
 * explicit hipStream_t, asynchronous launches, 0 = launched / >0 = hipError_t / <0 = CGVP_ERR_* from caster_gvp.h,
 * re-entrant, no state), and carry a version of their own, so the main C ABI does not move when this one grows.
 */
#ifndef CASTER_GVP_ATTNSCORE_H
#define CASTER_GVP_ATTNSCORE_H

#include <stdint.h>

#include "caster_gvp.h" /* CGVP_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_ATTN_SCORE_VERSION 1
/* Most heads the kernel is compiled for (head_dim is 16, as for cgvp_attn_fwd: embed = 16 * heads). */
#define CGVP_ATTN_SCORE_MAX_HEADS 8

int cgvp_attn_score_version(void);

/* One direction of the cross attention, on the operands cgvp_attn_fwd took and the log-sum-exp it saved:
 * pair b's queries are rows q_ptr[b] .. q_ptr[b+1] of q, its keys rows k_ptr[b] .. k_ptr[b+1] of k. */
typedef struct {
  const float* q;          /* [num_q][16 * heads], 16-byte aligned                                             */
  const float* k;          /* [num_k][16 * heads], 16-byte aligned                                             */
  const float* lse;        /* [num_q][heads]: log sum_k exp(scale q.k) per query and head (cgvp_attn_fwd);
                              16-byte aligned when heads is a multiple of 4, else 4-byte                       */
  const int64_t* q_ptr;    /* [num_pairs + 1], ascending, q_ptr[num_pairs] <= num_q                            */
  const int64_t* k_ptr;    /* [num_pairs + 1], ascending, k_ptr[num_pairs] <= num_k                            */
  int64_t num_q, num_k;
  float* out_mean;         /* [num_k] fp32, 4-byte aligned                                                     */
  float* out_max;          /* [num_k] fp32, 4-byte aligned                                                     */
} cgvp_attn_score_problem;

/* For every key row k of every pair b, with nq_b = q_ptr[b+1] - q_ptr[b] and q over the pair's queries:
 *
 *   w[q][k]     = (1 / heads) * sum_h exp(scale * Q_h[q] . K_h[k] - lse[q][h])      nn.MultiheadAttention's
 *                                                                                   head-averaged weight
 *   out_mean[k] = (1 / nq_b) * sum_q w[q][k]
 *   out_max[k]  = max_q w[q][k]            (the head average first, then the maximum: not a maximum over heads)
 *
 * in fp32, compact: element k of the outputs belongs to row k of `k`.  One launch for up to two problems (the two
 * directions of the module).  One workgroup owns 16 keys of one pair for all heads, its waves split the pair's
 * queries and their partial sums and maxima are combined in a fixed order: no atomics, two calls on the same values
 * agree bitwise.
 *
 * Edges: a key whose pair has NO queries gets out_mean = out_max = 0 (the reference cannot produce such a pair: it
 * would take the mean of an empty column).  A pair without keys writes nothing.  Rows of `k` that no pair covers
 * (behind k_ptr[num_pairs]) are not written.  Nothing is read outside the ptr-delimited rows, nothing is written
 * outside [0, num_k) of the outputs, and the call never uses hipMemset.  num_pairs == 0 launches nothing.
 *
 * CGVP_ERR_BAD_ARG, before anything is launched (and before the num_pairs == 0 return): problems NULL, num_problems
 * outside 1..2, num_pairs < 0 or >= 2^30, heads < 1, a negative row count, (rows + 16) * 16 * heads >= 2^31 (rows are
 * addressed with 32-bit element offsets), a NULL q_ptr / k_ptr, q or lse NULL with num_q > 0, k or an output NULL with
 * num_k > 0 (an empty side needs no buffers), a misaligned pointer.  CGVP_ERR_UNSUPPORTED_DIMS: heads above
 * CGVP_ATTN_SCORE_MAX_HEADS. */
int cgvp_attn_node_scores(const cgvp_attn_score_problem* problems, int32_t num_problems, int64_t num_pairs,
                          int32_t heads, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_ATTNSCORE_H */
