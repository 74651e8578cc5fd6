/*
 * caster_gvp_pairscore.h -- per-node attention scores of the varlen cross attention over a LIST OF PAIRS of unique
 * graphs: what cgvp_attn_node_scores_hd (caster_gvp_attnscore.h, caster_gvp_attnhd.h) computes for a collated batch,
 * on the operands of cgvp_attn_fwd_pairs (caster_gvp_attnpairs.h).  The query and key rows of every UNIQUE graph are
 * read where they lie; the pairing is two index tables; only the log-sum-exp and the two outputs are per pair.  No
 * per-pair copy of the rows, no dense [B, Lq_max, Lk_max] tensor, nothing read back: the call can sit inside a
 * captured graph.  Inference only.
 *
 * A header of its own beside caster_gvp.h, as caster_gvp_attnpairs.h is: the entry points live in the same
 * libcaster_gvp.so, follow the same conventions (caller-owned DEVICE pointers, nothing allocated or retained, an
 * explicit hipStream_t, asynchronous launches, 0 = launched / >0 = hipError_t / <0 = CGVP_ERR_* from caster_gvp.h,
 * re-entrant, no state), and carry a version of their own, so the main C ABI does not move.
 */
#ifndef CASTER_GVP_PAIRSCORE_H
#define CASTER_GVP_PAIRSCORE_H

#include <stdint.h>

#include "caster_gvp.h" /* CGVP_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_PAIR_SCORE_VERSION 1

int cgvp_pair_score_version(void);

/* One direction of the cross attention over a pair list.  E = heads * head_dim. */
typedef struct {
  const float* q;            /* [num_q][E] query rows of the UNIQUE query graphs, 16-byte aligned                   */
  const float* k;            /* [num_k][E] key rows of the UNIQUE key graphs, 16-byte aligned                       */
  const float* lse;          /* [num_qout][heads] log sum_k exp(scale q.k) per PAIR row and head, as
                                cgvp_attn_fwd_pairs wrote it for this direction (its `lse` at its `out_ptr`);
                                16-byte aligned when heads is a multiple of 4, else 4-byte                          */
  const int64_t* q_ptr;      /* [num_q_graphs + 1] ascending row offsets, q_ptr[num_q_graphs] <= num_q              */
  const int64_t* k_ptr;      /* [num_k_graphs + 1] ascending row offsets, k_ptr[num_k_graphs] <= num_k              */
  int64_t num_q_graphs, num_k_graphs, num_q, num_k;
  const int64_t* q_graph;    /* [num_pairs] in 0 .. num_q_graphs - 1: the query graph of pair b                     */
  const int64_t* k_graph;    /* [num_pairs] in 0 .. num_k_graphs - 1: the key graph of pair b                       */
  const int64_t* qout_ptr;   /* [num_pairs + 1] ascending offsets of the pairs' QUERY rows in lse:
                                qout_ptr[b+1] - qout_ptr[b] == q_ptr[q_graph[b]+1] - q_ptr[q_graph[b]]              */
  int64_t num_qout;          /* rows of lse; qout_ptr[num_pairs] <= num_qout                                        */
  const int64_t* kout_ptr;   /* [num_pairs + 1] ascending offsets of the pairs' KEY rows in the outputs:
                                kout_ptr[b+1] - kout_ptr[b] == k_ptr[k_graph[b]+1] - k_ptr[k_graph[b]]              */
  int64_t num_kout;          /* entries of the outputs; kout_ptr[num_pairs] <= num_kout                             */
  float* out_mean;           /* [num_kout] fp32, 4-byte aligned                                                     */
  float* out_max;            /* [num_kout] fp32, 4-byte aligned                                                     */
} cgvp_attn_pairs_score_problem;

/* For every pair b and key row j of its key graph, with qg = q_graph[b], kg = k_graph[b], r over the rows of the query
 * graph and nq = q_ptr[qg+1] - q_ptr[qg]:
 *
 *   w[r][j]                    = (1 / heads) * sum_h exp(scale * Q_h[q_ptr[qg] + r] . K_h[k_ptr[kg] + j]
 *                                                        - lse[qout_ptr[b] + r][h])
 *   out_mean[kout_ptr[b] + j]  = (1 / nq) * sum_r w[r][j]
 *   out_max [kout_ptr[b] + j]  = max_r w[r][j]           (the head average first, then the maximum)
 *
 * in fp32.  The arithmetic of a pair is that of cgvp_attn_node_scores_hd, instruction for instruction: the same rows
 * give the same bits wherever they lie.  One workgroup owns 16 keys of one pair for all heads, its waves split the
 * pair's queries and their partial sums and maxima are combined in a fixed order: no atomics, two calls on the same
 * values agree bitwise.  Up to two problems (the two directions of the module) go in one launch when they share heads
 * and head_dim; directions of different widths take one call each.
 *
 * Edges: a key whose pair has NO queries gets out_mean = out_max = 0.  A pair without keys writes nothing.  Entries of
 * the outputs behind kout_ptr[num_pairs] are not written.  Nothing is read outside the ptr-delimited rows, nothing is
 * written outside [0, kout_ptr[num_pairs]) of the outputs, and the call never uses hipMemset.
 *
 * The index tables are DEVICE memory: the entry point cannot look at them, and the kernel does not check them.  The
 * caller guarantees what the struct's comments say (the Python layer checks them on the host before it launches).
 *
 * head_dim must be 16, 32 or 64: anything else returns CGVP_ERR_UNSUPPORTED_DIMS before every other check; so does
 * heads * head_dim > 128 (the kernel keeps the keys of all heads in registers), after the checks of the scalar
 * arguments.  CGVP_ERR_BAD_ARG, before anything is launched (and before the num_pairs == 0 return, which launches
 * nothing and returns 0): problems NULL, num_problems outside 1..2, num_pairs < 0 or >= 2^30, heads < 1, a negative
 * graph or row count, (rows + 16) * heads * head_dim >= 2^31 for num_q or num_k, (num_qout + 16) * heads >= 2^31,
 * num_kout + 16 >= 2^31 (rows are addressed with 32-bit element offsets), a NULL q_ptr / k_ptr / q_graph / k_graph /
 * qout_ptr / kout_ptr, q NULL with num_q > 0, lse NULL with num_qout > 0, k NULL with num_k > 0, an output NULL with
 * num_kout > 0, q or k not 16-byte aligned, an lse not aligned as above, an index table not 8-byte aligned, an output
 * not 4-byte aligned.  A refused call launches nothing, for either problem. */
int cgvp_attn_node_scores_pairs(const cgvp_attn_pairs_score_problem* problems, int32_t num_problems /* 1 or 2 */,
                                int64_t num_pairs, int32_t heads, int32_t head_dim /* 16, 32, 64 */, float scale,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_PAIRSCORE_H */
