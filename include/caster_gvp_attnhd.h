/*
 * caster_gvp_attnhd.h -- the varlen cross attention for head dims 16, 32 and 64.  cgvp_attn_fwd / cgvp_attn_bwd /
 * cgvp_attn_weights of caster_gvp.h, their _dropout forms of caster_gvp_attndrop.h and cgvp_attn_node_scores of
 * caster_gvp_attnscore.h are compiled into one head width (embed = 16 * heads).  The entry points below are the same
 * kernels with the head width as an argument: embed = head_dim * heads, and `scale` is what the caller passes
 * (nn.MultiheadAttention: 1 / sqrt(head_dim)).  A head of 16 M dims is M k-chunks of the same 16 x 16 x 4 score product
 * and M output tiles of the same P V product; the dropout factor of (seed, offset, stream, head, q, k) does not depend on
 * the head width.
 *
 * A header of its own beside caster_gvp.h, as caster_gvp_attndrop.h and caster_gvp_attnscore.h are: the entry points
 * live in the same libcaster_gvp.so, follow the same conventions (caller-owned DEVICE pointers, nothing allocated or
 * retained, an explicit hipStream_t, asynchronous launches, 0 = launched / >0 = hipError_t / <0 = CGVP_ERR_* from
 * caster_gvp.h, re-entrant, no state), and carry a version of their own, so the main C ABI does not move.
 */
#ifndef CASTER_GVP_ATTNHD_H
#define CASTER_GVP_ATTNHD_H

#include <stdint.h>

#include "caster_gvp.h"          /* cgvp_attn_problem, cgvp_rng, CGVP_ERR_* */
#include "caster_gvp_attnscore.h" /* cgvp_attn_score_problem */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_ATTN_HD_VERSION 1

int cgvp_attn_hd_version(void);

/* head_dim must be 16, 32 or 64: anything else returns CGVP_ERR_UNSUPPORTED_DIMS, before every other check and before
 * anything is launched.  With head_dim = 16 each call is, bit for bit, the entry point it is named after.
 *
 * Every buffer of `problems` is that of cgvp_attn_fwd / cgvp_attn_bwd / cgvp_attn_weights with rows of
 * heads * head_dim floats (q, k, v, out, g_out, g_q, g_k, g_v) and of `heads` floats (lse, delta).  The two problems of
 * one call share heads and head_dim; directions of different widths take one call each.
 *
 * rng == NULL: no dropout, the argument checks of cgvp_attn_fwd / cgvp_attn_bwd.  rng != NULL: one cgvp_rng per
 * problem, the arithmetic, the factor and the argument checks of cgvp_attn_fwd_dropout / cgvp_attn_bwd_dropout
 * (caster_gvp_attndrop.h).
 *
 * CGVP_ERR_BAD_ARG, before anything is launched (and before the num_pairs == 0 return, which launches nothing and
 * returns 0): everything the entry points above reject, with the 32-bit offset limit taken at this width:
 * (rows + 16) * heads * head_dim >= 2^31. */
int cgvp_attn_fwd_hd(const cgvp_attn_problem* problems, int32_t num_problems, int64_t num_pairs, int32_t heads,
                     int32_t head_dim, float scale, const cgvp_rng* rng /* one per problem, or NULL */, void* stream);
int cgvp_attn_bwd_hd(const cgvp_attn_problem* problems, int32_t num_problems, int64_t num_pairs, int32_t heads,
                     int32_t head_dim, float scale, const cgvp_rng* rng /* one per problem, or NULL */, void* stream);
int cgvp_attn_weights_hd(const cgvp_attn_problem* problems, int32_t num_problems, int64_t num_pairs, int32_t heads,
                         int32_t head_dim, float scale, void* stream);

/* cgvp_attn_node_scores with rows of heads * head_dim floats.  The kernel keeps the keys of all heads in registers:
 * it is compiled for heads * head_dim <= 16 * CGVP_ATTN_SCORE_MAX_HEADS (an embed width of at most 128); a wider
 * shape returns CGVP_ERR_UNSUPPORTED_DIMS (reduce the dense weights of cgvp_attn_weights_hd instead). */
int cgvp_attn_node_scores_hd(const cgvp_attn_score_problem* problems, int32_t num_problems, int64_t num_pairs,
                             int32_t heads, int32_t head_dim, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_ATTNHD_H */
