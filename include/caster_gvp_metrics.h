/*
 * caster_gvp_metrics.h -- the evaluation metrics of a run on the device: what the reference's loops keep on the host
 * around the training step (train_model.py:609-631, 645-674: a `.item()` per batch for a batch-size-weighted mean of
 * the losses) and what its test evaluation computes at the end (train_model.py:759-793: MSE, MAE, Pearson and the
 * concordance index, the last one a Python double loop over all pairs of rows).  Here predictions and targets are
 * appended to device buffers without a host synchronisation (so the append can sit inside a captured step), and one
 * call computes every metric from the buffers; the concordance index is an exact all-pairs integer count.
 *
 * A header of its own beside caster_gvp.h, as caster_gvp_optim.h is: the entry points below live in the same
 * libcaster_gvp.so, follow the same conventions (caller-owned DEVICE pointers, nothing allocated or retained, an
 * explicit hipStream_t, asynchronous launches, 0 = launched / >0 = hipError_t / <0 = CGVP_ERR_* from caster_gvp.h,
 * re-entrant, no state), and carry a version of their own, so the main C ABI does not move when this one grows.
 */
#ifndef CASTER_GVP_METRICS_H
#define CASTER_GVP_METRICS_H

#include <stdint.h>

#include "caster_gvp.h" /* CGVP_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_METRICS_VERSION 1
/* Rows of one tile of the pair count: one workgroup counts one tile pair of the lower triangle at a time. */
#define CGVP_METRICS_TILE 256
/* Rows of one partial of the moment sums. */
#define CGVP_METRICS_CHUNK 1024
/* Most rows a buffer may hold (2^26): the pair counts then stay below 2^51, far from 2^63 and exact in fp64. */
#define CGVP_METRICS_MAX_ROWS 67108864

int cgvp_metrics_version(void);

/* state: DEVICE int64 [2] = {rows stored, rows dropped}, 8-byte aligned.  Zeroes both (with a kernel). */
int cgvp_metrics_reset(int64_t* state, void* stream);

/* Appends the n fp32 values of pred and of target (any 4-byte alignment) to pred_buf / target_buf [capacity] at the
 * position state[0] holds WHEN THE KERNEL RUNS (a captured launch replays correctly), then state[0] += rows written.
 * Rows that do not fit are not written and are counted in state[1]; nothing is written outside [0, capacity) of the
 * two buffers (a state[0] outside [0, capacity] is read as the nearer end).  dry != 0: the launch happens and writes
 * nothing at all (the warm-up passes of a capture).  n == 0 launches nothing.  One workgroup, no atomics: appends to
 * one state must be ordered by their stream.
 * CGVP_ERR_BAD_ARG, before anything is launched: n < 0, capacity < 0 or > CGVP_METRICS_MAX_ROWS, a NULL or
 * misaligned pointer (4 bytes for the float arrays, 8 for state; the buffers may be NULL when capacity == 0). */
int cgvp_metrics_append(const float* pred, const float* target, int64_t n, float* pred_buf, float* target_buf,
                        int64_t capacity, int64_t* state, int32_t dry, void* stream);

/* Bytes of workspace cgvp_metrics_compute needs for max_rows rows, or CGVP_ERR_BAD_ARG (max_rows < 0 or
 * > CGVP_METRICS_MAX_ROWS).  8-byte aligned, any content. */
int64_t cgvp_metrics_workspace_bytes(int64_t max_rows);

/* Every metric of the first n rows of pred_buf / target_buf (fp32, any 4-byte alignment):
 *   n = count_dev ? min(max(count_dev[0], 0), max_rows) : max_rows
 * count_dev (DEVICE int64, the `state` of the append) is read by the kernels: the grids are sized from max_rows and
 * workgroups beyond n exit, so a captured or repeated call follows the count.  Rows behind n are never looked at.
 *
 *   out_counts  int64 [4]  = {n, concordant, tied_pred, comparable}
 *   out_vals    double [6] = {mse, mae, pearson, ci, mean_pred, mean_target}
 *
 * Moments: fp64 accumulation of the fp32 inputs in two passes (means, then centred sums), one partial per
 * CGVP_METRICS_CHUNK rows, summed inside the chunk and across chunks in a fixed order -- no float atomics, two calls
 * on the same values agree bitwise.  mse = sum (p - t)^2 / n, mae = sum |p - t| / n,
 * pearson = sum p~ t~ / sqrt(sum p~^2 * sum t~^2) with p~ = p - mean_pred, t~ = t - mean_target, NaN when either sum
 * of squares is 0 (what torch.corrcoef returns).  n == 0: every value is NaN except ci = 0.
 *
 * Pair counts over all i > j, fp32 comparisons that follow IEEE (a NaN compares false everywhere):
 *   comparable = #{t_i > t_j or t_i < t_j}
 *   concordant = #{(t_i > t_j and p_i > p_j) or (t_i < t_j and p_i < p_j)}
 *   tied_pred  = #{comparable and p_i == p_j}
 *   ci         = (concordant + 0.5 * tied_pred) / comparable in fp64, 0 when comparable == 0
 * which is calc_concordance_index of train_model.py:773-790 term for term, its treatment of NaN included: a NaN
 * target makes its pairs incomparable, a NaN prediction on a comparable pair counts in the denominator only.
 * Integer sums do not depend on their order: the counts are exact and reproducible.
 *
 * Launches: two moment kernels with a one-workgroup kernel between them, the pair-count kernel (one workgroup per
 * tile pair of CGVP_METRICS_TILE rows, striding over the triangle when it has more tile pairs than the grid), and a
 * one-workgroup kernel that sums the partials and writes the outputs.  max_rows == 0 launches only the last.
 * workspace: cgvp_metrics_workspace_bytes(max_rows) or more; not shared with a call that may run concurrently.
 *
 * CGVP_ERR_BAD_ARG, before anything is launched: max_rows < 0 or > CGVP_METRICS_MAX_ROWS, a NULL or misaligned
 * pointer (4 bytes for the float arrays, which may be NULL when max_rows == 0; 8 for count_dev -- which may be
 * NULL --, out_counts, out_vals and workspace), a workspace that is too small. */
int cgvp_metrics_compute(const float* pred_buf, const float* target_buf, const int64_t* count_dev, int64_t max_rows,
                         int64_t* out_counts, double* out_vals, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_METRICS_H */
