/*
 * caster_gvp_optim.h -- the optimizer update of a training step on the device: unscale, global-norm clip, Adam /
 * AdamW and the loss-scale update (train_model.py:578-587 of the reference) as at most three kernels per launch
 * table, every scalar read from device memory, so that the whole update can sit inside a captured step.
 *
 * A header of its own beside caster_gvp.h, as caster_gvp_structure.h is: the entry points below live in the same
 * libcaster_gvp.so, follow the same conventions (caller-owned DEVICE pointers, nothing allocated or retained, an
 * explicit hipStream_t, asynchronous launches, 0 = launched / >0 = hipError_t / <0 = CGVP_ERR_* from caster_gvp.h,
 * re-entrant, no state), and carry a version of their own, so the main C ABI does not move when this one grows.
 */
#ifndef CASTER_GVP_OPTIM_H
#define CASTER_GVP_OPTIM_H

#include <stdint.h>

#include "caster_gvp.h" /* CGVP_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_OPTIM_VERSION 1
/* Segments per kernel launch: the table travels BY VALUE in the kernel arguments (as cgvp_stage_item does for
 * cgvp_stage_buffers), so nothing is read from host memory when a captured launch replays.  HIP documents 4 KB of
 * kernel arguments; 80 entries of 44 bytes and the scalars stay below it.  A call with more segments issues more
 * launches, the global norm still covers all of them. */
#define CGVP_OPTIM_MAX_SEGMENTS 80
/* Elements of one norm partial (and of one workgroup of the update). */
#define CGVP_OPTIM_CHUNK 4096

int cgvp_optim_version(void);

/* One parameter tensor: fp32, contiguous, numel elements each, ANY 4-byte alignment (16-byte loads and stores are
 * used per array where its address allows them).  grad is only read.  A segment with numel == 0 is skipped and its
 * pointers are not looked at. */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} cgvp_optim_segment;

/* Host scalars, baked into the launch. */
typedef struct {
  double beta1, beta2;      /* in [0, 1) */
  double eps;               /* >= 0 */
  double weight_decay;
  int32_t decoupled;        /* 0 = Adam (L2 term added to the gradient), 1 = AdamW (the parameter is decayed) */
  int32_t dry;              /* 1 = write grad_norm and found_inf only */
  double max_norm;          /* <= 0: no clipping */
  double growth_factor, backoff_factor;
  int32_t growth_interval;  /* >= 1 */
  int32_t reserved;         /* 0 */
} cgvp_optim_hyper;

/* Bytes of workspace a step over segments of these sizes needs (numel[i] >= 0; one fp64 partial per
 * CGVP_OPTIM_CHUNK elements of every segment, plus a block of scalars), or CGVP_ERR_BAD_ARG.  8-byte aligned. */
int64_t cgvp_optim_workspace_bytes(const int64_t* numel, int32_t num_segments);

/* ONE optimizer step over `segs` (a HOST array).  Device scalars, read when the kernels run (so a replayed capture
 * sees what the caller wrote since): lr [1] float, step [1] float = the count of applied updates (torch.optim.Adam's
 * `step`), and optionally the two tensors of a torch.amp.GradScaler, scale [1] float and growth_tracker [1] int32
 * (both or neither).  Outputs grad_norm [1] and found_inf [1], floats.
 *
 * With inv = 1 / scale[0] (1 without a scale):
 *   found_inf = 1 exactly when some gradient element is NaN or +-Inf, else 0
 *   grad_norm = inv * sqrt(sum g^2) over ALL segments, accumulated in fp64: one partial per CGVP_OPTIM_CHUNK
 *               elements of a segment, summed inside the chunk and across chunks in a fixed order -- no float
 *               atomics, nothing depends on the grid or on the alignment, two calls on the same values agree bitwise
 *   c         = max_norm > 0 ? min(1, max_norm / (grad_norm + 1e-6)) : 1
 *   g^        = g * inv * c                                  (gradient memory is never written)
 * found_inf: param, exp_avg, exp_avg_sq and step stay as they are.  Otherwise step += 1 and, per element,
 *   decoupled == 0: g^ += weight_decay * p          decoupled == 1: p *= 1 - lr * weight_decay
 *   m += (g^ - m) * (1 - beta1)
 *   v  = beta2 * v + (1 - beta2) * g^ * g^
 *   p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * (torch.optim.Adam / AdamW with amsgrad=False, maximize=False).  With a scale, GradScaler.update() follows:
 *   found_inf: scale *= backoff_factor, growth_tracker = 0; otherwise growth_tracker += 1, and when it reaches
 *   growth_interval it returns to 0 and scale *= growth_factor (a grown scale that is not finite is not stored).
 * dry: grad_norm and found_inf are written, nothing else changes.
 *
 * Launches: ceil(n / CGVP_OPTIM_MAX_SEGMENTS) norm kernels, one scalar kernel, and (unless dry) as many update
 * kernels; n = segments with numel > 0.  workspace: cgvp_optim_workspace_bytes of these sizes (or more), 8-byte
 * aligned, any content; it must not be shared with a step that may run concurrently.
 *
 * CGVP_ERR_BAD_ARG, before anything is launched: num_segments < 0, a NULL table, a negative numel, a NULL or
 * 4-byte-misaligned pointer (segments, scalars), scale without growth_tracker or the reverse, a workspace that is
 * NULL, misaligned or too small, betas outside [0, 1), eps < 0 (or NaN), growth_interval < 1. */
int cgvp_optim_adam_step(const cgvp_optim_segment* segs, int32_t num_segments, const cgvp_optim_hyper* hyper,
                         const float* lr, float* step, float* scale, int32_t* growth_tracker, float* grad_norm,
                         float* found_inf, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_OPTIM_H */
