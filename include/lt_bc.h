/* lt_bc.h - the two ends of the student's behaviour-cloning step: batch assembly, the masked loss with its statistics, and the AdamW
 * update (part of the lt_env.h ABI, which includes this file; LT_ABI_VERSION 21).  Semantics: `ReplayBuffer._prepare_padded_sequence`
 * (locotouch_amd/distill/replay_buffer.py; reference locotouch/distill/replay_buffer.py:89-128), `Student.batch_loss`
 * (locotouch_amd/distill/student.py; reference locotouch/distill/student.py:119-152) and torch.optim.AdamW with amsgrad=False,
 * maximize=False.  Implemented in csrc/lt_bc.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a caller that never trains a student never calls
 * them); locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h (`_abi.BC_SIGNATURES`).
 * All data pointers are device pointers unless said otherwise; everything is stream-ordered: no host synchronisation, no allocation, no
 * host read, no float atomics.  All arithmetic is f32.  Every sum has ONE fixed order that depends on the sizes alone, so the same
 * inputs give the same bits on every run.  Validation is host-side, before anything is launched: LT_EINVAL with an lt_last_error() text
 * that names the offending argument. */
#ifndef LT_BC_H
#define LT_BC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_BC_MAX_WIDTH 4096     /* the largest row width (floats) of the loss pair and of the action pair */
#define LT_BC_ROWS_PER_GROUP 256 /* rows of one workgroup partial of lt_bc_loss_forward: a lane per row */

/* index of each field of the `stats` record (f32 [LT_BC_STATS_FIELDS], 16-byte aligned) */
enum lt_bc_stats {
  LT_BC_LOSS = 0, LT_BC_ACTION_MSE = 1, LT_BC_ACTION_MAE = 2, LT_BC_DENOM = 3, LT_BC_STATS_FIELDS = 4
};

/* BATCH ASSEMBLY, one launch.  The buffer's flat rows are policy [rows_total][pe] and tactile [rows_total][td] (contiguous f32); trajectory
 * k begins at row first[k] and has len[k] steps, consecutive steps num_envs rows apart (first, len: int64 [num_trajs]).  Column b < nb of
 * the batch is trajectory traj_idx[b] (int64 [nb], 0 <= nb <= B); a column b >= nb has length 0.  Element (t, b) is VALID iff t < len:
 *     valid:    pol[t][b][:] = policy[first + t * num_envs][:], tac[t][b][:] = tactile[the same row][:], mask[t][b] = 1
 *     invalid:  pol[t][b][:] = 0, tac[t][b][:] = 0, mask[t][b] = 0
 * pol [L][B][pe], tac [L][B][td] (contiguous f32), mask [L][B] (uint8 / bool): EVERY element is written, so the outputs need no
 * initialisation.  All offsets are 64-bit.  Rows move as 16-, 8- or 4-byte vectors, the widest that the row width and the alignment of
 * source and destination allow (348 floats: 16 bytes; 442 floats: 8 bytes); only data moves, so the result does not depend on the width.
 * An index outside [0, num_trajs) or a source row outside [0, rows_total) is never read: the element is written as invalid. */
int lt_bc_gather(const float* policy, const float* tactile, int64_t rows_total, int64_t pe, int64_t td, const int64_t* first, const int64_t* len,
                 int64_t num_trajs, const int64_t* traj_idx, int64_t nb, int64_t num_envs, int64_t L, int64_t B, float* pol, float* tac,
                 uint8_t* mask, void* stream);

/* Host-only: floats of the scratch `ws` of lt_bc_loss_forward for R rows (needs no initialisation): four per workgroup partial. */
int lt_bc_loss_ws_floats(int64_t R, size_t* floats);

/* THE MASKED LOSS AND ITS STATISTICS over R = L * B rows, two launches (workgroup partials, then the finish).  pred, target [R][W]: the
 * loss pair; sa, ta [R][A]: student and teacher actions (both NULL: the loss pair IS the action pair, A is ignored - Monolithic
 * distillation; RMA passes the embedding pair and the actions); mask [R] (uint8 / bool, m_r = 0 or 1).  With c(x) = clamp(x, -clip_range,
 * clip_range), or x itself if clip_range <= 0:
 *     stats[LT_BC_DENOM]      = sum_r m_r
 *     stats[LT_BC_LOSS]       = sum_r m_r * (sum_w (pred - target)^2 / W) / denom
 *     stats[LT_BC_ACTION_MSE] = the same expression over (sa, ta)
 *     stats[LT_BC_ACTION_MAE] = sum_r m_r * (sum_a |c(sa) - c(ta)| / A) / denom * action_scale
 * ORDER: a row's sum runs in column order in one lane; the LT_BC_ROWS_PER_GROUP rows of a workgroup are combined by a butterfly over
 * each wave and then the four waves in order; the finish adds the workgroups' partials in index order.  denom == 0 is NOT guarded: the
 * three means are then 0 / 0 = NaN, as the eager code gives. */
int lt_bc_loss_forward(const float* pred, const float* target, int64_t W, const float* sa_or_null, const float* ta_or_null, int64_t A,
                       const uint8_t* mask, int64_t R, float clip_range, float action_scale, float* stats, float* ws, void* stream);

/* The gradient of stats[LT_BC_LOSS] with respect to pred, one launch:
 *     d_pred[r][w] = ((*g / denom) * m_r / W) * (2 * (pred[r][w] - target[r][w]))
 * *g: the incoming gradient, a device scalar; denom is read from `stats` as lt_bc_loss_forward left it: no host read sits between the
 * two.  d_pred [R][W] is overwritten (every element). */
int lt_bc_loss_backward(const float* pred, const float* target, int64_t W, const uint8_t* mask, int64_t R, const float* g, const float* stats,
                        float* d_pred, void* stream);

/* torch.optim.AdamW.step() (amsgrad=False, maximize=False) on FLAT f32 buffers of n elements, one launch; `step` = the 1-based count of
 * this update.  With bc1 = 1 - beta1^step and bc2 = 1 - beta2^step (computed on the host in double, as torch does):
 *     p *= 1 - lr * weight_decay;  m += (1 - beta1) * (g - m);  v = beta2 * v + (1 - beta2) * g * g
 *     p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
 * There is no gradient clipping.  Elementwise: an element whose p, g, m and v are 0 stays 0 (the padding between tensors). */
int lt_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_BC_H */
