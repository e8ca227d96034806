/* lt_obs_norm.h - device path of the trainer's running observation normaliser (part of the lt_env.h ABI, which includes this
 * file; LT_ABI_VERSION 21).  Semantics: EmpiricalNormalization of the reference, loco_rl/loco_rl/modules/normalizer.py:14-76, as the
 * runner uses it (loco_rl/loco_rl/runners/on_policy_runner.py:85-95,163-172).  Implemented in csrc/lt_obs_norm.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a trainer without `empirical_normalization`
 * never calls them); locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h.
 * All pointers are device pointers; stream-ordered, no host sync, no float atomics (fixed summation order: same bits every run). */
#ifndef LT_OBS_NORM_H
#define LT_OBS_NORM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of the workspace one network needs for a batch of n rows of width d.  n in [1, 2^31), d in [1, 1024].  16-byte aligned,
 * ZEROED once before its first use and then left to the kernels: besides the per-workgroup partial statistics it carries f64 copies
 * of mean and var, on which the recurrence runs (the module's f32 buffers receive their roundings; an f32 mean updated in place would
 * drift from the recurrence by half an ulp per step).  The copies are used only while the f32 buffers hold exactly what the kernels
 * last wrote; after anything else has written them (a loaded checkpoint, the torch class) the recurrence restarts from the f32 values,
 * so one workspace belongs to one normaliser. */
int lt_obs_norm_ws_floats(int64_t n, int d, size_t* floats);

/* One training-mode `forward` of the normaliser (normalizer.py:42-54) for up to two networks (d1 = 0: network 0 alone) on the same n
 * rows, in at most two launches.
 * merge != 0: `update` (normalizer.py:57-72) - if *count >= until (until < 0: no limit, the reference's `until=None`) nothing is
 *   updated (normalizer.py:60); else count += n, rate = n / count, and mean / var / std ([d] f32, the module's `_mean`, `_var`,
 *   `_std`) and count (int64, the module's `count`) are rewritten IN PLACE with the batch's mean and biased variance
 *   (normalizer.py:63-72).  The column statistics are two-pass sums in f64 merged with Chan's formula in a fixed order, never
 *   E[x^2] - E[x]^2.
 * merge == 0: evaluation mode, the running buffers are only read (the workspace may be NULL).
 * While updating, std and 1 / (std + eps) are roundings of the f64 root of the f64 var; where nothing is updated (merge == 0, or
 * `until` reached) 1 / (std + eps) is formed from the f32 std buffer as it stands.
 * Either way snap ([2][d]: mean, then 1 / (std + eps)) receives the statistics the rows are normalised with, and, when out is
 * non-NULL, out[n][d] = (rows - mean) * (1 / (std + eps)) (normalizer.py:54).  out must not alias rows. */
int lt_obs_norm_update(int64_t n, int merge, int64_t until, double eps,
                       const float* rows0, int d0, float* mean0, float* var0, float* std0, int64_t* count0, float* snap0, float* out0, float* ws0,
                       const float* rows1, int d1, float* mean1, float* var1, float* std1, int64_t* count1, float* snap1, float* out1, float* ws1,
                       void* stream);

/* out[r][:] = (rows[r][:] - mean_s) * inv_s (normalizer.py:54) with (mean_s, inv_s) = the [2][d] snapshot at
 * snaps + s * snap_stride floats, s = r / rows_per_snap: one launch normalises a whole [T][n][d] rollout storage through its per-slot
 * snapshots (rows_per_snap = n).  out may be rows itself (in place). */
int lt_obs_norm_apply(const float* rows, int64_t nrows, int d, const float* snaps, int64_t snap_stride, int64_t rows_per_snap, float* out,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_OBS_NORM_H */
