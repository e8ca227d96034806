/* lt_ppo_mirror.h - the PPO minibatch loss with the mirror loss WITHOUT data augmentation: the reference's `symmetry_cfg` branch with
 * `use_data_augmentation=False` (loco_rl/loco_rl/algorithms/ppo.py:305-337), with `use_mirror_loss` or for the log alone.  Implemented in
 * csrc/lt_ppo_sym.hip, beside lt_ppo_loss_sym (lt_ppo_sym.h), on the per-row functions both share with lt_ppo_loss.
 *
 * A header of its own, NOT included by lt_env.h or lt_ppo_sym.h (whose signatures it leaves alone): one optional entry point - the
 * augmented modes and a run without `symmetry_cfg` never call it - bound by one row of locotouch_amd/_abi.py's header table.
 *
 * Pointers are device pointers, float pointers 4-byte and idx 8-byte aligned; the arguments are validated on the host ("<function>:
 * invalid argument: <field> must be ...", LT_EINVAL, nothing launched); the call is stream-ordered, allocates nothing and reads nothing
 * back. */
#ifndef LT_PPO_MIRROR_H
#define LT_PPO_MIRROR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* lt_ppo_loss_sym's argument list, with mu [2 M][A] the actor's output on [original; mirrored] rows and value [M], dvalue [M] the
 * critic's on the M original rows alone - the critic never sees a mirrored row.
 *   rows r < M: scored as lt_ppo_loss_opts scores them (idx, std_is_log, adv_stats, clipped value loss); surrogate, value loss, KL and
 *     the sigma (log sigma) gradient are sums over M rows, every mean has the divisor M; dmu[r], dvalue[r] carry the factor 1 / M
 *   mirror term: d = mu[M + r][a] - sign_a * mu[r][src_a] (act_table: the packed action table of lt_sym_table_pack, A words);
 *     acc[3] = sum d^2; out[5] = acc[3] / (M A); dmu[M + r][a] = mirror_coeff * 2 d / (M A) - with mirror_coeff == 0 the word +0.0 - and
 *     out[0] += mirror_coeff * out[5]; the target is detached, nothing flows into row r from it
 *   acc[20]: max |dmu| over all 2 M rows; acc[21]: max |dvalue| over M rows
 *   *sym_sum += out[5] by one lane of the finish launch
 * Every other slot of acc [24] and out [24] keeps lt_ppo_loss's meaning; out and sym_sum may be NULL (then no finish launch / no sum;
 * sym_sum needs out).  One launch plus the one-wave finish; the sums are lt_ppo_loss's: a fixed order inside a block, one atomic per
 * block and slot. */
int lt_ppo_loss_mirror(const float* mu, const float* std, const float* value, const float* actions, const float* old_logp, const float* adv,
                       const float* returns, const float* old_values, const float* old_mu, const float* old_sigma, const int64_t* idx, int64_t M,
                       int A, float clip, float value_loss_coef, float entropy_coef, int use_clipped_value_loss, int std_is_log,
                       const float* adv_stats, const int32_t* act_table, float mirror_coeff, float* dmu, float* dvalue, float* acc, float* out,
                       float* sym_sum, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_PPO_MIRROR_H */
