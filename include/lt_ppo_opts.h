/* lt_ppo_opts.h - two options of the reference's feed-forward ActorCritic + PPO pair on the fused path (part of the lt_env.h ABI, which
 * includes this file; LT_ABI_VERSION 21): `noise_std_type="log"` (loco_rl/loco_rl/modules/actor_critic.py:62-66,109-112) and
 * `normalize_advantage_per_mini_batch` (loco_rl/loco_rl/algorithms/ppo.py:41,176,223-225).  Implemented in csrc/lt_ppo.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a run with the scalar std and whole-rollout
 * advantage normalisation never calls the first and the third); locotouch_amd/_abi.py derives their binding from this file by the same
 * rule as from lt_env.h.  All pointers are device pointers, float pointers 4-byte and idx 8-byte aligned; every entry validates its
 * arguments on the host ("<function>: invalid argument: <field> must be ...", LT_EINVAL, nothing launched), is stream-ordered,
 * allocates nothing and reads nothing back. */
#ifndef LT_PPO_OPTS_H
#define LT_PPO_OPTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* std[a] = exp(log_std[a]) for a < A, 1 <= A <= 16: one launch.  The exponential is the device function lt_ppo_loss_opts forms its
 * sigma with, so the sigma a rollout stores and the sigma the loss forms from an unchanged log_std are the same bits (the probability
 * ratio of the first minibatch step of an update then differs from 1 only by the forward pass, as with the scalar std). */
int lt_std_from_log(const float* log_std, int A, float* std, void* stream);

/* lt_ppo_loss (lt_env.h) with two options; lt_ppo_loss itself is this entry with (0, NULL).
 * std_is_log != 0: `std` points at log_std [A] and sigma_a = exp(log_std[a]).  acc[4 + a] and out[8 + a] then hold the gradient with
 *   respect to LOG sigma_a - the sigma gradient times sigma_a, the entropy term contributing -entropy_coef - which lt_ppo_lr_rule
 *   copies into the parameter's gradient slot as it does the sigma gradient.  out[3] is still the entropy.
 * adv_stats != NULL: two floats (mean, 1 / (std + 1e-8)) as lt_adv_stats writes them; a row's advantage enters as
 *   (adv - adv_stats[0]) * adv_stats[1] where it is loaded (through idx, if given). */
int lt_ppo_loss_opts(const float* mu, const float* std, const float* value, const float* actions, const float* old_logp, const float* adv,
                     const float* returns, const float* old_values, const float* old_mu, const float* old_sigma, const int64_t* idx, int64_t M,
                     int A, float clip, float value_loss_coef, float entropy_coef, int use_clipped_value_loss, int std_is_log,
                     const float* adv_stats, float* dmu, float* dvalue, float* acc, float* out, void* stream);

/* The per-minibatch advantage statistics of one update (ppo.py:223-225: (adv - adv.mean()) / (adv.std() + 1e-8)) in ONE launch: for
 * minibatch b < nmb over rows idx[b * M .. (b + 1) * M) of the whole-storage `adv` (idx == NULL: rows b * M .. themselves),
 *   stats[2 b] = mean,   stats[2 b + 1] = 1 / (std + 1e-8f)   with the UNBIASED std, as torch.std.
 * Two passes - the mean, then the squared deviations from it - summed in float64 in a fixed order (one workgroup per minibatch, no
 * atomics: the same bits every run); never E[x^2] - E[x]^2.  M >= 2 (the std of one element is NaN in the reference), 1 <= nmb. */
int lt_adv_stats(const float* adv, const int64_t* idx, int64_t M, int nmb, float* stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_PPO_OPTS_H */
