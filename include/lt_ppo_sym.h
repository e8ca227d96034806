/* lt_ppo_sym.h - the mirror-symmetric PPO update on the fused path: the reference's `symmetry_cfg` branch (loco_rl/loco_rl/algorithms/
 * ppo.py:45,66-84,216-246,304-337) with `use_data_augmentation`, with or without the mirror loss.  Implemented in csrc/lt_ppo_sym.hip.
 *
 * A header of its own, NOT included by lt_env.h (whose ABI version and signatures it leaves alone): the entry points are one optional
 * unit - a run without `symmetry_cfg` never calls them - and locotouch_amd/_abi.py binds them by one row of its header table.
 *
 * The left-right mirror of a row is a signed permutation of its columns, mirrored[c] = sign[c] * row[src[c]] (locotouch_amd/rl/
 * symmetry.py builds the tables from the env's description).  Its DEVICE form is D int32 words, word c = src[c] | (sign[c] < 0 ? 1 << 31 :
 * 0): only lt_sym_table_pack writes it, after it has checked the table on the host, so an invalid table never reaches a kernel.
 *
 * Unless stated, pointers are device pointers, float pointers 4-byte and idx 8-byte aligned; every entry validates its arguments on
 * the host ("<function>: invalid argument: <field> must be ...", LT_EINVAL, nothing launched), is stream-ordered, allocates nothing and
 * reads nothing back. */
#ifndef LT_PPO_SYM_H
#define LT_PPO_SYM_H

#include <stddef.h>
#include <stdint.h>

#define LT_SYM_MAX_D 1024 /* widest row a table describes */

#ifdef __cplusplus
extern "C" {
#endif

/* HOST src[D] (int32), HOST sign[D] (float), 1 <= D <= 1024 -> the device form table[D] (int32, 4-byte aligned), in one launch that
 * carries the packed table in its arguments (the host arrays are free again when the call returns).  Refused unless src is a permutation
 * of 0 .. D - 1 and every sign is +1 or -1. */
int lt_sym_table_pack(const int32_t* src_host, const float* sign_host, int D, int32_t* table, void* stream);

/* The minibatches of one update with their mirror images, gathered once: from storage rows [R][D] (f32, or with rows_bf16 != 0 the bit
 * patterns of bf16 rows, 2-byte aligned), idx[nmb * m] (row of the storage behind minibatch row b * m + j) and a packed table, f32
 *   out[b][0][j][c] = rows[idx[b m + j]][c]        out[b][1][j][c] = sign[c] * rows[idx[b m + j]][src[c]]        (out [nmb][2][m][D])
 * so that minibatch b's forward input is ONE contiguous block of 2 m rows, [original; mirrored].  A wave reads a storage row once,
 * coalesced, permutes it through LDS and writes both halves coalesced; any D in range and any row alignment the element type allows
 * (rows of 270 floats are 8-byte aligned, of 270 bf16 4-byte).  No atomics; a row no index refers to is never read, and an index
 * outside [0, R) writes nothing.  The sign is applied to the bit pattern: copies, sign flips and the exact bf16 -> f32 widening only. */
int lt_sym_gather_rows(const void* rows, int rows_bf16, int64_t R, int D, const int64_t* idx, int nmb, int64_t m, const int32_t* table,
                       float* out, void* stream);

/* lt_ppo_loss_opts (lt_ppo_opts.h) for the augmented minibatch: mu [2 M][A] and value [2 M] are the forward outputs of the 2 M rows
 * [original; mirrored]; the seven storage tensors are read through idx[M] (NULL: rows 0 .. M - 1) ONCE per original row r, and a thread
 * scores the pair (r, M + r): row r as lt_ppo_loss_opts does, row M + r against the MIRRORED action sign_a * actions[idx[r]][src_a]
 * (act_table: the packed action table, A words) with the same old log-prob, advantage, return and old value.  sigma is NOT permuted:
 * the reference evaluates the mirrored actions under Normal(mu(mirrored obs), std) with std in its own order.
 *   surrogate and value loss: sums over 2 M rows, means with divisor 2 M; dmu [2 M][A], dvalue [2 M] carry the factor 1 / (2 M)
 *   the sigma (std_is_log: log sigma) gradient: summed over all 2 M rows, factor 1 / (2 M)
 *   KL: the first M rows, divided by M; entropy as in lt_ppo_loss
 *   mirror term: d = mu[M + r][a] - sign_a * mu[r][src_a]; acc[3] = sum d^2; out[5] = acc[3] / (M A) (the reference's MSELoss);
 *     with mirror_coeff != 0: dmu[M + r][a] += mirror_coeff * 2 d / (M A) and out[0] += mirror_coeff * out[5]; the target is detached,
 *     nothing flows into row r
 *   acc[20], acc[21]: max |dmu|, max |dvalue| over both halves, the mirror term included
 *   *sym_sum += out[5] by one lane of the finish launch (a running sum over the optimizer steps; read once per update)
 * Every other slot of acc [24] and out [24] keeps lt_ppo_loss's meaning; out and sym_sum may be NULL (then no finish launch / no sum).
 * One launch plus the one-wave finish. */
int lt_ppo_loss_sym(const float* mu, const float* std, const float* value, const float* actions, const float* old_logp, const float* adv,
                    const float* returns, const float* old_values, const float* old_mu, const float* old_sigma, const int64_t* idx, int64_t M,
                    int A, float clip, float value_loss_coef, float entropy_coef, int use_clipped_value_loss, int std_is_log,
                    const float* adv_stats, const int32_t* act_table, float mirror_coeff, float* dmu, float* dvalue, float* acc, float* out,
                    float* sym_sum, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_PPO_SYM_H */
