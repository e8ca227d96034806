/* lt_ledger.h - the episode ledger of DAgger collection and evaluation (part of the lt_env.h ABI, which includes this file;
 * LT_ABI_VERSION 21).  Semantics: the per-step trajectory bookkeeping of the reference's replay buffer (locotouch/distill/replay_buffer.py:
 * 58-72 for collect_data, :139-150 for evaluate), which locotouch_amd/distill/replay_buffer.py replays on the host from a blocking copy of
 * the rewards and dones; here the same rules run on the device, behind each env step.  Implemented in csrc/lt_ledger.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a caller that keeps its books on the host never
 * calls them); locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h (`_abi.LEDGER_SIGNATURES`).
 * All data pointers are device pointers unless said otherwise; everything is stream-ordered: no host synchronisation, no allocation, no
 * host read, no atomics of any kind.  Every list has ONE fixed order (step order, env-id order inside a step), whatever the schedule of
 * the waves.
 *
 * STATE: one caller-owned device allocation of lt_ledger_state_bytes(n) = 64 + 16 n bytes, 16-byte aligned, ZEROED once before its
 * first use:
 *     int64_t head[8]            step, kept_steps, episodes, trajs, stopped_at, overflow, keep_target, episode_target (LT_LEDGER_* below)
 *     double  reward_sum[n]      the running reward of the env's current episode
 *     int64_t start[n]           the step behind which the env's current trajectory began
 * The caller reads the head with one plain 64-byte device-to-host copy.  step counts the lt_ledger_step calls that were not ignored,
 * stopped_at is 0 while the ledger is running and the step it stopped on afterwards, overflow counts list entries that did not fit,
 * episodes and trajs count the entries appended to the two lists since lt_ledger_begin (written or not).
 *
 * RULES of one lt_ledger_step (s = the new value of step; D = the envs with done != 0, ascending):
 *   - stopped_at != 0: nothing happens; head, sums, starts and lists stay bit for bit.
 *   - reward_sum[e] += (double)reward[e] for every env: one f64 add per env per step, in step order.
 *   - every env of D, in order, appends (reward_sum[e], s - start[e]) to the episode list - start as it was before this step - and sets
 *     reward_sum[e] = 0.
 *   - env e of D is KEPT iff keep_target < 0, or kept_steps (before this step) + the lengths of the envs of D below e < keep_target.
 *     Lengths are >= 1, so the kept envs are a prefix of D.  A kept env appends (e, start[e], s) to traj (if one is given), adds its
 *     length to kept_steps and sets start[e] = s.  An env of D that is not kept leaves start alone.
 *   - then stopped_at = s if keep_target >= 0 and kept_steps >= keep_target, or if episode_target >= 0 and episodes >= episode_target.
 *     The episode list holds every done env of the stopping step.
 *   - entry number k of a list (counted from lt_ledger_begin) goes to slot k - first of the list given with THIS call; a slot outside
 *     [0, cap) is not written and counted in overflow, the entries that fit are still written, in order.  `first` lets a caller that has
 *     read the first entries away reuse their slots: it passes the number of entries it has consumed.
 * Validation is host-side: LT_EINVAL with an lt_last_error() text that names the offending argument. */
#ifndef LT_LEDGER_H
#define LT_LEDGER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* index of each head field, in int64 units from the start of the state */
enum lt_ledger_head {
  LT_LEDGER_STEP = 0, LT_LEDGER_KEPT_STEPS = 1, LT_LEDGER_EPISODES = 2, LT_LEDGER_TRAJS = 3, LT_LEDGER_STOPPED_AT = 4,
  LT_LEDGER_OVERFLOW = 5, LT_LEDGER_KEEP_TARGET = 6, LT_LEDGER_EPISODE_TARGET = 7, LT_LEDGER_HEAD_FIELDS = 8
};

/* Host-only: bytes of the state for n envs (64 + 16 n).  n >= 1. */
int lt_ledger_state_bytes(int64_t n, size_t* bytes);

/* Starts a run: start[e] = 0, every counter of the head 0, reward_sum[e] = (double)reward_sums_in[e] (f32 [n]; NULL: zeros),
 * keep_target and episode_target as given (below 0: none, stored as -1).  One launch. */
int lt_ledger_begin(void* state, int64_t n, const float* reward_sums_in_or_null, int64_t keep_target, int64_t episode_target, void* stream);

/* One env step's bookkeeping by the rules above.  reward: f32 [n]; done: uint8 / bool [n]; ep_reward f64 / ep_length int64: the episode
 * list, ep_cap slots each, slot 0 = entry number ep_first (both NULL with ep_cap 0: every episode counts as overflow); traj: int64
 * [traj_cap][3] = (env, first step, end step), slot 0 = entry number traj_first (NULL with traj_cap 0: no trajectory list is kept and
 * none overflows).  A NULL list with a non-zero cap, a negative cap or a negative first is an error.  One launch: one workgroup of 1024
 * lanes walks the envs in chunks of 1024 (ballot + popcount for the slot, a wave then cross-wave scan of the lengths for the
 * kept-steps prefix, both carried from chunk to chunk). */
int lt_ledger_step(void* state, int64_t n, const float* reward, const uint8_t* done, double* ep_reward, int64_t* ep_length, int64_t ep_first,
                   int64_t ep_cap, int64_t* traj, int64_t traj_first, int64_t traj_cap, void* stream);

/* reward_sums_out[e] = (float)reward_sum[e] (round to nearest even): the sums a later lt_ledger_begin carries on from.  The state is only
 * read.  One launch. */
int lt_ledger_end(const void* state, int64_t n, float* reward_sums_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_LEDGER_H */
