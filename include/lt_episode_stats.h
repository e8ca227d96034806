/* lt_episode_stats.h - statistics over the finished episodes of ALL envs, kept on the device (part of the lt_env.h ABI;
 * LT_ABI_VERSION 21).  lt_telemetry.h gives time series of a few envs; this unit gives the population view an evaluation table needs:
 * per metric the number of finished episodes and the sum, the sum of squares, the minimum and the maximum of the episodes' values, and
 * how the episodes ended.  The reference has nothing here (its play loop prints env 0's observations).  Implemented in
 * csrc/lt_episode_stats.hip.
 *
 * An optional unit in a header of its own (a caller that keeps no statistics never calls it); locotouch_amd/_abi.py derives the binding
 * from this file (`_abi.EPISODE_STATS_SIGNATURES`).  Everything is stream-ordered: no allocation, no host read, no atomics; every launch
 * is graph-capturable and bit-deterministic.  The code is compiled without FMA contraction and without the build's relaxed-math
 * switches: every operation below is one IEEE operation, rounded on its own.
 *
 * A CHANNEL is lt_telemetry.h's: the value of env e is base[e * env_stride + offset], converted to f32 by value.
 *
 * A METRIC has 1 ... LT_EPISODE_STATS_MAX_PAIRS channel pairs (a_p, b_p), a term g, a reduce over the steps of an episode and two
 * switches.  PER STEP, in f32:
 *     s = ((+0.0f + g(a_0, b_0)) + g(a_1, b_1)) + ...                                    left to right
 *     g:  VALUE a | ABS |a| | SQUARE a * a | DIFF_SQUARE (a - b) * (a - b) | ABS_PRODUCT |a * b|          (b is read by the last two only)
 * A step is SAMPLED by a metric unless its `dones` is set and `include_done_step` is 0: at a step whose `dones` is set the arena already
 * holds the state behind the reset, so a metric over state channels leaves that step out; the step's reward is the finished episode's.
 * OVER THE SAMPLED STEPS of an episode, with run (f32) and count (i32) both 0 at the episode's start:
 *     MEAN, SUM   run = run + s;                                       count += 1
 *     MAX         run = count == 0 ? s : (s > run ? s : run);          count += 1       (a NaN sample never replaces a number; an
 *                 episode whose FIRST sample is NaN keeps it - s > NaN is false -, and its NaN value then stays in the env's sum and
 *                 sumsq and in the totals until they are cleared: n, min and max tell which metric it was)
 *     LAST        nothing is kept: the term is read at the done step, whatever include_done_step says
 * FINISH at the done step, in f64:
 *     MEAN (double)run / (double)count | SUM, MAX (double)run | LAST (double)s;    then, with `take_sqrt`, the IEEE square root
 * An episode with count == 0 contributes nothing to a MEAN, SUM or MAX metric.  Metric index M (one behind the caller's) is built in:
 * the episode's LENGTH in steps, the done step included.
 * FOLD of a value v into the env's accumulators {n, sum, sumsq, min, max} (f64) of that metric:
 *     min = n == 0 ? v : (v < min ? v : min);   max = n == 0 ? v : (v > max ? v : max);   n = n + 1;   sum = sum + v;   sumsq = sumsq + v * v
 * CAUSES of a finished episode (i32 [LT_EPISODE_STATS_CAUSES] per env): counter b < 16 counts the episodes whose `term_bits` value at
 * the done step (converted to f32 like every channel, then truncated to an integer; its low 16 bits count) has bit b set, counter 16
 * those whose `time_out` channel is non-zero there, counter 17 the episodes.
 * ARMING: an env is armed from lt_episode_stats_begin on with skip_running == 0.  With skip_running == 1 its first done only arms it
 * (that episode was already running when the recording began: it is dropped, causes and length included).
 *
 * The PLAN, in caller-owned device memory (16 x 12 pairs do not fit into kernel arguments), written by one async copy:
 *     lt_episode_stats_plan_bytes = LT_EPISODE_STATS_PLAN_HEADER_BYTES + LT_EPISODE_STATS_PLAN_METRIC_BYTES * nmetrics
 * The STATE of N envs and M metrics, in caller-owned device memory, 16-byte aligned; arrays one behind the other, the env index last
 * (neighbouring threads touch neighbouring elements):
 *     finished   f64 [M + 1][5][N]     {n, sum, sumsq, min, max} (LT_EPISODE_STATS_N ... _MAX) of metric m, m == M: the length
 *     run        f32 [M][N]
 *     count      i32 [M][N]
 *     steps      i32 [N]               steps of the running episode so far
 *     causes     i32 [18][N]
 *     armed      u8  [N]
 *     lt_episode_stats_state_bytes = N * (40 * (M + 1) + 8 * M + 4 + 72 + 1)
 * The RESULT block of lt_episode_stats_reduce, 8-byte aligned:
 *     totals     f64 [M + 1][5]        n, sum and sumsq summed over the envs; min and max over the envs with n > 0 (0 where there are none)
 *     causes     i64 [18]
 *     lt_episode_stats_result_bytes = 40 * (M + 1) + 144
 * The f64 sums over the envs have ONE order: thread t of 256 adds the envs t, t + 256, t + 512, ... in index order onto +0.0, into
 * partial[t]; then for stride = 128, 64, ..., 1 every t < stride does partial[t] = partial[t] + partial[t + stride]; partial[0] is the
 * total.  Min and max are combined along the same walk (an operand with n == 0 is passed over; otherwise b < a ? b : a, b > a ? b : a
 * with a the earlier one); the integer sums are order-free. */
#ifndef LT_EPISODE_STATS_H
#define LT_EPISODE_STATS_H

#include <stddef.h>
#include <stdint.h>

#include "lt_telemetry.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LT_EPISODE_STATS_MAX_METRICS 16
#define LT_EPISODE_STATS_MAX_PAIRS 12
#define LT_EPISODE_STATS_MAX_ENVS 16776960     /* 16 * 65535 * 16: a thread per env, 256 per workgroup, at most 65535 workgroups */
#define LT_EPISODE_STATS_CAUSES 18
#define LT_EPISODE_STATS_PLAN_HEADER_BYTES 112 /* 16 + the dones, time_out and term_bits channels */
#define LT_EPISODE_STATS_PLAN_METRIC_BYTES 784 /* 16 + 12 pairs of two channels */

enum lt_episode_stats_term {
  LT_EPISODE_STATS_VALUE = 0,
  LT_EPISODE_STATS_ABS,
  LT_EPISODE_STATS_SQUARE,
  LT_EPISODE_STATS_DIFF_SQUARE,
  LT_EPISODE_STATS_ABS_PRODUCT
};

enum lt_episode_stats_reduce {
  LT_EPISODE_STATS_MEAN = 0,
  LT_EPISODE_STATS_SUM,
  LT_EPISODE_STATS_MAX,
  LT_EPISODE_STATS_LAST
};

enum lt_episode_stats_field {
  LT_EPISODE_STATS_F_N = 0,
  LT_EPISODE_STATS_F_SUM,
  LT_EPISODE_STATS_F_SUMSQ,
  LT_EPISODE_STATS_F_MIN,
  LT_EPISODE_STATS_F_MAX,
  LT_EPISODE_STATS_FIELDS
};

typedef struct lt_episode_stats_pair {
  lt_telemetry_channel a;
  lt_telemetry_channel b;   /* absent: base == NULL (looked at by DIFF_SQUARE and ABS_PRODUCT only) */
} lt_episode_stats_pair;

typedef struct lt_episode_stats_metric {
  int32_t npairs;             /* 1 ... LT_EPISODE_STATS_MAX_PAIRS */
  int32_t term;               /* lt_episode_stats_term */
  int32_t reduce;             /* lt_episode_stats_reduce */
  int32_t take_sqrt;          /* 0 | 1: the square root of the finished value */
  int32_t include_done_step;  /* 0 | 1 */
  lt_episode_stats_pair pairs[LT_EPISODE_STATS_MAX_PAIRS];  /* entries from `npairs` on are ignored */
} lt_episode_stats_metric;

/* Host-only: the byte counts by the formulas above.  LT_EINVAL for nmetrics outside 1 ... LT_EPISODE_STATS_MAX_METRICS, nenvs outside
 * 1 ... LT_EPISODE_STATS_MAX_ENVS or a null `bytes`. */
int lt_episode_stats_plan_bytes(int nmetrics, size_t* bytes);
int lt_episode_stats_state_bytes(int nmetrics, int nenvs, size_t* bytes);
int lt_episode_stats_result_bytes(int nmetrics, size_t* bytes);

/* Writes the plan of `metrics` (HOST array) and of the `dones`, `time_out` and `term_bits` channels (HOST) for `nenvs` envs into
 * `device_plan` (device, 16-byte aligned, `bytes` >= lt_episode_stats_plan_bytes): ONE async copy on `stream` from a staging copy of
 * its own (the caller's arrays are free on return).
 * LT_EINVAL with "<function>: invalid argument: <field> must be ...", before anything is copied, for: a null metrics, dones, time_out
 * or term_bits; nmetrics or nenvs outside its range; a metric's npairs outside 1 ... LT_EPISODE_STATS_MAX_PAIRS, term outside 0 ... 4,
 * reduce outside 0 ... 3, take_sqrt or include_done_step outside 0 ... 1; a channel (a of every pair, b of every pair of a DIFF_SQUARE or
 * ABS_PRODUCT metric, the three named ones) with a dtype outside 0 ... 3, a base that is null or not aligned to its element, a negative
 * env_stride or offset; a null or misaligned device_plan; too few bytes.  (Whether (nenvs - 1) * env_stride + offset lies inside a
 * channel's array only the caller knows.) */
int lt_episode_stats_plan_write(const lt_episode_stats_metric* metrics, int nmetrics, const lt_telemetry_channel* dones,
                                const lt_telemetry_channel* time_out, const lt_telemetry_channel* term_bits, int nenvs, void* device_plan,
                                size_t bytes, void* stream);

/* Zeroes the whole state of `nenvs` envs and `nmetrics` metrics and arms every env (skip_running == 0) or none (1): ONE launch.
 * LT_EINVAL for counts outside their ranges, a null or misaligned (16 bytes) state, a skip_running outside 0 ... 1. */
int lt_episode_stats_begin(void* state, int nmetrics, int nenvs, int skip_running, void* stream);

/* One env step's worth (see above): ONE launch, a thread per env, 256 per workgroup.  It reads the plan's channels, accumulates, and at
 * a set `dones` folds the finished episode into the env's own accumulators.  LT_EINVAL, before the launch, for counts outside their
 * ranges or a null or misaligned (16 bytes) device_plan or state.  A plan that lt_episode_stats_plan_write did not write for these
 * counts makes the launch do nothing. */
int lt_episode_stats_step(const void* device_plan, void* state, int nmetrics, int nenvs, void* stream);

/* Restarts the RUNNING part of the state - run, count and steps become 0, every env is armed (skip_running == 0) or none (1) - and leaves
 * `finished` and `causes` alone: ONE launch.  For a caller that resets all envs without a `dones` (lt_env_reset_all between two
 * collections): the episodes cut off there are dropped, not merged into the ones that start.  Refusals as lt_episode_stats_begin's. */
int lt_episode_stats_restart_running(void* state, int nmetrics, int nenvs, int skip_running, void* stream);

/* Zeroes `finished` and `causes` only; running episodes (run, count, steps, armed) are untouched.  ONE launch. */
int lt_episode_stats_clear_finished(void* state, int nmetrics, int nenvs, void* stream);

/* The totals over the envs into `result` (device, 8-byte aligned, lt_episode_stats_result_bytes): ONE launch of ONE workgroup of 256
 * threads, in the order stated above.  The state is only read. */
int lt_episode_stats_reduce(const void* state, int nmetrics, int nenvs, void* result, void* stream);

/* VALUE queries: the number of kernel launches one lt_episode_stats_step / _reduce issues (1), or a negative LT_* code for arguments
 * it refuses.  Host-only. */
int lt_episode_stats_step_launches(const void* device_plan, const void* state, int nmetrics, int nenvs);
int lt_episode_stats_reduce_launches(const void* state, int nmetrics, int nenvs, const void* result);

#ifdef __cplusplus
}
#endif

#endif /* LT_EPISODE_STATS_H */
