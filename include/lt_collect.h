/* lt_collect.h - the tactile delay line and the per-step recording of the student-driven collection loop (part of the lt_env.h ABI,
 * which includes this file; LT_ABI_VERSION 21).  Semantics: TactileRecorder of the reference (locotouch/distill/tactile_recorder.py:4-34)
 * and the per-step copies of its replay buffer (locotouch/distill/replay_buffer.py:42-61), restated as a ring buffer so that nothing is
 * shifted, filled or zeroed.  Implemented in csrc/lt_collect.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a caller without a delay line never calls them);
 * locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h (`_abi.COLLECT_SIGNATURES`).
 * All data pointers are device pointers unless said otherwise; everything is stream-ordered: no host synchronisation, no allocation,
 * no host read, no atomics, no arithmetic on a row - rows are moved, so every output is bit for bit an input row (or zeros).
 *
 * STATE: one caller-owned device allocation of lt_delay_state_bytes(n, d, depth) bytes, at least 4-byte aligned (16-byte alignment
 * lets the kernels move 16 bytes per lane), ZEROED once before its first use:
 *     float   ring[n][depth][d]      the last `depth` rows pushed per env
 *     (padding to the next multiple of 16 bytes)
 *     int32_t head[n]                slot of the newest row
 *     int32_t count[n]               pushes since the env's last reset, saturating at depth
 *     int32_t delay[n]               the env's delay in steps, 0 <= delay < depth
 * so the size is 4 n depth d rounded up to a multiple of 16, plus 12 n.
 *
 * Rules per env:
 *   reset  : count = 0, delay = the freshly drawn value.  The ring is NOT touched.
 *   push   : the row is stored at slot head = (head + 1) mod depth, count = min(count + 1, depth).
 *   delayed: the row pushed min(delay, count - 1) pushes ago; zeros while count == 0 (between a reset and the next push).
 * This is the reference's shift register, whose first signal after a reset fills the whole register: a slot not yet overwritten since
 * the reset would hold that first signal, which is the oldest row the rule can reach and is still in the ring while count <= depth.
 *
 * Row operands are [n][d] f32 with unit column stride and their own ROW STRIDE in floats (a column slice of wider rows is read or written
 * in place).  Validation is host-side: LT_EINVAL with an lt_last_error() text that names the offending argument. */
#ifndef LT_COLLECT_H
#define LT_COLLECT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only: bytes of the state for n envs, rows of d floats and a ring of `depth` rows (= the largest delay + 1 or more; the
 * reference uses max_delay).  n, d, depth >= 1. */
int lt_delay_state_bytes(int64_t n, int64_t d, int64_t depth, size_t* bytes);

/* Resets the envs whose mask byte is non-zero (mask: uint8 / bool [n]; NULL: every env): count = 0, delay = fresh_delays[env] (int64
 * [n], what torch.randint drew).  One lane per env, three ints touched.  A value outside [0, depth) is NOT checked on the device: the
 * caller guarantees it.  One launch. */
int lt_delay_reset(void* state, int64_t n, int64_t d, int64_t depth, const uint8_t* mask_or_null, const int64_t* fresh_delays, void* stream);

/* Pushes rows[n][d] (row r at rows + r * rows_stride) and writes the delayed rows to out0 and, if non-NULL, out1 (row r at
 * out + r * out_stride).  An optional third pair copies copy_src[n][copy_d] to copy_dst (NULL / 0: none; copy_src without copy_dst, or
 * the reverse, is an error): the policy rows go to their store slot in the same launch.  One launch.
 * No destination may overlap an input (rows, copy_src) or the state: the byte ranges the operands span are compared.
 * In place: the slot read is never the slot written (delay < depth) except for min(delay, count - 1) == 0, where the delayed row is
 * the row being pushed and comes from the value just loaded, not from the ring. */
int lt_delay_push(void* state, int64_t n, int64_t d, int64_t depth, const float* rows, int64_t rows_stride, float* out0, int64_t out0_stride,
                  float* out1, int64_t out1_stride, const float* copy_src, int64_t copy_src_stride, float* copy_dst, int64_t copy_dst_stride,
                  int64_t copy_d, void* stream);

/* The delayed rows without a push (the state is only read): out[n][d], row r at out + r * out_stride.  One launch. */
int lt_delay_read(const void* state, int64_t n, int64_t d, int64_t depth, float* out, int64_t out_stride, void* stream);

/* The recording behind an env step, one launch, one lane per env: reward_out[e] = reward[e] (f32 [n], both contiguous),
 * done_mask_out[e] = dones[e] != 0 (dones: int64 [n], the env view's dtype; done_mask_out: uint8 / bool [n] - the tensor a student's
 * pending reset mask can point at), and, when state is non-NULL, the delay-line reset of the finished envs with fresh_delays as in
 * lt_delay_reset.  state NULL: the two copies alone (d, depth and fresh_delays are ignored). */
int lt_collect_after_step(void* state_or_null, int64_t n, int64_t d, int64_t depth, const float* reward, const int64_t* dones,
                          const int64_t* fresh_delays, float* reward_out, uint8_t* done_mask_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_COLLECT_H */
