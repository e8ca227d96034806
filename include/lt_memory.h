/* lt_memory.h - one ROLLOUT step of the two LSTM memories of a recurrent policy (`ActorCriticRecurrent`: `memory_a` in front of the
 * actor, `memory_c` in front of the critic) in one launch (part of the lt_env.h ABI, which includes this file; LT_ABI_VERSION 21).
 * lt_lstm.h serves the UPDATE's shape (B around 47 trajectories, many steps); this file serves the rollout's: one step, B = num_envs
 * rows, K = I + H with I the observation width, two networks at once.  Implemented in csrc/lt_memory.hip.
 *
 * Semantics per network, step t of a rollout (reference loco_rl/loco_rl/algorithms/ppo.py:130-131 `act`, :170 `reset(dones)`):
 *     (h, c)   = where(dones[t-1], 0, raw state step t-1 left)          `PolicyMemory.reset(dones)`, applied where the operand is loaded
 *     saved[t] = (h, c)                                                   the state BEFORE the step, what the update starts trajectories from
 *     a = x_t W_ih^T + b_ih + h W_hh^T + b_hh;  i, f, o = sigmoid(a_i, a_f, a_o);  g = tanh(a_g)      PyTorch's gate order (i, f, g, o)
 *     c' = f * c + i * g;  h' = o * tanh(c')                              the new RAW state, written to ANOTHER buffer than the one read
 * Products are exact f32 (v_mfma_f32_16x16x4_f32), accumulation is f32, every sum has ONE fixed order that depends on the sizes alone:
 * the same inputs give the same bits on every run.  Stream-ordered: no allocation, no host read, no float atomics.  Validation is
 * host-side, before anything is launched: LT_EINVAL with an lt_last_error() text "<function>: invalid argument: <field> must be ...".
 *
 * Supported: a single-layer LSTM with biases, f32, H a multiple of 64 with 64 <= H <= 512, I >= 1 with I + H <= 1248 (a workgroup
 * keeps its weight panel, 32 gate rows x (I + H), in LDS), 1 <= N <= 16 * 65535. */
#ifndef LT_MEMORY_H
#define LT_MEMORY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One memory's operands of one step.  All pointers are device pointers to contiguous f32.  16-byte aligned: w_hh [4H][H], b_ih, b_hh
 * [4H], h_in, c_in, h_out, c_out [N][H], saved_h, saved_c [N][H] (slot t of a [T][1][N][H] array).  4-byte aligned: x [N][I] (the
 * observation rows of slot t; I need not be a multiple of 4) and w_ih [4H][I].  h_out / c_out must not overlap h_in / c_in of either
 * network: other workgroups of the same launch still read those (the ping-pong of the caller). */
typedef struct lt_memory_net {
  const float* x;
  int I;
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* h_in;
  const float* c_in;
  float* h_out;
  float* c_out;
  float* saved_h;
  float* saved_c;
} lt_memory_net;

/* ONE launch: the step above for `actor` and `critic` (a grid dimension selects the network).  dones: uint8 [N] of the PREVIOUS step, or
 * NULL (t = 0: the state is taken as it is).  Every element of h_out, c_out, saved_h and saved_c of both networks is written. */
int lt_memory_step(const lt_memory_net* actor, const lt_memory_net* critic, const uint8_t* dones, int N, int H, void* stream);

/* ONE small launch behind the last env step: out = where(dones, 0, raw) for the four state arrays [N][H] of both networks (dones: uint8
 * [N] of the LAST step, NULL = a plain copy) - the state a following eager step, `compute_returns` or a checkpoint sees. */
int lt_memory_finish(const float* h_a, const float* c_a, const float* h_c, const float* c_c, const uint8_t* dones, int N, int H,
                     float* out_h_a, float* out_c_a, float* out_h_c, float* out_c_c, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_MEMORY_H */
