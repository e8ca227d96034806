/* lt_policy.h - one INFERENCE step of a trained recurrent policy (`ActorCriticRecurrent.act_inference`, reference
 * loco_rl/loco_rl/modules/actor_critic_recurrent.py:40-42, with the runner's observation normaliser in front): what play, evaluation and
 * a deployment loop run per env step.  A header of its own, NOT included by lt_env.h: one optional unit (the opt-in
 * `rl/fused_policy.py::FusedRecurrentPolicy` alone calls it); locotouch_amd/_abi.py derives its binding from this file by the same rule
 * as from the other headers (`_abi.POLICY_SIGNATURES`).  LT_ABI_VERSION stays 21.  Implemented in csrc/lt_policy.hip.
 *
 * Semantics of one step, per row r < n:
 *     (h, c) = where(done_mask[r], 0, (h_in[r], c_in[r]))        `reset(dones)` behind the previous step, folded into this one
 *     x      = obs[r], or (obs[r] - norm_mean) / (norm_std + norm_eps)   `EmpiricalNormalization` in evaluation mode
 *     (h', c') = cell(x, h, c)  ->  h_out[r], c_out[r]            the cell of lt_memory.h (LSTM) / lt_memory_gru.h (GRU)
 *     actions_out[r] = actor(h')                                  the mean action, no sampling
 * TWO launches on `stream`: the memory step (lt_policy_memory_kernel) and the actor MLP (lt_mlp_forward's launch on h_out).
 *
 * The memory step keeps the summation order of lt_memory_step / lt_memory_gru_step and shares their gate arithmetic: on the same
 * weights, rows, state and mask, h_out / c_out are bit for bit what those entry points write for their actor network.  Products are
 * exact f32 (v_mfma_f32_16x16x4_f32), accumulation is f32, every sum has ONE fixed order that depends on I and H alone: the same inputs
 * give the same bits on every run, and a row's bits depend neither on n nor on where in the batch the row stands.  Stream-ordered: no
 * allocation, no host read, no float atomics.  Validation is host-side, before anything is launched: LT_EINVAL with an lt_last_error()
 * text "<function>: invalid argument: <field> must be ...". */
#ifndef LT_POLICY_H
#define LT_POLICY_H

#include <stdint.h>

#include "lt_env.h" /* lt_mlp_desc, lt_row_format, LT_* status codes */

#ifdef __cplusplus
extern "C" {
#endif

enum lt_policy_rnn { LT_POLICY_RNN_LSTM = 0, LT_POLICY_RNN_GRU = 1 };

typedef struct lt_policy_desc {
  int32_t rnn_type;   /* lt_policy_rnn */
  int32_t rnn_layers; /* must be 1 */
  int32_t rnn_hidden; /* H: a multiple of 64, 64 <= H <= 512 */
  int32_t obs_dim;    /* I >= 1, I + H <= 1248 (the limit of lt_memory.h) */
  lt_mlp_desc actor;  /* dims[0] == rnn_hidden; what lt_mlp_forward serves, LT_ROWS_F32 */
} lt_policy_desc;

/* The memory's parameters: device pointers to contiguous f32 in torch's layouts and gate orders (LSTM i, f, g, o: w_ih [4H][I], w_hh
 * [4H][H], b_ih, b_hh [4H]; GRU r, z, n: [3H] rows).  4-byte aligned: w_ih (I need not be a multiple of 4), norm_mean, norm_std [I];
 * 16-byte aligned: w_hh, b_ih, b_hh.  norm_mean / norm_std: both NULL (the rows are taken as they are) or both set. */
typedef struct lt_policy_memory {
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* norm_mean;
  const float* norm_std;
  float norm_eps;
} lt_policy_memory;

/* Host-only (no device is touched): LT_OK if the kernels serve `desc`, else LT_EINVAL naming the refused field. */
int lt_policy_validate(const lt_policy_desc* desc);

/* One step for n rows (1 <= n <= 16 * 65535).
 * actor_packed: what lt_mlp_pack produces for desc->actor (16-byte aligned).
 * obs: row r is the obs_dim floats at obs + r * obs_row_stride (floats, >= obs_dim), 4-byte aligned: the env's policy rows, or a column
 *   slice of wider rows, are read in place.
 * done_mask: uint8 / bool [n] or NULL (the state is taken as it is).
 * h_in, h_out [n][H], 16-byte aligned; c_in, c_out likewise for an LSTM and NULL for a GRU.  h_out / c_out must not overlap h_in / c_in:
 *   other workgroups of the launch still read those (the caller ping-pongs, as with lt_memory_step).  Every element of h_out / c_out
 *   and of actions_out [n][actor output] is written. */
int lt_policy_step(const lt_policy_desc* desc, const lt_policy_memory* mem, const float* actor_packed, const float* obs,
                   int64_t obs_row_stride, const uint8_t* done_mask, const float* h_in, const float* c_in, float* h_out, float* c_out,
                   int64_t n, float* actions_out, void* stream);

/* A VALUE, not a status: the number of kernel launches one lt_policy_step(desc, ..., n, ...) issues (2), or a negative LT_* code for
 * a descriptor lt_policy_validate refuses or an n lt_policy_step refuses.  Host-only. */
int lt_policy_step_launches(const lt_policy_desc* desc, int64_t n);

#ifdef __cplusplus
}
#endif

#endif /* LT_POLICY_H */
