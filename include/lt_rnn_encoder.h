/* lt_rnn_encoder.h - the two pieces in front of an `ActorCriticRNNEncoder`'s stacks during a rollout (a unit of the lt_env.h ABI with a
 * header of its own; LT_ABI_VERSION 21).  Reference: loco_rl/loco_rl/modules/actor_critic_rnn_encoder.py:110-145: the TAIL columns of an
 * observation row go through a memory (GRU or LSTM), the memory's output through an encoder MLP, and the embedding is concatenated behind
 * the HEAD columns of the row.  Both pieces are the kernels of lt_memory.h / lt_memory_gru.h and of lt_encoder.h with ONE operand read
 * from another place; nothing of those headers changes.  Implemented in csrc/lt_memory.hip, csrc/lt_memory_gru.hip (the step) and
 * csrc/lt_encoder.hip (the encoder).
 *
 * a. The memory step on STRIDED rows: lt_memory_step / lt_memory_gru_step with each network's x rows read in place at
 *    x + r * x_stride floats (x_stride >= I) - the tail columns of a storage slot.  Everything else is as lt_memory.h and lt_memory_gru.h
 *    state it: the reset mask applied where the operand is loaded, the pre-step state into the saved slot, the new raw state into the
 *    other ping-pong buffer, and the same sums in the same order - with x_stride == I the launch IS the contiguous one, and on any
 *    stride the bits are those of the contiguous step on a contiguous copy of the rows.  x is 4-byte aligned (the tail at column 270 of
 *    a 348-wide row is only 8-byte aligned); 16-byte loads are used where x, I and x_stride all allow them, which moves no sum.
 *    lt_memory_finish / lt_memory_gru_finish close a rollout as ever.
 *
 * b. The encoder on a SECOND array: per row r < n and per network
 *        out[r] = [ obs[r, 0 : flat_dim] | enc(h[r, 0 : enc_in]) ]
 *    with enc the Linear stack of lt_encoder.h (same layers, same sums: a sum's order depends on the layer's input width alone, so
 *    `out` equals lt_encoder_forward on rows [obs[r, :flat_dim] | h[r]] bit for bit).  Inference form only.
 *
 * Stream-ordered: no allocation, no host read, no float atomics.  Validation is host-side, before anything is launched: LT_EINVAL with
 * an lt_last_error() text "<function>: invalid argument: <field> must be ...". */
#ifndef LT_RNN_ENCODER_H
#define LT_RNN_ENCODER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_RNN_ENCODER_MAX_LAYERS 6 /* = LT_ENCODER_MAX_LAYERS */

/* One memory's operands of one step: the fields of lt_memory_net / lt_memory_gru_net and the row stride of x.  All pointers are device
 * pointers to f32.  16-byte aligned and contiguous: w_hh, b_ih, b_hh, the state arrays [N][H].  4-byte aligned: x (row r at
 * x + r * x_stride floats, I columns read) and w_ih [gates * H][I].  LSTM (lt_memory_step_strided): all of c_in, c_out, saved_c are
 * given.  GRU (lt_memory_gru_step_strided): all three are NULL.  h_out / c_out must be other buffers than h_in / c_in. */
typedef struct lt_rnn_encoder_memory {
  const float* x;
  int64_t x_stride;
  int32_t I;
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
} lt_rnn_encoder_memory;

/* ONE launch each: lt_memory_step / lt_memory_gru_step on strided x rows.  dones: uint8 [N] of the PREVIOUS step, or NULL.  Sizes as in
 * lt_memory.h: H a multiple of 64 in [64, 512], I >= 1 with I + H <= 1248, 1 <= N <= 16 * 65535. */
int lt_memory_step_strided(const lt_rnn_encoder_memory* actor, const lt_rnn_encoder_memory* critic, const uint8_t* dones, int N, int H,
                           void* stream);
int lt_memory_gru_step_strided(const lt_rnn_encoder_memory* actor, const lt_rnn_encoder_memory* critic, const uint8_t* dones, int N, int H,
                               void* stream);

/* One network's encoder and operands.  The widths are lt_encoder_desc's with enc_in the columns of an h row (the memory's hidden
 * size): 1 <= enc_in <= 512, 0 <= flat_dim <= obs_dim, 1 to LT_RNN_ENCODER_MAX_LAYERS layers of widths that are multiples of 8 and at
 * most 512, `activation` LT_ACT_ELU / LT_ACT_RELU / LT_ACT_TANH, `final_activation` one of those or LT_ACT_NONE.
 *   obs         4-byte aligned, row r at obs + r * obs_stride floats (obs_stride >= obs_dim >= 1); only the head columns are read
 *   h           16-byte aligned, row r at h + r * h_stride floats (h_stride >= enc_in, a multiple of 4)
 *   weight[l]   [dims[l]][dims[l - 1]] (layer 0: [dims[0]][enc_in]), bias[l] [dims[l]]: 4-byte aligned
 *   out         [n][flat_dim + embedding width], 4-byte aligned; must overlap neither obs nor h
 *   acts[l]     all NULL: this launch has the inference form alone */
typedef struct lt_rnn_encoder_net {
  int32_t obs_dim;
  int32_t flat_dim;
  int32_t enc_in;
  int32_t num_layers;
  int32_t dims[LT_RNN_ENCODER_MAX_LAYERS];
  int32_t activation;
  int32_t final_activation;
  const float* obs;
  int64_t obs_stride;
  const float* h;
  int64_t h_stride;
  const float* weight[LT_RNN_ENCODER_MAX_LAYERS];
  const float* bias[LT_RNN_ENCODER_MAX_LAYERS];
  float* out;
  float* acts[LT_RNN_ENCODER_MAX_LAYERS];
} lt_rnn_encoder_net;

/* ONE launch: the rows of b. for `actor` and, when non-NULL, `critic` (a grid dimension selects the network). */
int lt_rnn_encoder_forward(const lt_rnn_encoder_net* actor, const lt_rnn_encoder_net* critic, int n, void* stream);

/* Kernel launches of lt_rnn_encoder_forward for these networks' widths (critic may be NULL; pointers are not looked at): 1, or the
 * negative LT_* code of a refused one. */
int lt_rnn_encoder_forward_launches(const lt_rnn_encoder_net* actor, const lt_rnn_encoder_net* critic);

#ifdef __cplusplus
}
#endif

#endif /* LT_RNN_ENCODER_H */
