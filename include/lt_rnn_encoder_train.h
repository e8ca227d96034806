/* lt_rnn_encoder_train.h - the encoder of an `ActorCriticRNNEncoder` during the PPO update (a unit of the lt_env.h ABI with a header of
 * its own; LT_ABI_VERSION 21): the training form of lt_rnn_encoder.h's launch, and the backward pass from the gradient w.r.t. the rows
 * the stacks read to the gradient w.r.t. the memory's output.  Nothing of lt_rnn_encoder.h or lt_encoder.h changes.  Implemented in
 * csrc/lt_encoder.hip.
 *
 * a. lt_rnn_encoder_forward_train: lt_rnn_encoder_forward with the training form of lt_encoder.h - acts[l] [n][dims[l]] receives the
 *    activation behind hidden layer l, and with a final activation acts[num_layers - 1] receives the PRE-activation embedding.  The same
 *    kernel, the same sums: `out` equals lt_rnn_encoder_forward's bit for bit, `acts` those of lt_encoder_forward on rows
 *    [obs[r, :flat_dim] | h[r]].
 *
 * b. lt_rnn_encoder_backward: per row r < n and per network, with E = dims[L - 1], W_l the weight of layer l ([dims[l]][dims[l - 1]],
 *    layer 0: [dims[0]][enc_in]) and f the final activation,
 *        g        = dx[r, flat_dim : flat_dim + E]                      read in place, rows dx_stride floats apart
 *        dz_{L-1} = g * f'                                              NONE: g;  TANH: 1 - emb^2, emb = out[r, flat_dim + .];
 *                                                                       ELU: pre > 0 ? 1 : exp(pre);  RELU: pre > 0, pre = acts[L - 1]
 *        da_{l-1} = dz_l W_l,  dz_{l-1} = da_{l-1} * act'(acts[l - 1])  l = L - 1 .. 1, from the stored OUTPUTS a of the activation:
 *                                                                       ELU: a > 0 ? 1 : a + 1;  RELU: a > 0;  TANH: 1 - a^2
 *        dh       = dz_0 W_0                                            [n][enc_in]: the `dout` of lt_memory_seq_backward /
 *                                                                       lt_memory_gru_seq_backward
 *    Every dz_l is written as [n][dims[l]] (dW_l = dz_l^T in_l and db_l = column sums of dz_l are the caller's).  Products are exact
 *    f32 (v_mfma_f32_16x16x4_f32), accumulation is f32, and every sum has ONE fixed order that depends on the layer's widths alone
 *    (16-wide blocks of the summed index in order, dealt to four partial sums that are added pairwise): the same inputs give the same
 *    bits on every run, and a row's bits depend neither on n nor on where the row stands.
 *
 * Stream-ordered: no allocation, no host read, no float atomics.  Validation is host-side, before anything is launched: LT_EINVAL with
 * an lt_last_error() text "<function>: invalid argument: <field> must be ...".  Limits as lt_rnn_encoder_net: 1 to
 * LT_RNN_ENCODER_MAX_LAYERS layers, widths that are multiples of 8 and at most 512, 1 <= enc_in <= 512, 1 <= n <= 16 * 65535. */
#ifndef LT_RNN_ENCODER_TRAIN_H
#define LT_RNN_ENCODER_TRAIN_H

#include <stdint.h>

#include "lt_rnn_encoder.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LT_RNN_ENCODER_TRAIN_MAX_LAYERS 6 /* = LT_RNN_ENCODER_MAX_LAYERS */

/* ONE launch: lt_rnn_encoder_forward in the training form.  acts of each network: all of the first num_layers - 1 and, with a final
 * activation, acts[num_layers - 1] too (4-byte aligned, [n][dims[l]]); every other entry NULL. */
int lt_rnn_encoder_forward_train(const lt_rnn_encoder_net* actor, const lt_rnn_encoder_net* critic, int n, void* stream);

/* One network's operands of the backward pass.  All pointers are device pointers to f32, 4-byte aligned unless noted.
 *   dx          rows read in place, row r at dx + r * dx_stride floats (dx_stride >= flat_dim + dims[num_layers - 1])
 *   out         [n][flat_dim + embedding width], what the forward launch wrote; read (and asked for) with LT_ACT_TANH as the final
 *               activation only
 *   weight[l]   as lt_rnn_encoder_net
 *   acts[l]     as the training form left them: the first num_layers - 1, and acts[num_layers - 1] with a final activation (read with
 *               LT_ACT_ELU / LT_ACT_RELU; asked for with LT_ACT_TANH as well, so that the forward's arrays pass as they are)
 *   dz[l]       OUT [n][dims[l]], l < num_layers
 *   dh          OUT [n][enc_in], 16-byte aligned
 * An output of a network must overlap neither its dx, out, any of its acts or weights, nor another of its outputs (all refused by
 * name); keeping the two networks' arrays apart is the caller's. */
typedef struct lt_rnn_encoder_grad {
  int32_t flat_dim;
  int32_t enc_in;
  int32_t num_layers;
  int32_t dims[LT_RNN_ENCODER_TRAIN_MAX_LAYERS];
  int32_t activation;
  int32_t final_activation;
  const float* dx;
  int64_t dx_stride;
  const float* out;
  const float* weight[LT_RNN_ENCODER_TRAIN_MAX_LAYERS];
  const float* acts[LT_RNN_ENCODER_TRAIN_MAX_LAYERS];
  float* dz[LT_RNN_ENCODER_TRAIN_MAX_LAYERS];
  float* dh;
} lt_rnn_encoder_grad;

/* ONE launch: the rows of b. for `actor` and, when non-NULL, `critic` (a grid dimension selects the network). */
int lt_rnn_encoder_backward(const lt_rnn_encoder_grad* actor, const lt_rnn_encoder_grad* critic, int n, void* stream);

/* Kernel launches of lt_rnn_encoder_backward for these networks' widths (critic may be NULL; pointers are not looked at): 1, or the
 * negative LT_* code of a refused one. */
int lt_rnn_encoder_backward_launches(const lt_rnn_encoder_grad* actor, const lt_rnn_encoder_grad* critic);

#ifdef __cplusplus
}
#endif

#endif /* LT_RNN_ENCODER_TRAIN_H */
