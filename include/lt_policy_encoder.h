/* lt_policy_encoder.h - one INFERENCE step of a trained encoder policy: `ActorCriticRNNEncoder.act_inference` (reference
 * loco_rl/loco_rl/modules/actor_critic_rnn_encoder.py:110-128) or `ActorCriticEncoder.act_inference`
 * (loco_rl/loco_rl/modules/actor_critic_encoder.py:85-100), with the runner's observation normaliser in front: what play, evaluation and
 * a deployment loop run per env step.  A header of its own, NOT included by lt_env.h: one optional unit (the opt-in
 * `rl/fused_policy.py::FusedEncoderPolicy` alone calls it); locotouch_amd/_abi.py binds it by one row of its table
 * (`_abi.POLICY_ENCODER_SIGNATURES`).  LT_ABI_VERSION stays 21.  Implemented in csrc/lt_policy_encoder.hip.
 *
 * Semantics of one step, per row r < n, with x = obs[r], or (obs[r] - norm_mean) / (norm_std + norm_eps) over the WHOLE row
 * (`EmpiricalNormalization` in evaluation mode, as lt_policy.h states it):
 *   RNN form (rnn_type LT_POLICY_RNN_LSTM / LT_POLICY_RNN_GRU), TWO launches on `stream`:
 *     (h, c)   = where(done_mask[r], 0, (h_in[r], c_in[r]))      `reset(dones)` behind the previous step, folded into this one
 *     (h', c') = cell(x[obs_dim - tail_dim :], h, c)  ->  h_out[r], c_out[r]
 *     e        = encoder(h')                                     a Linear stack as lt_encoder.h's, enc_in = rnn_hidden
 *     a        = actor([ x[: flat_dim] | e ])  ->  actions_out[r]      the mean action, no sampling
 *   plain form (rnn_type LT_POLICY_ENCODER_NO_MEMORY), ONE launch:
 *     e = encoder(x[obs_dim - tail_dim :]);  a = actor([ x[: flat_dim] | e ])
 *
 * Launch 1 of the RNN form is lt_policy.h's memory step (lt_policy_memory_kernel) on the tail columns of the rows and the tail slices of
 * the statistics: h_out / c_out are bit for bit what lt_policy_step writes on those operands, and without a normaliser what
 * lt_memory_step_strided / lt_memory_gru_step_strided (lt_rnn_encoder.h) write for their actor network.
 *
 * The other launch (lt_policy_encoder_kernel) runs head normalisation, encoder, concatenation and actor for a row block whose
 * activations never leave LDS, on the plan and with the arithmetic of lt_encoder.h's kernel: exact f32 products
 * (v_mfma_f32_16x16x4_f32), f32 accumulation, k blocks of 16 in index order dealt to four partial sums that are added pairwise, then the
 * bias.  The encoder layers keep that kernel's sums: the embedding is bit for bit the embedding columns of lt_rnn_encoder_forward (RNN
 * form, on h_out) or lt_encoder_forward (plain form, on the normalised rows).  The actor layers sum over their input columns in torch's
 * order, [head | embedding], by the same rule.  A row's bits depend on the row and the parameters alone: neither on n, nor on the row's
 * place in the batch, nor on the row-block and panel heights the host picks.  All parameters are read live, in torch's layouts; nothing
 * is packed.  Stream-ordered: no allocation, no host read, no float atomics.  Validation is host-side, before anything is launched:
 * LT_EINVAL with an lt_last_error() text "<function>: invalid argument: <field> must be ...".
 *
 * Supported: f32 rows, the inference form.  Memory as lt_policy.h: one layer, rnn_hidden a multiple of 64 in [64, 512],
 * tail_dim + rnn_hidden <= 1248.  Encoder as lt_encoder.h / lt_rnn_encoder.h: 1 to LT_POLICY_ENCODER_MAX_LAYERS layers, widths
 * multiples of 8 in [8, 512], input width (rnn_hidden, or tail_dim in the plain form) in [1, 512], hidden activation ELU / ReLU / tanh,
 * final activation one of those or none.  Actor: 1 to LT_POLICY_ENCODER_MAX_LAYERS layers, hidden widths multiples of 8 in [8, 512], an
 * output width (the action count) of 1 to 512, hidden activation ELU / ReLU / tanh, none behind the last layer.  The actor's input,
 * flat_dim + embedding width, is at most LT_POLICY_ENCODER_MAX_ACTOR_IN = 1008 columns: what the 160 KiB of LDS hold at the smallest
 * row block and panel (16 rows each: two activation buffers of 1008 + 8 and 512 + 8 floats a row, a panel of 1008 + 8).
 * 0 <= flat_dim <= obs_dim, 1 <= tail_dim <= obs_dim, 1 <= n <= 16 * 65535. */
#ifndef LT_POLICY_ENCODER_H
#define LT_POLICY_ENCODER_H

#include <stdint.h>

#include "lt_policy.h" /* lt_policy_rnn; through it lt_env.h: lt_activation, LT_* status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define LT_POLICY_ENCODER_MAX_LAYERS 6 /* = LT_ENCODER_MAX_LAYERS = LT_MLP_MAX_LAYERS */
#define LT_POLICY_ENCODER_MAX_ACTOR_IN 1008
#define LT_POLICY_ENCODER_NO_MEMORY (-1) /* rnn_type of the plain form */

typedef struct lt_policy_encoder_desc {
  int32_t rnn_type;             /* lt_policy_rnn, or LT_POLICY_ENCODER_NO_MEMORY */
  int32_t rnn_layers;           /* 1 (0 in the plain form) */
  int32_t rnn_hidden;           /* H: a multiple of 64, 64 <= H <= 512 (0 in the plain form) */
  int32_t obs_dim;              /* columns of an observation row */
  int32_t flat_dim;             /* head columns the actor reads */
  int32_t tail_dim;             /* tail columns the memory (RNN form) or the encoder (plain form) reads */
  int32_t enc_layers;
  int32_t enc_dims[LT_POLICY_ENCODER_MAX_LAYERS];   /* outputs of encoder layer l; enc_dims[enc_layers - 1] is the embedding width E */
  int32_t enc_activation;       /* lt_activation behind every encoder layer but the last */
  int32_t enc_final_activation; /* lt_activation behind the last (LT_ACT_NONE: none) */
  int32_t actor_layers;
  int32_t actor_dims[LT_POLICY_ENCODER_MAX_LAYERS]; /* outputs of actor layer l; the last is the action count A */
  int32_t actor_activation;     /* lt_activation between the actor's layers (none behind the last) */
} lt_policy_encoder_desc;

/* The parameters: device pointers to contiguous f32 in torch's layouts.  The memory's as lt_policy_memory (w_ih [gates * H][tail_dim],
 * 4-byte aligned; w_hh, b_ih, b_hh 16-byte aligned), all four NULL in the plain form.  enc_weight[l] [enc_dims[l]][its input width],
 * enc_bias[l] [enc_dims[l]], actor_weight[l] (layer 0: [actor_dims[0]][flat_dim + E]), actor_bias[l]: 4-byte aligned; entries behind
 * the layer counts are not looked at.  norm_mean, norm_std [obs_dim], 4-byte aligned: both NULL (the rows are taken as they are) or
 * both set. */
typedef struct lt_policy_encoder_params {
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* enc_weight[LT_POLICY_ENCODER_MAX_LAYERS];
  const float* enc_bias[LT_POLICY_ENCODER_MAX_LAYERS];
  const float* actor_weight[LT_POLICY_ENCODER_MAX_LAYERS];
  const float* actor_bias[LT_POLICY_ENCODER_MAX_LAYERS];
  const float* norm_mean;
  const float* norm_std;
  float norm_eps;
} lt_policy_encoder_params;

/* Host-only (no device is touched): LT_OK if the kernels serve `desc`, else LT_EINVAL naming the refused field. */
int lt_policy_encoder_validate(const lt_policy_encoder_desc* desc);

/* One step for n rows.
 * obs: row r is the obs_dim floats at obs + r * obs_row_stride (floats, >= obs_dim), 4-byte aligned: the env's policy rows, or a column
 *   slice of wider rows, are read in place.
 * done_mask: uint8 / bool [n] or NULL (the state is taken as it is); NULL in the plain form.
 * h_in, h_out [n][H], 16-byte aligned; c_in, c_out likewise for an LSTM, NULL for a GRU; all four NULL in the plain form.  h_out / c_out
 *   must not overlap h_in / c_in (the caller ping-pongs, as with lt_policy_step).
 * actions_out [n][A]; embedding_out NULL or [n][E]: 4-byte aligned, every element is written.  No output may overlap obs or another
 *   output. */
int lt_policy_encoder_step(const lt_policy_encoder_desc* desc, const lt_policy_encoder_params* params, const float* obs,
                           int64_t obs_row_stride, const uint8_t* done_mask, const float* h_in, const float* c_in, float* h_out,
                           float* c_out, int64_t n, float* actions_out, float* embedding_out, void* stream);

/* A VALUE, not a status: the number of kernel launches one lt_policy_encoder_step(desc, ..., n, ...) issues - 2 with a memory, 1
 * without -, or a negative LT_* code for a descriptor lt_policy_encoder_validate refuses or an n lt_policy_encoder_step refuses.
 * Host-only. */
int lt_policy_encoder_step_launches(const lt_policy_encoder_desc* desc, int64_t n);

#ifdef __cplusplus
}
#endif

#endif /* LT_POLICY_ENCODER_H */
