/* lt_encoder.h - the piece in front of an `ActorCriticEncoder`'s actor (and of its critic, when that has an encoder): an encoder MLP on
 * the TAIL columns of an observation row, its embedding concatenated behind the HEAD columns (a unit of the lt_env.h ABI with a header
 * of its own; LT_ABI_VERSION 21).  Reference: loco_rl/loco_rl/modules/actor_critic_encoder.py:85-117.  Implemented in
 * csrc/lt_encoder.hip.
 *
 * Semantics per row r < n and per network:
 *     e      = enc(obs[r, obs_dim - enc_in : obs_dim])     a Linear stack, `activation` behind every layer but the last,
 *                                                           `final_activation` (LT_ACT_NONE: none) behind the last
 *     out[r] = [ obs[r, 0 : flat_dim] | e ]                width flat_dim + embedding_dim, contiguous rows
 * The head columns are copies, bit for bit.  Products are exact f32 (v_mfma_f32_16x16x4_f32), accumulation is f32, and every sum has
 * ONE fixed order that depends on the layer's input width alone (16-wide k blocks in index order dealt to four partial sums, added
 * pairwise, then the bias): the same inputs give the same bits on every run, and a row's bits depend neither on n nor on where the row
 * stands.  Stream-ordered: no allocation, no host read, no float atomics.  Validation is host-side, before anything is launched:
 * LT_EINVAL with an lt_last_error() text "<function>: invalid argument: <field> must be ...".
 *
 * Supported: f32 rows; 1 to LT_ENCODER_MAX_LAYERS (= LT_MLP_MAX_LAYERS) layers; hidden and embedding widths that are multiples of 8
 * and at most LT_ENCODER_MAX_WIDTH; 1 <= enc_in <= LT_ENCODER_MAX_WIDTH, enc_in <= obs_dim, 0 <= flat_dim <= obs_dim; `activation` one
 * of LT_ACT_ELU, LT_ACT_RELU, LT_ACT_TANH (lt_env.h `lt_activation`), `final_activation` one of those or LT_ACT_NONE;
 * 1 <= n <= 16 * 65535. */
#ifndef LT_ENCODER_H
#define LT_ENCODER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_ENCODER_MAX_LAYERS 6
#define LT_ENCODER_MAX_WIDTH 512

typedef struct lt_encoder_desc {
  int32_t obs_dim;                      /* columns of an observation row */
  int32_t flat_dim;                     /* head columns copied to the output */
  int32_t enc_in;                       /* tail columns the encoder reads */
  int32_t num_layers;
  int32_t dims[LT_ENCODER_MAX_LAYERS];  /* outputs of layer l; dims[num_layers - 1] is the embedding width */
  int32_t activation;
  int32_t final_activation;
} lt_encoder_desc;

/* One network's operands.  All pointers are device pointers to f32, 4-byte aligned (the tail at column 270 of a 348-wide row is only
 * 8-byte aligned, and the parameters may be views of a flat bucket).
 *   obs         rows read in place, row r at obs + r * obs_stride floats (obs_stride >= obs_dim): a storage slot during the rollout,
 *               gathered minibatch rows during the update
 *   weight[l]   [dims[l]][dims[l - 1]] (layer 0: [dims[0]][enc_in]), torch's layout; bias[l] [dims[l]]
 *   out         [n][flat_dim + embedding width]; must not overlap obs
 *   acts[l]     all NULL: the inference form.  All of the first num_layers - 1 given: the training form - acts[l] [n][dims[l]] receives
 *               the activation behind hidden layer l, f32 and unsplit, the very values the next layer reads; with a final activation
 *               acts[num_layers - 1] [n][embedding width] must be given too and receives the PRE-activation embedding. */
typedef struct lt_encoder_net {
  lt_encoder_desc desc;
  const float* obs;
  int64_t obs_stride;
  const float* weight[LT_ENCODER_MAX_LAYERS];
  const float* bias[LT_ENCODER_MAX_LAYERS];
  float* out;
  float* acts[LT_ENCODER_MAX_LAYERS];
} lt_encoder_net;

/* Host only: LT_OK for a descriptor the kernel serves, else LT_EINVAL naming the field. */
int lt_encoder_validate(const lt_encoder_desc* desc);

/* ONE launch: the rows above for `actor` and, when non-NULL, `critic` (a grid dimension selects the network). */
int lt_encoder_forward(const lt_encoder_net* actor, const lt_encoder_net* critic, int n, void* stream);

/* Kernel launches of lt_encoder_forward for these descriptors (critic may be NULL): 1, or the negative LT_* code of a refused one. */
int lt_encoder_forward_launches(const lt_encoder_desc* actor, const lt_encoder_desc* critic);

#ifdef __cplusplus
}
#endif

#endif /* LT_ENCODER_H */
