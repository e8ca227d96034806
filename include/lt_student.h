/* lt_student.h - one fused inference step of the deployed student policy (part of the lt_env.h ABI, which includes this file;
 * LT_ABI_VERSION 21).  Semantics: `Student.forward` on one env step (reference locotouch/distill/student.py:40-60 with
 * loco_rl/loco_rl/models/{cnn_2d,rnn,memory_module,mlp}.py): tactile image -> conv stack (+ max-pool) -> Linear head -> one GRU cell
 * -> ELU MLP -> concatenation with the proprioception -> ELU MLP -> actions.  Implemented in csrc/lt_student.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a caller that never runs a student never calls
 * them); locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h (`_abi.STUDENT_SIGNATURES`).
 * All data pointers are device pointers; everything is stream-ordered: no host synchronisation, no allocation, no host read and no
 * float atomics (every sum has one fixed order: same bits every run, and a row's bits depend neither on n nor on where in the batch
 * the row stands).  All arithmetic is f32 (exact f32 products, f32 accumulation): no input domain beyond f32's own. */
#ifndef LT_STUDENT_H
#define LT_STUDENT_H

#include <stddef.h>
#include <stdint.h>

#include "lt_env.h" /* lt_mlp_desc, lt_activation, lt_row_format, LT_* status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define LT_STUDENT_MAX_CONVS 3
#define LT_STUDENT_MAX_MLP_LAYERS 6 /* = LT_MLP_MAX_LAYERS */
#define LT_STUDENT_ROW_TILE 16      /* rows of one workgroup of the GRU / MLP launches */
#define LT_STUDENT_ENV_TILE 8       /* rows of one workgroup of the tactile-encoder launch */
#define LT_STUDENT_GRU_TILE 64      /* hidden units of one workgroup of the GRU launch: rnn_hidden must be a multiple */

enum lt_student_rnn { LT_STUDENT_RNN_GRU = 0, LT_STUDENT_RNN_LSTM = 1 };

/* The architecture.  `Student` of the registered task: img 2 x 17 x 13, convs 24/24/24 with kernels 4/3/2 and configured strides
 * 2/1/1, use_maxpool, head_out 64, GRU 512, encoder 512-256-128-64-64, proprio_dim 270, backbone 334-512-256-128-12. */
typedef struct lt_student_desc {
  int32_t img_channels, img_height, img_width;  /* the tactile row is img_channels * img_height * img_width floats, C x H x W */
  int32_t num_convs;                            /* 1 .. LT_STUDENT_MAX_CONVS */
  int32_t conv_channels[LT_STUDENT_MAX_CONVS];  /* output channels */
  int32_t conv_kernel[LT_STUDENT_MAX_CONVS];    /* square kernels */
  int32_t conv_stride[LT_STUDENT_MAX_CONVS];    /* the CONFIGURED stride: use_maxpool != 0 -> the conv runs at stride 1 and a max-pool
                                                 * of this size and stride follows its activation (1: none; 2 is the largest served) */
  int32_t conv_padding[LT_STUDENT_MAX_CONVS];   /* must be 0 */
  int32_t use_maxpool;
  int32_t conv_activation;                      /* lt_activation behind every conv: LT_ACT_RELU is the one served */
  int32_t conv_norm;                            /* 0: no norm layer (the one served) */
  int32_t head_out;                             /* Linear(flattened conv output, head_out), no activation: a multiple of 16 */
  int32_t rnn_type;                             /* lt_student_rnn: LT_STUDENT_RNN_GRU is the one served */
  int32_t rnn_layers;                           /* must be 1 */
  int32_t rnn_hidden;                           /* a multiple of LT_STUDENT_GRU_TILE, <= 512 */
  lt_mlp_desc encoder;                          /* dims[0] = rnn_hidden; LT_ACT_ELU; LT_ROWS_F32 */
  lt_mlp_desc backbone;                         /* dims[0] = proprio_dim + encoder output; LT_ACT_ELU; LT_ROWS_F32; inputs <= 512 */
  int32_t proprio_dim;                          /* >= 0 */
} lt_student_desc;

/* Device pointers to the module's own parameter tensors, in torch's layouts: conv weight [out][in][k][k], Linear weight [out][in],
 * GRU weight_ih_l0 [3H][head_out], weight_hh_l0 [3H][H], bias_ih_l0 / bias_hh_l0 [3H] (gate order r, z, n). */
typedef struct lt_student_params {
  const float* conv_w[LT_STUDENT_MAX_CONVS];
  const float* conv_b[LT_STUDENT_MAX_CONVS];
  const float* head_w;
  const float* head_b;
  const float* gru_w_ih;
  const float* gru_w_hh;
  const float* gru_b_ih;
  const float* gru_b_hh;
  const float* enc_w[LT_STUDENT_MAX_MLP_LAYERS];
  const float* enc_b[LT_STUDENT_MAX_MLP_LAYERS];
  const float* bb_w[LT_STUDENT_MAX_MLP_LAYERS];
  const float* bb_b[LT_STUDENT_MAX_MLP_LAYERS];
} lt_student_params;

/* Host-only (no device is touched): LT_OK if the kernels serve `desc`, else LT_EINVAL with an lt_last_error() text that names the
 * offending field (rnn_type, rnn_layers, conv_norm, conv_padding, conv_activation, conv_stride, encoder / backbone with the member,
 * rnn_hidden, head_out, input_format for bf16 rows, ...).  Every other entry point below validates the same way first. */
int lt_student_validate(const lt_student_desc* desc);

/* Floats of the packed parameter buffer (16-byte aligned device memory). */
int lt_student_packed_floats(const lt_student_desc* desc, size_t* floats);
/* Packs the parameters into the layout the kernels walk: convolution and head weights transposed (the output channel runs fastest),
 * [W_ih | W_hh] side by side per gate row, every MLP matrix zero-padded to multiples of 16 in both directions.  ONE launch on
 * `stream`, no host read: call it again after every optimizer step that changed the module. */
int lt_student_pack(const lt_student_desc* desc, const lt_student_params* params, float* packed, void* stream);

/* Floats of the scratch `ws` of lt_student_step for n rows (16-byte aligned; needs no initialisation). */
int lt_student_ws_floats(const lt_student_desc* desc, int64_t n, size_t* floats);

/* One env step of the student for n rows.
 * proprio: row r is the proprio_dim floats at proprio + r * proprio_row_stride (floats): the leading columns of the env's policy rows
 *   are read in place.  tactile: row r is the image at tactile + r * tactile_row_stride.
 * done_mask (uint8 / bool [n], or NULL): a row whose byte is non-zero starts from a ZERO hidden state - the reset after the previous
 *   step's `dones`, folded into this step.
 * h [n][rnn_hidden]: the hidden state, replaced IN PLACE by the new one.  actions_out [n][backbone output].
 * Launches lt_student_step_launches(desc, n) kernels. */
int lt_student_step(const lt_student_desc* desc, const float* packed, const float* proprio, int64_t proprio_row_stride, const float* tactile,
                    int64_t tactile_row_stride, const uint8_t* done_mask, float* h, int64_t n, float* actions_out, float* ws, void* stream);

/* VALUE query: the number of kernel launches one lt_student_step(desc, ..., n, ...) issues (<= 4), or a negative LT_* code for a
 * descriptor lt_student_validate refuses.  Host-only. */
int lt_student_step_launches(const lt_student_desc* desc, int64_t n);

#ifdef __cplusplus
}
#endif

#endif /* LT_STUDENT_H */
