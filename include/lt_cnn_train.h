/* lt_cnn_train.h - the training form of the student's tactile CNN head (part of the lt_env.h ABI family; LT_ABI_VERSION 21).
 * Semantics: `CNN2dHead` (reference loco_rl/loco_rl/models/cnn_2d.py): nn.Conv2d -> ReLU -> MaxPool2d -> ... -> flatten -> Linear, forward
 * over the n images of a padded batch and the backward pass to every parameter.  Implemented in csrc/lt_cnn_train.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a caller that never trains a student never calls
 * them); locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h (`_abi.CNN_TRAIN_SIGNATURES`).
 * All data pointers are device pointers; everything is stream-ordered: no host synchronisation, no allocation, no host read and no
 * float atomics.  All arithmetic is f32 (exact f32 products, f32 accumulation).
 *   forward:  a row's embedding has the bits lt_student_step's encoder gives it; they depend neither on n nor on the row's place.
 *   backward: the maps are recomputed, not saved.  ReLU passes gradient where the pre-activation is > 0; a max-pool window pays its
 *             FIRST maximum in row-major window order (PyTorch's rule); rows and columns the pool's floor drops get none.  Every sum
 *             has one fixed order that depends on n alone: the same inputs give the same gradient bits on every run. */
#ifndef LT_CNN_TRAIN_H
#define LT_CNN_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_CNN_MAX_CONVS 3   /* = LT_STUDENT_MAX_CONVS */
#define LT_CNN_TILE 8        /* images of one tile = LT_STUDENT_ENV_TILE */
#define LT_CNN_MAX_SLABS 256 /* workgroups of the backward launch: each owns a slab of consecutive tiles */

/* The conv-stack part of lt_student_desc, field for field. */
typedef struct lt_cnn_desc {
  int32_t img_channels, img_height, img_width;  /* a row of x is img_channels * img_height * img_width floats, C x H x W */
  int32_t num_convs;                            /* 1 .. LT_CNN_MAX_CONVS */
  int32_t conv_channels[LT_CNN_MAX_CONVS];  /* output channels */
  int32_t conv_kernel[LT_CNN_MAX_CONVS];    /* square kernels */
  int32_t conv_stride[LT_CNN_MAX_CONVS];    /* the CONFIGURED stride: use_maxpool != 0 -> the conv runs at stride 1 and a max-pool
                                                 * of this size and stride follows its activation (1: none; 2 is the largest served) */
  int32_t conv_padding[LT_CNN_MAX_CONVS];   /* must be 0 */
  int32_t use_maxpool;
  int32_t conv_activation;                      /* lt_activation behind every conv: LT_ACT_RELU is the one served */
  int32_t conv_norm;                            /* 0: no norm layer (the one served) */
  int32_t head_out;                             /* Linear(flattened conv output, head_out), no activation: a multiple of 16 */
} lt_cnn_desc;

/* Device pointers to the module's own parameter tensors, in torch's layouts: conv weight [out][in][k][k], conv bias [out], head weight
 * [head_out][flat], head bias [head_out]. */
typedef struct lt_cnn_params {
  const float* conv_w[LT_CNN_MAX_CONVS];
  const float* conv_b[LT_CNN_MAX_CONVS];
  const float* head_w;
  const float* head_b;
} lt_cnn_params;

/* Where the gradients go: the same shapes and layouts, so they can be the parameters' .grad tensors. */
typedef struct lt_cnn_grads {
  float* conv_w[LT_CNN_MAX_CONVS];
  float* conv_b[LT_CNN_MAX_CONVS];
  float* head_w;
  float* head_b;
} lt_cnn_grads;

/* Host-only (no device is touched): LT_OK if the kernels serve `desc`, else LT_EINVAL with an lt_last_error() text that names the
 * offending field.  The served stacks are those of lt_student_validate (at most LT_STUDENT_MAX_CONVS convolutions, square kernels,
 * padding 0, ReLU, no norm layer, a pool of at most 2, head_out a multiple of 16) whose maps and gradient maps of one tile fit in LDS.
 * Every other entry point below validates the same way first. */
int lt_cnn_validate(const lt_cnn_desc* desc);

/* Floats of the scratch `ws` for n images (16-byte aligned; needs no initialisation): the packed weights and one gradient partial
 * per workgroup of the backward launch.  A scratch sized for n serves every smaller n; lt_cnn_forward touches the packed weights only,
 * so lt_cnn_ws_floats(desc, 1, ..) floats serve it at every n. */
int lt_cnn_ws_floats(const lt_cnn_desc* desc, int64_t n, size_t* floats);

/* emb_out [n][head_out] = the head's output for x [n][C * H * W] (contiguous).  Packs the weights into ws itself.
 * Launches lt_cnn_launches(desc, n, 0) kernels. */
int lt_cnn_forward(const lt_cnn_desc* desc, const lt_cnn_params* params, const float* x, int64_t n, float* emb_out, float* ws, void* stream);

/* grads_out = the gradient of sum(emb * d_emb) with respect to every conv weight and bias and the head weight and bias, for x
 * [n][C * H * W] and d_emb [n][head_out] (both contiguous).  OVERWRITES grads_out (it does not accumulate); there is no input gradient.
 * Packs the weights into ws itself (it does not need the forward's).  Launches lt_cnn_launches(desc, n, 1) kernels. */
int lt_cnn_backward(const lt_cnn_desc* desc, const lt_cnn_params* params, const float* x, const float* d_emb, int64_t n,
                    const lt_cnn_grads* grads_out, float* ws, void* stream);

/* VALUE query: the number of kernel launches one lt_cnn_forward (backward == 0) or lt_cnn_backward (backward != 0) issues - it does not
 * depend on n -, or a negative LT_* code for a descriptor lt_cnn_validate refuses or n < 1.  Host-only. */
int lt_cnn_launches(const lt_cnn_desc* desc, int64_t n, int backward);

#ifdef __cplusplus
}
#endif

#endif /* LT_CNN_TRAIN_H */
