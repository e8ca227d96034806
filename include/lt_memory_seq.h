/* lt_memory_seq.h - the two LSTM memories of a recurrent policy over a WHOLE ROLLOUT [T][E] of an env block, forward and backward: the
 * UPDATE's counterpart of lt_memory.h (one rollout step).  A header of its own, NOT included by lt_env.h: one optional unit (the opt-in
 * `fused_recurrent_update` of rl/ppo.py alone calls it); locotouch_amd/_abi.py derives its binding from this file by the same rule as
 * from the other headers (`_abi.MEMORY_SEQ_SIGNATURES`).  LT_ABI_VERSION stays 21.  Implemented in csrc/lt_memory.hip.
 *
 * Why whole rollouts: `PolicyMemory.reset(dones)` zeroes the state of done envs, so the hidden state saved at the first step of a
 * trajectory that starts after a done is all zeros.  The padded batch of trajectories the reference's update runs therefore equals,
 * row for row, ONE pass over the block's envs for all T steps that starts from the state saved at step 0 and replaces the carried (h, c)
 * by zeros wherever dones[t-1] is set - and no gradient crosses a done in either form.
 *
 * Semantics per network, step t (lt_memory.h's step, PyTorch's gate order i, f, g, o):
 *     (h, c)    = t == 0 ? (h0, c0) : where(dones[t-1], 0, (out[t-1], cell[t-1]))       applied where the operand is loaded
 *     h_prev[t], c_prev[t] = (h, c)                                                      what dW_hh and the gate gradients need
 *     a = x_t W_ih^T + b_ih + h W_hh^T + b_hh;  gates[t] = (sigmoid(a_i), sigmoid(a_f), tanh(a_g), sigmoid(a_o))
 *     cell[t] = f * c + i * g;  out[t] = o * tanh(cell[t])
 * Backward, t = T - 1 .. 0 (dgates[T] = 0, the carry dc_T f_T = 0):
 *     dh_t = dout[t] + where(dones[t], 0, dgates[t+1] W_hh)
 *     dc_t = where(dones[t], 0, dc_{t+1} * f_{t+1}) + dh_t * o_t * (1 - tanh^2(cell[t]))
 *     dgates[t] = (dc_t g i (1 - i), dc_t c_prev[t] f (1 - f), dc_t i (1 - g^2), dh_t tanh(cell[t]) o (1 - o))
 * The gradients of (h0, c0) and of x are not computed: the saved states and the observations carry no gradient.  The caller forms
 * dW_hh = dgates^T h_prev, dW_ih = dgates^T X and db_ih = db_hh = the column sums of dgates.
 *
 * Products are exact f32 (v_mfma_f32_16x16x4_f32), accumulation is f32, every sum has ONE fixed order that depends on the sizes alone:
 * the same inputs give the same bits on every run.  Stream-ordered: no allocation, no host read, no float atomics.  Validation is
 * host-side, before anything is launched: LT_EINVAL with an lt_last_error() text "<function>: invalid argument: <field> must be ...".
 *
 * Supported (lt_memory_step's set): a single-layer LSTM with biases, f32, H a multiple of 64 with 64 <= H <= 512, I >= 1 with
 * I + H <= 1248, 1 <= E <= 16 * 65535, T >= 1. */
#ifndef LT_MEMORY_SEQ_H
#define LT_MEMORY_SEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One memory's operands of the forward pass.  Device pointers to f32.  4-byte aligned: x (row e of step t is x + t * x_stride + e * I,
 * I floats: a block [:, e0:e1] of the rollout storage [T][N][I] is read in place with x_stride = N * I) and w_ih [4H][I].  16-byte
 * aligned and contiguous: w_hh [4H][H], b_ih, b_hh [4H], h0, c0 [E][H], out, cell, h_prev, c_prev [T][E][H], gates [T][E][4H].  No
 * output may overlap h0 or c0 of either network (other workgroups of the first launch still read those).  Every element of the five
 * outputs is written. */
typedef struct lt_memory_seq_net {
  const float* x;
  int64_t x_stride;
  int I;
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* h0;
  const float* c0;
  float* out;
  float* cell;
  float* gates;
  float* h_prev;
  float* c_prev;
} lt_memory_seq_net;

/* T launches, both networks in each (a grid dimension selects the network).  dones: uint8, row t at dones + t * dones_stride, E bytes
 * (dones_stride >= E), or NULL (no reset anywhere); the mask of step t is row t - 1, step 0 takes (h0, c0) as given. */
int lt_memory_seq_forward(const lt_memory_seq_net* actor, const lt_memory_seq_net* critic, const uint8_t* dones, int64_t dones_stride,
                          int T, int E, int H, void* stream);

/* One memory's operands of the backward pass.  All 16-byte aligned, contiguous f32: dout [T][E][H] (the gradient of `out`), w_hh [4H][H],
 * cell, c_prev [T][E][H] and gates [T][E][4H] as lt_memory_seq_forward left them  ->  dgates [T][E][4H], every element written.
 * dc_carry [E][H]: scratch, the dc carry between steps (needs no initialisation; each element is read and rewritten by the one lane
 * that owns it).  There is no dh carry: the recurrent GEMM's result is consumed by the lane that owns the element. */
typedef struct lt_memory_seq_grad {
  const float* dout;
  const float* w_hh;
  const float* cell;
  const float* gates;
  const float* c_prev;
  float* dgates;
  float* dc_carry;
} lt_memory_seq_grad;

/* T launches, both networks in each: one pointwise launch opens the recursion at t = T - 1, then one per step t = T - 2 .. 0 (the
 * recurrent GEMM dgates[t+1] W_hh with the gate gradients of step t as its epilogue).  lt_lstm_backward's plan has one launch more,
 * the one that leaves dh0 / dc0; nothing here needs them.  dones as in lt_memory_seq_forward. */
int lt_memory_seq_backward(const lt_memory_seq_grad* actor, const lt_memory_seq_grad* critic, const uint8_t* dones, int64_t dones_stride,
                           int T, int E, int H, void* stream);

/* A VALUE, not a status: the output units per workgroup (64, 32 or 16 - the kernel variant) lt_memory_seq_backward takes for (E, H) on
 * the current device; 0 where it would refuse E or H.  The choice depends on the device's CU count and moves work between workgroups
 * only, never a sum's order; tests pin it so that the variant a shape is meant to cover cannot drift unnoticed. */
int lt_memory_seq_backward_units(int E, int H);

#ifdef __cplusplus
}
#endif

#endif /* LT_MEMORY_SEQ_H */
