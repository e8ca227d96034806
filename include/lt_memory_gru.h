/* lt_memory_gru.h - the two GRU memories of a recurrent policy (`ActorCriticRecurrent(rnn_type="gru")`): one ROLLOUT step of both in
 * one launch (the GRU counterpart of lt_memory.h) and both over a WHOLE ROLLOUT [T][E] of an env block, forward and backward (the
 * counterpart of lt_memory_seq.h).  A header of its own, NOT included by lt_env.h: one optional unit (the opt-in `fused_gru_memories`
 * of rl/fused.py and rl/ppo.py alone calls it); locotouch_amd/_abi.py derives its binding from this file by the same rule as from the
 * other headers (`_abi.MEMORY_GRU_SIGNATURES`).  LT_ABI_VERSION stays 21.  Implemented in csrc/lt_memory_gru.hip.
 *
 * Semantics per network, step t (PyTorch's gate order r, z, n; reference loco_rl/loco_rl/algorithms/ppo.py:130-131 `act`, :170
 * `reset(dones)`):
 *     h        = where(dones[t-1], 0, raw h step t-1 left)                `PolicyMemory.reset(dones)`, applied where the operand is loaded
 *     saved[t] = h                                                         the state BEFORE the step (`h_prev[t]` of the sequence form)
 *     r  = sigmoid(x W_ir^T + b_ir + h W_hr^T + b_hr);   z = sigmoid(x W_iz^T + b_iz + h W_hz^T + b_hz)
 *     hn = h W_hn^T + b_hn;                               n = tanh(x W_in^T + b_in + r * hn)
 *     h' = (1 - z) * n + z * h                                             the new RAW state, written to ANOTHER buffer than the one read
 * Backward over a rollout, t = T - 1 .. 0 (dhg[T] = 0, the carry dh_T z_T = 0):
 *     dh_t = dout[t] + where(dones[t], 0, dhg[t+1] W_hh + dh_{t+1} * z_{t+1})
 *     dn = dh_t (1 - z)(1 - n^2);   dz = dh_t (h_prev[t] - n) z (1 - z);   dr = dn * hn * r (1 - r)
 *     dig[t] = (dr, dz, dn)         dhg[t] = (dr, dz, dn * r)
 * The gradients of h0 and of x are not computed: the saved states and the observations carry no gradient.  The caller forms
 * dW_ih = dig^T X, dW_hh = dhg^T h_prev, db_ih = the column sums of dig and db_hh = those of dhg.
 *
 * Products are exact f32 (v_mfma_f32_16x16x4_f32), accumulation is f32, every sum has ONE fixed order that depends on the sizes alone:
 * the same inputs give the same bits on every run.  Stream-ordered: no allocation, no host read, no float atomics.  Validation is
 * host-side, before anything is launched: LT_EINVAL with an lt_last_error() text "<function>: invalid argument: <field> must be ...".
 *
 * Supported (lt_memory.h's set): a single-layer GRU with biases, f32, H a multiple of 64 with 64 <= H <= 512, I >= 1 with
 * I + H <= 1248 (a workgroup keeps its weight panel, 32 rows x (I + H), in LDS), 1 <= N, E <= 16 * 65535, T >= 1. */
#ifndef LT_MEMORY_GRU_H
#define LT_MEMORY_GRU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One memory's operands of one rollout step.  Device pointers to contiguous f32.  16-byte aligned: w_hh [3H][H], b_ih, b_hh [3H], h_in,
 * h_out [N][H], saved_h [N][H] (slot t of a [T][1][N][H] array).  4-byte aligned: x [N][I] (I need not be a multiple of 4) and w_ih
 * [3H][I].  h_out must not be h_in: other workgroups of the same launch still read that (the ping-pong of the caller). */
typedef struct lt_memory_gru_net {
  const float* x;
  int I;
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* h_in;
  float* h_out;
  float* saved_h;
} lt_memory_gru_net;

/* ONE launch: the step above for `actor` and `critic` (a grid dimension selects the network).  dones: uint8 [N] of the PREVIOUS step, or
 * NULL (t = 0: the state is taken as it is).  Every element of h_out and saved_h of both networks is written. */
int lt_memory_gru_step(const lt_memory_gru_net* actor, const lt_memory_gru_net* critic, const uint8_t* dones, int N, int H, void* stream);

/* ONE small launch behind the last env step: out = where(dones, 0, raw) for the state array [N][H] of both networks (dones: uint8 [N]
 * of the LAST step, NULL = a plain copy) - the state a following eager step, `compute_returns` or a checkpoint sees. */
int lt_memory_gru_finish(const float* h_a, const float* h_c, const uint8_t* dones, int N, int H, float* out_h_a, float* out_h_c, void* stream);

/* One memory's operands of the forward pass over a rollout.  4-byte aligned: x (row e of step t is x + t * x_stride + e * I: a block
 * [:, e0:e1] of the rollout storage [T][N][I] is read in place with x_stride = N * I) and w_ih [3H][I].  16-byte aligned and contiguous:
 * w_hh [3H][H], b_ih, b_hh [3H], h0 [E][H], out, h_prev [T][E][H], gates [T][E][4H] (four planes of H per row: r, z, n, hn).  No output
 * may overlap h0 of either network.  Every element of the three outputs is written. */
typedef struct lt_memory_gru_seq_net {
  const float* x;
  int64_t x_stride;
  int I;
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* h0;
  float* out;
  float* gates;
  float* h_prev;
} lt_memory_gru_seq_net;

/* T launches, both networks in each.  dones: uint8, row t at dones + t * dones_stride, E bytes (dones_stride >= E), or NULL (no reset
 * anywhere); the mask of step t is row t - 1, step 0 takes h0 as given. */
int lt_memory_gru_seq_forward(const lt_memory_gru_seq_net* actor, const lt_memory_gru_seq_net* critic, const uint8_t* dones,
                              int64_t dones_stride, int T, int E, int H, void* stream);

/* One memory's operands of the backward pass.  All 16-byte aligned, contiguous f32: dout [T][E][H] (the gradient of `out`), w_hh
 * [3H][H], gates [T][E][4H] and h_prev [T][E][H] as lt_memory_gru_seq_forward left them  ->  dig, dhg [T][E][3H], every element written:
 * the two operands of the weight gradients as they are multiplied, no copy in between.  dh_carry [E][H]: scratch, the carry dh * z
 * between steps (needs no initialisation; each element is read and rewritten by the one lane that owns it). */
typedef struct lt_memory_gru_seq_grad {
  const float* dout;
  const float* w_hh;
  const float* gates;
  const float* h_prev;
  float* dig;
  float* dhg;
  float* dh_carry;
} lt_memory_gru_seq_grad;

/* T launches, both networks in each: one pointwise launch opens the recursion at t = T - 1, then one per step t = T - 2 .. 0 (the
 * recurrent GEMM dhg[t+1] W_hh, K = 3H, with the gate gradients of step t as its epilogue).  dones as in lt_memory_gru_seq_forward. */
int lt_memory_gru_seq_backward(const lt_memory_gru_seq_grad* actor, const lt_memory_gru_seq_grad* critic, const uint8_t* dones,
                               int64_t dones_stride, int T, int E, int H, void* stream);

/* A VALUE, not a status: the output units per workgroup (64, 32 or 16 - the kernel variant) lt_memory_gru_seq_backward takes for (E, H)
 * on the current device; 0 where it would refuse E or H.  The W_hh column panel is [units][3H + 8] floats of the 160 KiB of LDS: 64
 * units fit up to H = 192, 32 up to H = 384, 16 always.  The choice moves work between workgroups only, never a sum's order. */
int lt_memory_gru_seq_backward_units(int E, int H);

#ifdef __cplusplus
}
#endif

#endif /* LT_MEMORY_GRU_H */
