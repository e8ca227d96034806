/* lt_lstm.h - the LSTM recurrence of `Memory` / `PolicyMemory` over a padded batch of whole trajectories (part of the lt_env.h ABI, which
 * includes this file; LT_ABI_VERSION 21).  Semantics: a single-layer, unidirectional, time-major `nn.LSTM` with biases and without
 * projection (reference loco_rl/loco_rl/models/memory_module.py:6 and loco_rl/loco_rl/modules/actor_critic_recurrent.py:66-94, whose
 * default is "lstm"), gate order and formulas PyTorch's (i, f, g, o):
 *     a = x_t W_ih^T + b_ih + h_{t-1} W_hh^T + b_hh;  i, f, o = sigmoid(a_i, a_f, a_o);  g = tanh(a_g)
 *     c_t = f * c_{t-1} + i * g;  h_t = o * tanh(c_t)
 * Implemented in csrc/lt_lstm.hip: one launch per time step whose grid covers the chip, the time loop on the host side of these calls.
 *
 * The entry points live in a header of their own because they are one optional unit (a caller whose memories are GRUs never calls
 * them); locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h (`_abi.LSTM_SIGNATURES`).
 * All data pointers are device pointers to contiguous f32, 16-byte aligned; everything is stream-ordered: no host synchronisation, no
 * allocation, no host read and no float atomics.  Products are exact f32 (v_mfma_f32_16x16x4_f32), accumulation is f32, and every sum
 * has ONE fixed order that depends on the sizes alone, so the same inputs give the same bits on every run.  Validation is host-side,
 * before anything is launched: LT_EINVAL with an lt_last_error() text that names the function. */
#ifndef LT_LSTM_H
#define LT_LSTM_H

#ifdef __cplusplus
extern "C" {
#endif

/* FORWARD, L launches.  ig [L][B][4H] = X W_ih^T (no bias: one GEMM of the caller's over all steps), h0, c0 [B][H], w_hh [4H][H],
 * b_ih, b_hh [4H]  ->  out [L][B][H] (h_t), cell [L][B][H] (c_t), ws [L][B][4H] (the ACTIVATED gates i, f, g, o of each step; what the
 * backward pass reads).  Every element of the three outputs is written.  L, B >= 1; H >= 64 and a multiple of 64. */
int lt_lstm_forward(const float* ig, const float* h0, const float* c0, const float* w_hh, const float* b_ih, const float* b_hh, int L, int B,
                    int H, float* out, float* cell, float* ws, void* stream);

/* BACKWARD, L + 1 launches (one opens the recursion at t = L - 1, then one per step).  dout [L][B][H]: the gradient of `out`; dhn, dcn
 * [B][H]: the gradients of the final (h, c), each may be NULL (= 0); out, cell, ws, h0, c0, w_hh as lt_lstm_forward read / left them
 *   ->  dgates [L][B][4H]: the gradient of the gate pre-activations a (the input side and the hidden side of an LSTM share it: ONE
 * array), dh0, dc0 [B][H].  scratch [B][H]: the dc carry between steps (needs no initialisation; each element is read and rewritten by
 * the one lane that owns it; the dh carry needs no storage: an LSTM passes dh to the previous step through the recurrent GEMM alone,
 * whose result the same lane consumes at once).  tanh(c_t) is recomputed from `cell`.  The caller forms dW_hh = dgates^T H_prev,
 * dW_ih = dgates^T X, dX = dgates W_ih and db_ih = db_hh = the column sums of dgates.  `out` and `h0` are not read on the device (an LSTM's gate
 * gradients need c, not h; the two belong to the caller's dW_hh) but are required, so that a call names the whole forward record. */
int lt_lstm_backward(const float* dout, const float* dhn, const float* dcn, const float* out, const float* cell, const float* ws,
                     const float* h0, const float* c0, const float* w_hh, int L, int B, int H, float* dgates, float* scratch, float* dh0,
                     float* dc0, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_LSTM_H */
