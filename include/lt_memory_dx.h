/* lt_memory_dx.h - the gradient of a loss with respect to the INPUT ROWS of a recurrent policy's two memories: the one hop
 * lt_memory_seq_backward / lt_memory_gru_seq_backward (lt_memory_seq.h, lt_memory_gru.h) stop short of.  A policy whose memories read
 * observations never needs it; where a layer stands in front of a memory (an encoder on some columns of the row, as in the reference's
 * pre-encoder teacher) that layer trains on this gradient.  A header of its own, NOT included by lt_env.h: one optional unit
 * (rl/memory_seq.py calls it where a row tensor requires a gradient, or where `direct_backward` is given `dx_out`);
 * locotouch_amd/_abi.py derives its binding from this file by the same rule as from the other headers (`_abi.MEMORY_DX_SIGNATURES`).
 * LT_ABI_VERSION stays 21.  Implemented in csrc/lt_memory_dx.hip.
 *
 * Per network and row r < n, with K = gates * H (gates: 3 for a GRU, 4 for an LSTM):
 *     dx[r][i] = sum over k < K of dg[r][k] * w_ih[k][i]                  for i < I
 * dg is the cell's ih-side gate gradient as the sequence backward pass left it: `dgates` [T][E][4H] of lt_memory_seq_backward, `dig`
 * [T][E][3H] of lt_memory_gru_seq_backward, with n = T * E.  The call sequence is the sequence backward, then this.
 *
 * Products are exact f32 (v_mfma_f32_16x16x4_f32), accumulation is f32.  The k range is taken in 16-wide blocks in index order, block b
 * goes to partial sum b % 4, and the four sums are added as (0 + 1) + (2 + 3): ONE fixed order that depends on K alone.  A row's bits
 * depend on that row of dg and on w_ih and on nothing else - not on n, not on the row's place, not on the second network, not on the
 * tile shapes the host picks for the device.  Stream-ordered: no allocation, no host read, no atomics.  Validation is host-side, before
 * anything is launched: LT_EINVAL with an lt_last_error() text "<function>: invalid argument: <field> must be ...".
 *
 * Supported: f32, H a multiple of 64 with 64 <= H <= 512 (K = 192 .. 2048), 1 <= I <= 512 with I + H <= 1248, 1 <= n <= 16 * 65535. */
#ifndef LT_MEMORY_DX_H
#define LT_MEMORY_DX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One memory's operands.  Device pointers to f32.
 *   dg         [n][K], contiguous, 16-byte aligned.
 *   w_ih       [K][I], torch's layout, 4-byte aligned: a view of a flat parameter bucket will do.
 *   dx         OUT: row r is the I floats at dx + r * dx_stride, dx_stride >= I, 4-byte aligned - the result can land in the tail columns
 *              of a wider gradient row.  Every element of the I columns of every row is written; nothing outside them is.  It may not
 *              overlap dg or w_ih of either network. */
typedef struct lt_memory_dx_net {
  const float* dg;
  const float* w_ih;
  int I;
  float* dx;
  int64_t dx_stride;
} lt_memory_dx_net;

/* One launch for both networks (a grid dimension selects the network); they may differ in I and share n, H and gates.  critic may be
 * NULL: the actor alone, with the same bits. */
int lt_memory_input_grad(const lt_memory_dx_net* actor, const lt_memory_dx_net* critic, int64_t n, int H, int gates, void* stream);

/* A VALUE, not a status: the launches lt_memory_input_grad makes for these arguments - 1 - or, where it would refuse them, its
 * negative status (the lt_last_error() text names this function and the same field).  Nothing is launched. */
int lt_memory_input_grad_launches(const lt_memory_dx_net* actor, const lt_memory_dx_net* critic, int64_t n, int H, int gates);

#ifdef __cplusplus
}
#endif

#endif /* LT_MEMORY_DX_H */
