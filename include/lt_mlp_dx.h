/* lt_mlp_dx.h - the gradient of a PPO loss with respect to the INPUT ROWS of the actor and critic stacks: the one hop
 * lt_mlp_backward_pair (lt_env.h) stops short of.  A feed-forward policy never needs it (its input rows are observations); for a
 * recurrent policy the rows are the memories' outputs, and lt_memory_seq_backward / lt_memory_gru_seq_backward take this gradient as
 * `dout`.  A header of its own, NOT included by lt_env.h: one optional unit (the opt-in `direct_recurrent_update` of rl/ppo.py alone
 * calls it); locotouch_amd/_abi.py derives its binding from this file by the same rule as from the other headers
 * (`_abi.MLP_DX_SIGNATURES`).  LT_ABI_VERSION stays 21.  Implemented in csrc/lt_mlp_dx.hip (the hop) and csrc/lt_mlp.hip (the packing).
 *
 * The hop is a kernel of its own behind the chain's launch: it reads dz_0 as the chain leaves it (f32, or the SPLIT FORMAT times
 * scales_out[k], both decoded exactly) and W_0 from a section that lies BESIDE the transposed streams in `bpacked`, and forms
 *     dx [m][dims[0]] = dz_0 [m][dims[1]] . W_0 [dims[1]][dims[0]]
 * with exact f32 products (v_mfma_f32_32x32x2_f32) accumulated in f32 in ONE fixed order (ascending over dims[1]): the same inputs
 * give the same bits on every run, a row's bits do not depend on m.  No float atomics, no allocation, no host read; stream-ordered.
 * The hop multiplies f32 by f32, so it cannot saturate and adds nothing to sat_count; the chain in front of it counts as before.
 * Validation is host-side, before anything is launched: LT_EINVAL with an lt_last_error() text
 * "<function>: invalid argument: <field> must be ...". */
#ifndef LT_MLP_DX_H
#define LT_MLP_DX_H

#include <stddef.h>
#include <stdint.h>

#include "lt_env.h" /* lt_mlp_desc, LT_* status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of a `bpacked` buffer that serves lt_mlp_backward_pair_dx: the lt_mlp_backward_packed_floats(fwd) floats of the transposed
 * streams, in the layout lt_mlp_backward_pair reads, and behind them dims[1] x dims[0] floats of W_0 (row-major, as torch.nn.Linear
 * holds it).  `fwd` must have a backward stream (lt_mlp_backward_packed_floats) and dims[0] a multiple of 8, <= 512. */
int lt_mlp_backward_dx_packed_floats(const lt_mlp_desc* fwd, size_t* floats);

/* lt_mlp_pack_training (lt_env.h) with both W_0 sections filled as well - still ONE launch.  bpacked0 / bpacked1: both required,
 * lt_mlp_backward_dx_packed_floats floats each. */
int lt_mlp_pack_training_dx(const lt_mlp_desc* d0, const float* const* weights0, const float* const* biases0, float* packed0, float* bpacked0,
                            const lt_mlp_desc* d1, const float* const* weights1, const float* const* biases1, float* packed1, float* bpacked1,
                            void* stream);

/* lt_mlp_backward_pair (lt_env.h: every argument up to `stream` as there) and, behind it on the same stream, the input gradients:
 *   dx0 [m][fwd0->dims[0]], dx1 [m][fwd1->dims[0]]: OUT, f32, every element written; dx_k = dz_{k,0} . W_{k,0}, unscaled - the true
 *   gradient of the loss with respect to the stack's input rows.  16-byte aligned, as are dz*[0] and bpacked*.
 * dz*, amax*, scales_out and sat_count are exactly what lt_mlp_backward_pair writes.  A NULL dx_k skips that network's hop; with both
 * NULL the entry is lt_mlp_backward_pair bit for bit, and bpacked* need no W_0 section.  Where dx_k is given, bpacked_k holds
 * lt_mlp_backward_dx_packed_floats floats as lt_mlp_pack_training_dx left them, and fwd_k->dims[0] is a multiple of 8, <= 512.
 * Two launches (one with both dx NULL). */
int lt_mlp_backward_pair_dx(const lt_mlp_desc* fwd0, const float* bpacked0, const float* dy0, const float* const* acts0, float* const* dz0,
                            float* const* amax0, const lt_mlp_desc* fwd1, const float* bpacked1, const float* dy1, const float* const* acts1,
                            float* const* dz1, float* const* amax1, int64_t m, int acts_split, const float* in_amax0, const float* in_amax1,
                            int dz_split, float* scales_out, float* sat_count, float* dx0, float* dx1, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_MLP_DX_H */
