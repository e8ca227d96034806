/* lt_mlp_rows.h - the training forward and the backward chain of two networks in one launch, with a ROW COUNT PER NETWORK:
 * lt_mlp_forward_pair and lt_mlp_backward_pair (lt_env.h) with (m0, m1) in place of m.  The PPO update with the mirror loss and no data
 * augmentation (rl/ppo.py, include/lt_ppo_mirror.h) runs the actor on 2 m rows [original; mirrored] and the critic on m.
 *
 * A header of its own, NOT included by lt_env.h (whose ABI version and signatures it leaves alone): one optional unit, bound by one row
 * of locotouch_amd/_abi.py's header table.  Implemented in csrc/lt_mlp.hip: host code only.  The kernel and its instantiations are those
 * of the equal-row entries; it has always dealt its workgroups either by block range - [0, b0) run network 0, [b0, b0 + b1) network 1 -
 * or, where both networks need the same number of workgroups, by XCD, and these entries let b0 and b1 differ.  The row tiles per
 * workgroup are ONE choice for the launch, from the 16-row tiles of both networks together.  With m0 == m1 an entry chooses the launch
 * of its equal-row twin and writes the same bits.  Network k reads and writes its own m_k rows and nothing behind them.
 *
 * Validation is host-side, before anything is launched: LT_EINVAL with an lt_last_error() text "<function>: invalid argument: <field>
 * must be ...".  Stream-ordered, no allocation, no host read. */
#ifndef LT_MLP_ROWS_H
#define LT_MLP_ROWS_H

#include <stddef.h>
#include <stdint.h>

#include "lt_env.h" /* lt_mlp_desc, LT_* status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* lt_mlp_forward_pair: x0 [m0][dims0[0]], x1 [m1][dims1[0]] -> y0 [m0][out0], y1 [m1][out1] and acts_k[l] [m_k][dims_k[l + 1]].
 * m0, m1 >= 1; hidden widths multiples of 4. */
int lt_mlp_forward_pair_rows(const lt_mlp_desc* d0, const float* packed0, const float* x0, const lt_mlp_desc* d1, const float* packed1,
                             const float* x1, int64_t m0, int64_t m1, float* y0, float* y1, float* const* acts0, float* const* acts1,
                             int acts_split, void* stream);

/* Workgroups per network of lt_mlp_backward_pair_rows over (m0, m1) rows: *blocks_k = the entries of every amax array of network k.
 * With m0 == m1 both are lt_mlp_backward_blocks(fwd0, fwd1, m0). */
int lt_mlp_backward_blocks_rows(const lt_mlp_desc* fwd0, const lt_mlp_desc* fwd1, int64_t m0, int64_t m1, int64_t* blocks0, int64_t* blocks1);

/* lt_mlp_backward_pair: dy_k [m_k][out_k], acts_k[l] and dz_k[l] [m_k][dims_k[l + 1]], amax_k[l] [*blocks_k]; every other argument
 * as there (in_amax_k, dz_split, scales_out[2], sat_count). */
int lt_mlp_backward_pair_rows(const lt_mlp_desc* fwd0, const float* bpacked0, const float* dy0, const float* const* acts0, float* const* dz0,
                              float* const* amax0, const lt_mlp_desc* fwd1, const float* bpacked1, const float* dy1, const float* const* acts1,
                              float* const* dz1, float* const* amax1, int64_t m0, int64_t m1, int acts_split, const float* in_amax0,
                              const float* in_amax1, int dz_split, float* scales_out, float* sat_count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_MLP_ROWS_H */
