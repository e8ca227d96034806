// Device functions of the PPO minibatch loss, shared by its three kernels: lt_ppo_loss_kernel (lt_ppo.hip), lt_ppo_loss_sym_kernel
// (lt_ppo_sym.hip, the mirror-augmented batch) and lt_ppo_loss_mirror_kernel (the same file, the mirror loss without augmentation).  One text for the pieces whose numeric care was paid for once: the float64 exponential
// of a log-std policy's sigma, the KL with true divisions, the branch rules of the two clips, the block reduction and the one-wave finish.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace {

constexpr int MAX_A = 16;
constexpr float kHalfLog2Pi = 0.91893853320467274178f;

// sigma of a log-std policy (actor_critic.py:109-112).  The ONE exponential of lt_std_from_log (what a rollout stores as sigma) and of
// the loss kernels (what they compare that sigma against): the same bits from the same log_std.  Formed in float64 and rounded once: an
// error in sigma is the same in every row and enters a row's log-prob times z^2 (64 at |z| = 8), so the ulp an f32 exponential may be
// off by showed as 6.5e-6 of max |dmu| against float64 where the nearest float32 sigma gives 1e-6 (tests/test_hip_ppo_opts_f64.py).
// A workgroup forms its A sigmas once (the loss kernels keep them in LDS).
__device__ __forceinline__ float lt_sigma_of_log(float log_std) { return (float)exp((double)log_std); }

// One action's share of a row's log-prob: -z^2 / 2 - log sigma - log sqrt(2 pi).  LOG: stdp_a is log sigma, the parameter itself.
template <bool LOG>
__device__ __forceinline__ float lt_ppo_logp_term(float z, float sg, float stdp_a) {
  if constexpr (LOG) return -0.5f * z * z - stdp_a - kHalfLog2Pi;
  else return -0.5f * z * z - __logf(sg) - kHalfLog2Pi;
}

// One action's share of a row's KL to the behaviour policy (ppo.py:266-272).
// The two sigmas are state-independent, so an error in sg / os is the SAME in every row and does not average out over the
// minibatch, and each action's KL is a small difference of terms ~0.1: with the library's -freciprocal-math quotients and
// __logf the mean KL sat 2 - 8 times further from float64 than plain float32 does (tests/test_hip_ppo_f64.py).  True
// divisions and logf here; the kernels wait on memory either way.
__device__ __forceinline__ float lt_ppo_kl_term(float sg, float os, float om, float m) {
#pragma clang fp reciprocal(off)
  return logf(sg / os + 1.0e-5f) + (os * os + (om - m) * (om - m)) / (2.f * sg * sg) - 0.5f;
}

// The clipped surrogate of one row: declares its two branches `s1`, `s2` (the row's surrogate is fmaxf(s1, s2)) and `dsurr` = d surrogate /
// d ratio.  `torch.max(a, b)` splits the gradient evenly on ties; inside the clip range both branches are equal AND have the same
// derivative, so the closed form is exactly autograd's.  (A macro, as the two below and for their reason.)
#define LT_PPO_SURROGATE(advr, ratio, clip, s1, s2, dsurr)                        \
  const float s1 = -(advr) * (ratio);                                             \
  const float rc_##s1 = fminf(fmaxf(ratio, 1.f - (clip)), 1.f + (clip));          \
  const float s2 = -(advr) * rc_##s1;                                             \
  const bool inside_##s1 = (ratio) >= 1.f - (clip) && (ratio) <= 1.f + (clip);    \
  const float dsurr = (s1 > s2 || inside_##s1) ? -(advr) : 0.f;

// The value loss `vl` of one row (clipped or plain) and its derivative `dv` with respect to the value; both must be declared floats.
// This, the surrogate above and the block reduction below are MACROS, not functions: their text expands in place, so lt_ppo_loss_kernel compiles to the very
// instructions it compiled to before the text moved here (as inline functions with out-parameters the same arithmetic came out in
// another instruction order).
#define LT_PPO_VALUE_LOSS(v, R, old_values, src, clip, clipped_value, vl, dv)                                       \
  if (clipped_value) {                                                                                              \
    const float ov = (old_values)[src];                                                                             \
    const float dcl = fminf(fmaxf((v) - ov, -(clip)), clip);                                                        \
    const float vc = ov + dcl;                                                                                      \
    const float l1 = ((v) - (R)) * ((v) - (R)), l2 = (vc - (R)) * (vc - (R));                                       \
    const bool in_v = ((v) - ov) >= -(clip) && ((v) - ov) <= (clip);                                                \
    vl = fmaxf(l1, l2);                                                                                             \
    dv = (l1 > l2 || in_v) ? 2.f * ((v) - (R)) : 0.f; /* outside the clip range the clipped branch has no derivative */ \
  } else {                                                                                                          \
    vl = ((R) - (v)) * ((R) - (v));                                                                                 \
    dv = 2.f * ((v) - (R));                                                                                         \
  }

// Block reduction of a 256-thread loss block (wave butterflies, then 4 partials through LDS), one atomic per block and slot:
// acc[i] += sum of part[i] for i < 4 + A (slot 3 only with SLOT3), acc[20] / acc[21] = max with the block's two maxima (bit patterns of
// non-negative floats, merged with an integer atomicMax: order-independent).  Once per kernel, at the end of its body.
#define LT_PPO_BLOCK_REDUCE(part, amax_mu, amax_v, A, acc, SLOT3)                                                                 \
  __shared__ float red[4][4 + MAX_A];                                                                                             \
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                                                     \
  _Pragma("unroll") for (int i = 0; i < 4 + MAX_A; ++i) {                                                                         \
    float v = part[i];                                                                                                            \
    _Pragma("unroll") for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);                                         \
    if (lane == 0) red[wave][i] = v;                                                                                              \
  }                                                                                                                               \
  _Pragma("unroll") for (int off = 32; off > 0; off >>= 1) {                                                                      \
    amax_mu = fmaxf(amax_mu, __shfl_xor(amax_mu, off, 64));                                                                       \
    amax_v = fmaxf(amax_v, __shfl_xor(amax_v, off, 64));                                                                          \
  }                                                                                                                               \
  __shared__ float redm[4][2];                                                                                                    \
  if (lane == 0) { redm[wave][0] = amax_mu; redm[wave][1] = amax_v; }                                                             \
  __syncthreads();                                                                                                                \
  if (threadIdx.x < 4 + A && ((SLOT3) || threadIdx.x != 3)) {                                                                     \
    const int i = threadIdx.x;                                                                                                    \
    atomicAdd(acc + i, red[0][i] + red[1][i] + red[2][i] + red[3][i]);                                                            \
  } else if (threadIdx.x >= 64 && threadIdx.x < 66) { /* (another wave: one atomic per block and maximum) */                      \
    const int j = threadIdx.x - 64;                                                                                               \
    atomicMax((unsigned*)acc + 20 + j, __float_as_uint(fmaxf(fmaxf(redm[0][j], redm[1][j]), fmaxf(redm[2][j], redm[3][j]))));     \
  }

// The scalars of a minibatch loss from the sums of its loss kernel, the body of the one-wave finish (thread a < 64): out[0] loss, [1] mean
// surrogate, [2] mean value loss, [3] entropy, [4] mean KL, [8 + a] d loss / d sigma_a.  In PyTorch ops this was a dozen launches on
// 12-float tensors.  entropy = sum_a (0.5 + 0.5 log 2 pi + log sigma_a) (the same in every row: the std is state-independent).
// std_is_log (uniform): stdp is log sigma - the entropy's summand is the parameter itself, and its share of d loss / d log sigma_a is
// -ecoef.
__device__ __forceinline__ void lt_ppo_finalize(const float* __restrict__ acc, const float* __restrict__ stdp, int A, float inv_m, float vcoef, float ecoef,
                                                int std_is_log, float* __restrict__ out) {
  const int a = threadIdx.x;
  float e = 0.f;
  if (a < A && std_is_log) {
    e = 0.5f + kHalfLog2Pi + stdp[a];
    out[8 + a] = acc[4 + a] - ecoef;
  } else if (a < A) {
    const float sg = stdp[a];
    e = 0.5f + kHalfLog2Pi + logf(sg);
    out[8 + a] = acc[4 + a] - ecoef / sg;
  }
  for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off, 64);
  if (a == 0) {
    const float surr = acc[0] * inv_m, vl = acc[1] * inv_m;
    out[0] = surr + vcoef * vl - ecoef * e;
    out[1] = surr; out[2] = vl; out[3] = e; out[4] = acc[2] * inv_m;
  }
}

}  // namespace
