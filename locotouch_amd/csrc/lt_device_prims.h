// Hardware primitives of the env kernels: the only place that names gfx950 intrinsics.  Everything above (lt_device_math.h,
// lt_physics_crba.h) is plain C++ over these, so tools/host_twin can run the very same physics source on the CPU (its own
// lt_device_prims.h emulates the quad exchange with four lock-stepped threads) and compare formulations in seconds.
#pragma once

#include <hip/hip_runtime.h>

namespace lt {

// quad DPP: value of another lane of the caller's quad (quad_perm control word CTRL)
template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dppi(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
// v_sqrt_f32 / v_rsq_f32 as they are (1 ulp).  `sqrtf` expands to ~16 VALU operations (denormal pre-scaling + a correctly-rounded
// fix-up) - 12 of them sat in every physics substep; nothing on this path is near the denormal range or needs the last bit.
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float frsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
// v_sin_f32 / v_cos_f32: |err| ~1e-6 on |x| < 4.6 rad (joint angles, reset Euler angles)
__device__ __forceinline__ float fsin(float x) { return __sinf(x); }
__device__ __forceinline__ float fcos(float x) { return __cosf(x); }

// a wave-uniform integer as the compiler can see it (v_readfirstlane): what is indexed by it alone is fetched by scalar loads
__device__ __forceinline__ int wave_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// v_mfma_f32_16x16x4_f32: D[m][n] += sum_k A[m][k] B[k][n] on a 16 x 16 tile, k < 4.  Lane (i = l % 16, q = l / 16) supplies A[i][q] and
// B[q][i]; acc[v] of lane (i, q) is D[4 q + v][i].  Exact f32 products, f32 accumulation.
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma_16x16x4(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

// the cell arithmetic of the recurrent kernels (lt_lstm.hip, lt_gru.hip, lt_memory.hip, lt_memory_gru.hip): v_exp_f32 forms; tanh from
// exp(-2 |x|), which never overflows
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { const float e = __expf(-2.f * fabsf(x)); const float t = (1.f - e) / (1.f + e); return x < 0.f ? -t : t; }

// nothing is scheduled across this point: loads issued above it stay above the arithmetic below it
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

// a value the optimiser cannot tie to its source: what is recomputed from it is recomputed, not kept live in registers
__device__ __forceinline__ float opaque(float x) { asm volatile("" : "+v"(x)); return x; }

}  // namespace lt
