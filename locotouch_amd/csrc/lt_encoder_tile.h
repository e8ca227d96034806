// The device helpers of the row-block layer engine (plan and arithmetic: the header comment of lt_encoder.hip), shared by lt_encoder.hip
// (the encoder in front of the stacks, forward and backward) and lt_policy_encoder.hip (the play-time step: encoder and actor in one
// launch).  A four-wave workgroup keeps the activations of a row block in LDS, streams each layer's weights through LDS a panel at a
// time and takes 16 x 16 tiles of panel x block: `stage` / `stage_panel` fill LDS, `tile_sum` is one tile's product, `activate` the
// epilogue's function.  One statement of each, so one order of every sum: k blocks of 16 in index order dealt to four partial sums
// (block b to chain b % 4) that are added pairwise.  Internal to the translation units that include it: an unnamed namespace.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lt_device_prims.h"
#include "lt_env.h"

namespace {

using lt::f32x4;

// LDS row stride of a [rows][width] array (activations or a panel): round_up(width, 16) + 8 floats, an odd multiple of 8, so the 16
// lanes of a ds_read_b128 lane group start at 16 distinct multiples of 4 banks
__host__ __device__ inline int lds_stride(int width) { return (width + 15) / 16 * 16 + 8; }

__device__ __forceinline__ float activate(int kind, float x) {
  if (kind == LT_ACT_ELU) return x > 0.f ? x : expm1f(x);
  if (kind == LT_ACT_RELU) return x > 0.f ? x : 0.f;
  if (kind == LT_ACT_TANH) return tanhf(x);
  return x;
}

// floor(2^32 / d) + 1 (d a power of two: 2^32 / d): __umulhi(i, .) is i / d exactly while i * d < 2^32 - here i < 64 * 1024, d <= 1024
__device__ __forceinline__ unsigned div_magic(int d) { return 0xFFFFFFFFu / (unsigned)d + 1u; }

// Stages a [rows][cols] tile (elements of type V: float, or f32x4 where the source allows 16-byte loads; cols in elements) into LDS rows
// of dst_stride FLOATS: element (r, c) from src + r * src_stride floats where r < rows_ok and c < cols_ok, else zeros.  The loads of a
// thread are independent and U of them are in flight before the first LDS write: a load per loop trip would expose the whole
// global-memory latency once per element (measured: 110 us of a 112 us launch at 4096 rows).
template <int U, class V>
__device__ __forceinline__ void stage(const float* __restrict__ src, long long src_stride, int rows_ok, int cols_ok, float* __restrict__ dst,
                                      int dst_stride, int rows, int cols, int tid) {
  constexpr int VW = sizeof(V) / sizeof(float);
  const int total = rows * cols;
  const unsigned magic = div_magic(cols);
  for (int base = 0; base < total; base += 256 * U) {
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + 256 * u + tid;
      const int r = (int)__umulhi((unsigned)idx, magic), c = idx - r * cols;
      v[u] = V{};
      if (idx < total && r < rows_ok && c < cols_ok) v[u] = *(const V*)(src + (long long)r * src_stride + VW * c);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + 256 * u + tid;
      const int r = (int)__umulhi((unsigned)idx, magic), c = idx - r * cols;
      if (idx < total) *(V*)(dst + r * dst_stride + VW * c) = v[u];
    }
  }
}

// The panel of a forward layer: rows p0 .. p0 + pm16 - 1 of w [O][K] (torch's layout) into LDS rows of lds_stride(K) floats, zeros
// behind O and behind K up to the last k block's end.  16-byte loads where K and w allow them, UV of them in flight per thread, else
// 4-byte loads, US in flight; PAIR: 8-byte loads where K is even and w 8-byte aligned (the play-time step's 334-column layer).  The
// defaults are the encoder kernels' form.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int UV = 8, int US = 16, bool PAIR = false>
__device__ __forceinline__ void stage_panel(const float* __restrict__ w, int K, int O, int p0, int pm16, float* __restrict__ panel, int tid) {
  const int K16 = (K + 15) / 16 * 16, kp = K16 + 8;
  if ((K & 3) == 0 && ((uintptr_t)w & 15) == 0)
    stage<UV, f32x4>(w + (long long)p0 * K, K, O - p0, K / 4, panel, kp, pm16, K16 / 4, tid);
  else if (PAIR && (K & 1) == 0 && ((uintptr_t)w & 7) == 0)
    stage<US, f32x2>(w + (long long)p0 * K, K, O - p0, K / 2, panel, kp, pm16, K16 / 2, tid);
  else
    stage<US, float>(w + (long long)p0 * K, K, O - p0, K, panel, kp, pm16, K16, tid);
}

// One 16 x 16 tile over nblk k blocks of 16: ap / bp are lane (i, q)'s addresses in the A operand (panel row 16 mt + i, column 4 q) and
// the B operand (activation row 16 s + i, column 4 q); MFMA step e of block b consumes the k-set {16 b + 4 q + e}, so either operand is
// one ds_read_b128 per block.  Returns the pairwise sum of the four chains: component v of lane (i, q) is D[4 q + v][i].
__device__ __forceinline__ f32x4 tile_sum(const float* ap, const float* bp, int nblk) {
  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < nblk; b0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (b0 + u < nblk) {
        const f32x4 wv = *(const f32x4*)(ap + 16 * (b0 + u));
        const f32x4 xv = *(const f32x4*)(bp + 16 * (b0 + u));
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u] = lt::mfma_16x16x4(wv[e], xv[e], acc[u]);
      }
    }
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

}  // namespace
