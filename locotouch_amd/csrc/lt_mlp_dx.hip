// lt_mlp_dx.hip - the input gradient of the actor and critic stacks (include/lt_mlp_dx.h): dx = dz_0 . W_0 behind the backward chain of
// lt_mlp_backward_pair.  The chain (csrc/lt_mlp.hip) keeps its launch and its instantiations; this is one more launch that reads what the
// chain wrote - dz_0 as f32, or in the split format (one dword per element, f16 hi | f16 lo << 16, value = hi + lo / 64) still multiplied
// by the launch's power-of-two scale - and W_0 from the section lt_mlp_pack_training_dx leaves behind the transposed streams.
//
// Arithmetic: both decodings of dz_0 are exact in f32 (hi has 11 significant bits, lo / 64 lies at least 11 binades below it), the
// products are exact f32 (v_mfma_f32_32x32x2_f32), the sums f32 in ascending order of the hidden index, and the scale leaves through one
// multiplication by its exact reciprocal: the error is an f32 GEMM's own, and the hop cannot saturate.
// One workgroup of 4 waves forms a 128 x 128 block of dx (2 x 2 tiles of 32 x 32 per wave) from 32-wide panels staged in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lt_host_check.h"
#include "lt_mlp_dx.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int AS = BK + 4;   // floats per row of the dz panel: 16-byte rows, lanes of a tile spread over the banks
constexpr int BS = BN + 32;  // floats per row of the W_0 panel: the two k rows a wave reads at once lie 32 banks apart
constexpr int MAX_IN = 512;
constexpr float LO_INV = 1.f / 64.f;

struct DxNet {
  const float* dz;     // [m][n0]
  const float* w;      // [n0][k0]
  const float* scale;  // split dz: the scale it still carries (device float, a power of two); nullptr: none
  float* dx;           // [m][k0]; nullptr: this network has no hop
  int n0, k0, split;
};
struct DxArgs {
  DxNet net[2];
  long long m;
};

__device__ __forceinline__ float unsplit(unsigned w) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu)) + (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)) * LO_INV;
}

__global__ __launch_bounds__(256) void lt_mlp_dx_kernel(const DxArgs a) {
  const DxNet& n = a.net[blockIdx.z];
  const int col0 = blockIdx.y * BN;
  if (!n.dx || col0 >= n.k0) return;  // (uniform: the grid is that of the wider network)
  __shared__ __attribute__((aligned(16))) float As[BM * AS];
  __shared__ __attribute__((aligned(16))) float Bs[BK * BS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;  // the wave's 64 x 64 corner of the block
  const int h = lane >> 5, j = lane & 31;
  const long long row0 = (long long)blockIdx.x * BM;
  f32x16 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;
  for (int kb = 0; kb < n.n0; kb += BK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // dz panel: 128 rows x 8 groups of 4 hidden features; rows beyond m and features beyond n0 are zeros
      const int f = tid + 256 * i, r = f >> 3, q = f & 7;
      const long long row = row0 + r;
      const int k = kb + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < a.m && k < n.n0) {
        const uint4 u = *(const uint4*)(n.dz + row * n.n0 + k);
        v = n.split ? make_float4(unsplit(u.x), unsplit(u.y), unsplit(u.z), unsplit(u.w))
                    : make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
      }
      *(float4*)&As[r * AS + 4 * q] = v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // W_0 panel: 32 hidden features x 32 groups of 4 input columns
      const int f = tid + 256 * i, r = f >> 5, q = f & 31;
      const int k = kb + r, c = col0 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < n.n0 && c < n.k0) v = *(const float4*)(n.w + (long long)k * n.k0 + c);
      *(float4*)&Bs[r * BS + 4 * q] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < BK; kk += 2) {  // lane (j, h): A[row j][k = kk + h], B[k = kk + h][column j]
      float af[2], bf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t] = As[(wr + 32 * t + j) * AS + kk + h];
        bf[t] = Bs[(kk + h) * BS + wc + 32 * t + j];
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
    }
    __syncthreads();
  }
  float inv = 1.f;
  if (n.scale) {  // a power of two in the normal range (lt_mlp_kernel builds it from its exponent): the reciprocal by the exponent, exact
    const unsigned e = (__float_as_uint(*n.scale) >> 23) & 0xFFu;
    inv = __uint_as_float((254u - e) << 23);
  }
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int c = col0 + wc + 32 * tj + j;  // accumulator register r of lane (j, h): row (r & 3) + 8 (r >> 2) + 4 h, column j
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long row = row0 + wr + 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < a.m && c < n.k0) n.dx[row * n.k0 + c] = acc[ti][tj][r] * inv;
      }
    }
}

constexpr const char* FN = "lt_mlp_backward_pair_dx";

}  // namespace

extern "C" int lt_mlp_backward_pair_dx(const lt_mlp_desc* fwd0, const float* bpacked0, const float* dy0, const float* const* acts0, float* const* dz0,
                                       float* const* amax0, const lt_mlp_desc* fwd1, const float* bpacked1, const float* dy1, const float* const* acts1,
                                       float* const* dz1, float* const* amax1, int64_t m, int acts_split, const float* in_amax0, const float* in_amax1,
                                       int dz_split, float* scales_out, float* sat_count, float* dx0, float* dx1, void* stream) {
  const lt_mlp_desc* fw[2] = {fwd0, fwd1};
  const float* pk[2] = {bpacked0, bpacked1};
  const float* dy[2] = {dy0, dy1};
  const float* const* ac[2] = {acts0, acts1};
  float* const* dz[2] = {dz0, dz1};
  float* const* am[2] = {amax0, amax1};
  float* dx[2] = {dx0, dx1};
  const char* const who[2] = {"network 0: ", "network 1: "};
  if (m <= 0 || (m + BM - 1) / BM > 0x7FFFFFFFll) return refuse(FN, "", "m", "positive and below 2^31 blocks of 128 rows");
  size_t base[2] = {0, 0};
  for (int k = 0; k < 2; ++k) {
    if (!fw[k]) return refuse(FN, who[k], "fwd", "non-null");
    if (lt_mlp_backward_packed_floats(fw[k], &base[k]) != LT_OK)
      return refuse(FN, who[k], "fwd", "a network with a backward stream (lt_mlp_backward_packed_floats: ELU, >= 2 layers, hidden widths multiples of 8, <= 64 outputs)");
    if (dx[k] && (fw[k]->dims[0] % 8 != 0 || fw[k]->dims[0] > MAX_IN)) return refuse(FN, who[k], "fwd->dims[0]", "a multiple of 8 and <= 512");
    const ptr_check ptrs[] = {{"bpacked", pk[k], dx[k] ? 16 : 4}, {"dy", dy[k], 4}, {"acts", ac[k], 4}, {"dz", dz[k], 4}, {"amax", am[k], 4}};
    if (const int rc = check_ptrs(FN, who[k], ptrs)) return rc;
    for (int l = 0; l + 1 < fw[k]->num_layers; ++l) {
      const ptr_check layer[] = {{"acts[l]", ac[k][l], 4}, {"dz[l]", dz[k][l], l == 0 && dx[k] ? 16 : 4}, {"amax[l]", am[k][l], 4}};
      if (const int rc = check_ptrs(FN, who[k], layer)) return rc;
    }
    if (dx[k] && (uintptr_t)dx[k] % 16 != 0) return refuse(FN, who[k], "dx", "16-byte aligned (or NULL: no hop for this network)");
  }
  if (dz_split && (!in_amax0 || !in_amax1 || !scales_out)) return refuse(FN, "", "in_amax0, in_amax1 and scales_out", "non-null where dz_split is set");
  if (const int rc = lt_mlp_backward_pair(fwd0, bpacked0, dy0, acts0, dz0, amax0, fwd1, bpacked1, dy1, acts1, dz1, amax1, m, acts_split, in_amax0, in_amax1,
                                          dz_split, scales_out, sat_count, stream))
    return rc;
  if (!dx0 && !dx1) return LT_OK;
  DxArgs a = {};
  a.m = m;
  int widest = 0;
  for (int k = 0; k < 2; ++k) {
    DxNet& n = a.net[k];
    n.dx = dx[k];
    if (!dx[k]) continue;
    n.dz = dz[k][0]; n.w = pk[k] + base[k]; n.n0 = fw[k]->dims[1]; n.k0 = fw[k]->dims[0]; n.split = dz_split != 0;
    n.scale = dz_split ? scales_out + k : nullptr;
    widest = n.k0 > widest ? n.k0 : widest;
  }
  hipLaunchKernelGGL(lt_mlp_dx_kernel, dim3((unsigned)((m + BM - 1) / BM), (unsigned)((widest + BN - 1) / BN), 2), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status(FN);
}
