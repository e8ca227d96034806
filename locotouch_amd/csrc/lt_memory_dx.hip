// The input gradient of a recurrent policy's two memories (include/lt_memory_dx.h): dx = dg W_ih, an [n x K] . [K x I] product per
// network, K = gates H, in one launch.  The plan is lt_memory_seq_bwd_kernel's (lt_memory_tile.h: dh = dg W_hh, the same sum order):
// a workgroup owns CT = 16 MT OUTPUT columns and a row block of RB rows;
//   1. its W_ih panel - COLUMNS c0 .. c0 + CT - 1 of W_ih, stored as rows [CT][K + 8] - is staged into LDS once (K = 2048: 16 columns,
//      128.5 KiB; K = 768, 1024: 32; K <= 512: 64 where I is that wide and the grid still covers the chip).  W_ih's rows are I floats
//      apart and only 4-byte aligned: scalar loads, consecutive columns by consecutive lanes.  Panel rows of columns >= I are zeros;
//   2. the four waves walk the row block in 16-row sub-tiles; the B operand (dg rows) comes straight from global memory, one 16-byte
//      load per lane and 16-wide k block, double-buffered in groups of four (K is a multiple of 64: whole groups); the A operand is
//      one ds_read_b128 per M tile and k block (the row stride K + 8 is an odd multiple of 8 floats);
//   3. the epilogue is a guarded store: panel row 16 mt + 4 g + v holds column c0 + 4 MT g + 4 mt + v, so lane (n, g) of the D layout
//      owns 4 MT consecutive columns of row n; rows may be any stride >= I apart and only 4-byte aligned, so the stores are scalar.
// grid (ceil(I_max / CT), ceil(n / RB), networks), block 256; a workgroup whose columns lie past its network's I leaves at once.
// Sum order: k blocks in index order dealt to four partial sums (block b to chain b % 4), added pairwise - whatever CT and RB are.
#include "lt_memory_dx.h"
#include "lt_memory_tile.h"

namespace {

struct DxNet { const float* dg; const float* w_ih; float* dx; long long DS; int I; };
struct DxArgs { DxNet net[2]; int n, K, RB; };

template <int MT>  // 16-column MFMA tiles per workgroup: 4, 2 or 1
__global__ __launch_bounds__(256) void lt_memory_dx_kernel(const DxArgs a) {
  constexpr int CT = 16 * MT;
  extern __shared__ __attribute__((aligned(16))) float panel[];  // [CT][KP]
  const DxNet& p = a.net[blockIdx.z];
  const int n = a.n, K = a.K, KP = K + 8, I = p.I;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int c0 = blockIdx.x * CT;
  if (c0 >= I) return;  // (the whole workgroup: the other network is wider)
  const int r0 = blockIdx.y * a.RB;
  const int r1 = min(n, r0 + a.RB);

  // ---- 1. the panel, once: W_ih[j][c0 + u] (consecutive u: coalesced) -> panel row 16 mt + 4 g + v with u = 4 MT g + 4 mt + v
  for (int idx = tid; idx < K * CT; idx += 256) {
    const int j = idx / CT, u = idx - j * CT;
    const int pr = 16 * ((u >> 2) % MT) + 4 * (u / (4 * MT)) + (u & 3);
    panel[pr * KP + j] = c0 + u < I ? p.w_ih[(long long)j * I + c0 + u] : 0.f;
  }
  __syncthreads();

  // ---- 2. the row block, 16 rows per wave and pass
  const int nblk = K / 16;  // a multiple of four
  const int nsub = (r1 - r0 + 15) / 16;
  for (int s = wave; s < nsub; s += 4) {
    const int row = r0 + 16 * s + i;
    const bool row_ok = row < r1;
    const int rc = row_ok ? row : r0;  // (a clamped lane computes a column of D nobody stores)
    const float* grow = p.dg + (long long)rc * K + 4 * q;
    f32x4 acc[4][MT];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[u][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 cur[4], nxt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = *(const f32x4*)(grow + 16 * u);
    for (int b0 = 0; b0 < nblk; b0 += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        nxt[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (b0 + 4 < nblk) nxt[u] = *(const f32x4*)(grow + 16 * (b0 + 4 + u));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* ap = panel + i * KP + 16 * (b0 + u) + 4 * q;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const f32x4 w = *(const f32x4*)(ap + 16 * mt * KP);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[u][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[e], cur[u][e], acc[u][mt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
    }
    // ---- 3. epilogue: sum[v] of lane (n, g), tile mt is D[4 g + v][n] = dx of column c0 + 4 MT g + 4 mt + v, row n
    if (!row_ok) continue;
    const int col0 = c0 + 4 * MT * q;
    float* out = p.dx + (long long)row * p.DS + col0;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 sum = (acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt]);
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (col0 + 4 * mt + v < I) out[4 * mt + v] = sum[v];
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
int check_net(const char* fn, const char* who, const lt_memory_dx_net* m, const lt_memory_dx_net* other, long long n, int H, int K) {
  if (m->I < 1 || m->I > 512 || m->I + H > 1248) return refuse(fn, who, ".I", "in [1, 512] with I + H <= 1248");
  if (m->dx_stride < m->I) return refuse(fn, who, ".dx_stride", "at least I");
  if (const int rc = check_ptrs(fn, who, {{".dg", m->dg, 16}, {".w_ih", m->w_ih, 4}, {".dx", m->dx, 4}})) return rc;
  const long long span = (n - 1) * (long long)m->dx_stride + m->I;  // floats from the first element written to the last
  for (const lt_memory_dx_net* o : {m, other})
    if (o && ((o->dg && overlaps(m->dx, span, o->dg, n * K)) || (o->w_ih && o->I > 0 && overlaps(m->dx, span, o->w_ih, (long long)K * o->I))))
      return refuse(fn, who, ".dx", "a buffer that does not overlap dg / w_ih of either network");
  return LT_OK;
}

int check_call(const char* fn, const lt_memory_dx_net* actor, const lt_memory_dx_net* critic, int64_t n, int H, int gates) {
  if (gates != 3 && gates != 4) return refuse(fn, "", "gates", "3 (GRU) or 4 (LSTM)");
  if (n < 1 || n > 16 * 65535) return refuse(fn, "", "n", "in [1, 16 * 65535]");
  if (const int rc = check_sizes(fn, "n", (int)n, H)) return rc;
  if (!actor) return refuse(fn, "actor", "", "non-null");
  if (const int rc = check_net(fn, "actor", actor, critic, n, H, gates * H)) return rc;
  if (critic)
    if (const int rc = check_net(fn, "critic", critic, actor, n, H, gates * H)) return rc;
  return LT_OK;
}

// output columns per workgroup: the widest panel (64, 32 or 16 columns of W_ih) that fits the LDS, is no wider than the half of it
// would already cover, and still leaves the grid at least half a workgroup per CU (64-row passes), else narrower.  The choice moves
// work between workgroups, never a sum's order.
int dx_cols(int n, int K, int imax, int nets) {
  int ct = 16;
  for (const int cand : {64, 32, 16}) {
    if (cand * (K + 8) * (int)sizeof(float) > kLdsBytes) continue;
    if (cand > 16 && cand / 2 >= imax) continue;
    const int tiles = nets * ((imax + cand - 1) / cand);
    const int rb = row_block(n, tiles);
    ct = cand;
    if (2LL * tiles * ((n + rb - 1) / rb) >= cu_count()) break;
  }
  return ct;
}

}  // namespace

extern "C" {

int lt_memory_input_grad_launches(const lt_memory_dx_net* actor, const lt_memory_dx_net* critic, int64_t n, int H, int gates) {
  if (const int rc = check_call("lt_memory_input_grad_launches", actor, critic, n, H, gates)) return rc;
  return 1;
}

int lt_memory_input_grad(const lt_memory_dx_net* actor, const lt_memory_dx_net* critic, int64_t n, int H, int gates, void* stream) {
  const char* fn = "lt_memory_input_grad";
  if (const int rc = check_call(fn, actor, critic, n, H, gates)) return rc;
  const int nets = critic ? 2 : 1;
  const lt_memory_dx_net* src[2] = {actor, critic ? critic : actor};
  DxArgs a;
  for (int k = 0; k < 2; ++k) a.net[k] = {src[k]->dg, src[k]->w_ih, src[k]->dx, (long long)src[k]->dx_stride, src[k]->I};
  a.n = (int)n; a.K = gates * H;
  const int imax = nets == 2 && critic->I > actor->I ? critic->I : actor->I;
  const int ct = dx_cols(a.n, a.K, imax, nets);
  const int tiles = (imax + ct - 1) / ct;
  a.RB = row_block(a.n, nets * tiles);
  const int lds = ct * (a.K + 8) * (int)sizeof(float);
  const kernel_fn<DxArgs> kernel = ct == 64 ? lt_memory_dx_kernel<4> : ct == 32 ? lt_memory_dx_kernel<2> : lt_memory_dx_kernel<1>;
  if (const int rc = allow_lds(kernel)) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)((a.n + a.RB - 1) / a.RB), (unsigned)nets), dim3(256), lds, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // extern "C"
