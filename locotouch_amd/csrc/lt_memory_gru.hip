// The two GRU memories of a recurrent policy: one rollout step of both in one launch, and both over a whole rollout of an env block,
// forward and backward (include/lt_memory_gru.h).  The GRU counterpart of lt_memory.hip, in a file of its own: that file, and with it
// every LSTM instantiation, is byte for byte what it was.
//
// Step kernel.  lt_memory_step_kernel's layout, unchanged: a workgroup owns UT hidden units and a ROW BLOCK of RB rows, stages its
// weight panel [4 UT][I + H] into LDS once, the four waves walk the row block in 16-row sub-tiles with the B operand (x_t | h rows)
// straight from global memory, and the gate arithmetic is the epilogue in registers.  The n gate needs its x part and its h part as
// SEPARATE sums (b_hn sits inside r * (...)), so a unit again has four panel rows:
//     v = 0: [W_ir | W_hr]      v = 1: [W_iz | W_hz]      v = 2: [W_in | 0]      v = 3: [0 | W_hn]
// and lane (n, g) of the D layout still holds everything of one unit of row n: (a_r, a_z, the x part of a_n, h W_hn^T).  A quarter of
// the MFMAs multiply zeros; a three-row layout would put the gates of one unit into different lanes (the M index of a 16-row tile is
// 4 g + v: three rows per unit do not divide it) and the epilogue through LDS.
// grid (H / UT, ceil(N / RB), 2 networks), block 256.
//
// The reset mask is applied WHERE THE OPERAND IS LOADED, as in lt_memory.hip: h of the previous step is read as where(done, 0, .) by
// every workgroup that needs it and the buffer itself is never rewritten.  The new raw state goes to the other ping-pong buffer.  The
// workgroups of unit tile 0 also copy the masked pre-step state of their row block into the storage slot.
//
// Arithmetic: v_mfma_f32_16x16x4_f32, exact f32 products, f32 accumulation, k blocks in index order (x side first, then h) dealt to
// four partial sums that are added pairwise: one fixed order, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "lt_env.h"
#include "lt_internal.h"
#include "lt_memory_gru.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { const float e = __expf(-2.f * fabsf(x)); const float t = (1.f - e) / (1.f + e); return x < 0.f ? -t : t; }

struct NetArgs {
  const float* x; const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; const float* h_in;
  float* h_out; float* saved_h;
  int I, IP, KP;  // IP: I rounded up to 16 (the x side's k blocks; the panel holds zeros in [I, IP)); KP: LDS row stride in floats
};
struct StepArgs { NetArgs net[2]; const uint8_t* dones; int N, H, RB; };
// TRAIN (lt_memory_gru_seq_forward): r, z, n and hn of every (row, unit) also go to `gates` ([N][4H] per network)
struct SeqStepArgs : StepArgs { float* gates[2]; };

constexpr int kLdsBytes = 160 * 1024;

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// LDS row stride: IP + H + 8 is an odd multiple of 8 floats (lt_memory.hip's rule: 16 distinct bank groups per ds_read_b128 lane group)
__host__ __device__ inline int panel_stride(int I, int H) { return round_up(I, 16) + H + 8; }

// The B operand of k block `blk` for lane (row, q): x[row][16 blk + 4 q .. + 3] (zeros past I; rows are only 4-byte aligned unless
// `xvec`), or behind the x side's blocks where(done, 0, h[row][...]).
__device__ __forceinline__ f32x4 load_b(const float* __restrict__ xrow, const float* __restrict__ hrow, int blk, int q, int I, int xblks, bool xvec,
                                        bool done) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (blk < xblks) {
    const int k = 16 * blk + 4 * q;
    if (xvec && k + 3 < I) {
      v = *(const f32x4*)(xrow + k);
    } else {
      if (k < I) v[0] = xrow[k];
      if (k + 1 < I) v[1] = xrow[k + 1];
      if (k + 2 < I) v[2] = xrow[k + 2];
      if (k + 3 < I) v[3] = xrow[k + 3];
    }
  } else if (!done) {
    v = *(const f32x4*)(hrow + 16 * (blk - xblks) + 4 * q);
  }
  return v;
}

// MT consecutive floats as ONE access (MT = 4: 16 bytes, MT = 2: 8 bytes; the offsets are multiples of MT floats from 16-byte aligned rows)
template <int MT> __device__ __forceinline__ void load_units(const float* __restrict__ src, float* dst) {
  if constexpr (MT == 4) { const f32x4 v = *(const f32x4*)src; dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3]; }
  else { const f32x2 v = *(const f32x2*)src; dst[0] = v[0]; dst[1] = v[1]; }
}
template <int MT> __device__ __forceinline__ void store_units(float* __restrict__ dst, const float* src) {
  if constexpr (MT == 4) *(f32x4*)dst = (f32x4){src[0], src[1], src[2], src[3]};
  else *(f32x2*)dst = (f32x2){src[0], src[1]};
}

template <int UT, bool TRAIN = false>  // UT: hidden units per workgroup, 16 or 8
__global__ __launch_bounds__(256) void lt_memory_gru_step_kernel(const std::conditional_t<TRAIN, SeqStepArgs, StepArgs> a) {
  constexpr int MT = UT / 4;  // 16-row MFMA tiles of the panel; lane (n, g) of the D layout owns units g * MT .. + MT - 1 of its row
  extern __shared__ __attribute__((aligned(16))) float panel[];  // [4 UT][KP]
  const NetArgs& p = a.net[blockIdx.z];
  const int N = a.N, H = a.H, I = p.I, IP = p.IP, KP = p.KP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * UT;
  const int r0 = blockIdx.y * a.RB;
  const int r1 = min(N, r0 + a.RB);

  // ---- 1. the weight panel, once.  Panel row pr = 16 mt + 4 g + v holds row v (file comment) of unit j0 + g * MT + mt
  for (int idx = tid; idx < 4 * UT * IP; idx += 256) {
    const int pr = idx / IP, k = idx - pr * IP, v = pr & 3;
    const int unit = j0 + ((pr >> 2) & 3) * MT + (pr >> 4);
    panel[pr * KP + k] = v < 3 && k < I ? p.w_ih[(long long)(v * H + unit) * I + k] : 0.f;
  }
  const int h4 = H / 4;
  for (int idx = tid; idx < 4 * UT * h4; idx += 256) {
    const int pr = idx / h4, k4 = idx - pr * h4, v = pr & 3;
    const int unit = j0 + ((pr >> 2) & 3) * MT + (pr >> 4), wrow = (v == 3 ? 2 : v) * H + unit;
    f32x4 w = {0.f, 0.f, 0.f, 0.f};
    if (v != 2) w = *(const f32x4*)(p.w_hh + (long long)wrow * H + 4 * k4);
    *(f32x4*)(panel + pr * KP + IP + 4 * k4) = w;
  }

  // ---- the masked pre-step state of this row block -> the storage slot (unit tile 0 alone; every element of the slot's rows)
  if (blockIdx.x == 0) {
    for (int idx = tid; idx < (r1 - r0) * h4; idx += 256) {
      const int r = r0 + idx / h4;
      const long long o = (long long)r * H + 4 * (idx % h4);
      const bool done = a.dones && a.dones[r] != 0;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(p.saved_h + o) = done ? z : *(const f32x4*)(p.h_in + o);
    }
  }

  // ---- the biases of this lane's units (lane (n, g): units j0 + g * MT + mt): b_ir + b_hr, b_iz + b_hz, b_in, b_hn
  float bias[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int unit = j0 + q * MT + mt;
    bias[mt][0] = p.b_ih[unit] + p.b_hh[unit];
    bias[mt][1] = p.b_ih[H + unit] + p.b_hh[H + unit];
    bias[mt][2] = p.b_ih[2 * H + unit];
    bias[mt][3] = p.b_hh[2 * H + unit];
  }
  __syncthreads();

  // ---- 2. the row block, 16 rows per wave and pass
  const int xblks = IP / 16, nblk = xblks + H / 16;
  const bool xvec = (I & 3) == 0 && ((uintptr_t)p.x & 15) == 0;
  const int nsub = (r1 - r0 + 15) / 16;
  for (int s = wave; s < nsub; s += 4) {
    const int row = r0 + 16 * s + i;  // the row this lane feeds as the B operand, and (n = i) the row it owns in the epilogue
    const bool row_ok = row < r1;
    const int rc = row_ok ? row : r0;  // (a clamped lane computes a column of D nobody stores)
    const bool done = a.dones && a.dones[rc] != 0;
    const float* xrow = p.x + (long long)rc * I;
    const float* hrow = p.h_in + (long long)rc * H;
    // the epilogue's operand, requested now: h of (row, units j0 + q * MT .. + MT - 1)
    float hp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) hp[mt] = 0.f;
    if (!done) load_units<MT>(hrow + j0 + q * MT, hp);
    // four partial sums per panel row (k block b goes to chain b % 4), added pairwise at the end
    f32x4 acc[4][MT];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[u][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 cur[4], nxt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = load_b(xrow, hrow, u, q, I, xblks, xvec, done);  // (nblk >= 5: H >= 64 and I >= 1)
    for (int b0 = 0; b0 < nblk; b0 += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        nxt[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (b0 + 4 + u < nblk) nxt[u] = load_b(xrow, hrow, b0 + 4 + u, q, I, xblks, xvec, done);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (b0 + u < nblk) {
          const float* ap = panel + i * KP + 16 * (b0 + u) + 4 * q;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const f32x4 w = *(const f32x4*)(ap + 16 * mt * KP);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[e], cur[u][e], acc[u][mt], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
    }
    // ---- 3. epilogue: sum[v] of lane (n, g) is D[4 g + v][n] = panel row v of unit j0 + g * MT + mt, row n
    if (!row_ok) continue;
    float hnew[MT];
    [[maybe_unused]] float act[4][MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 sum = (acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt]);
      const float gr = sigmoidf_(sum[0] + bias[mt][0]);
      const float gz = sigmoidf_(sum[1] + bias[mt][1]);
      const float hn = sum[3] + bias[mt][3];
      const float gn = tanhf_(sum[2] + bias[mt][2] + gr * hn);
      hnew[mt] = (1.f - gz) * gn + gz * hp[mt];
      if constexpr (TRAIN) { act[0][mt] = gr; act[1][mt] = gz; act[2][mt] = gn; act[3][mt] = hn; }
    }
    store_units<MT>(p.h_out + (long long)row * H + j0 + q * MT, hnew);
    if constexpr (TRAIN) {
      float* g = a.gates[blockIdx.z] + (long long)row * 4 * H + j0 + q * MT;
#pragma unroll
      for (int v = 0; v < 4; ++v) store_units<MT>(g + v * H, act[v]);
    }
  }
}

// out = where(dones, 0, raw) for the two state arrays; grid (ceil(N H / 4 / 256), 2 arrays)
struct FinishArgs { const float* in[2]; float* out[2]; const uint8_t* dones; int N, H; };

__global__ __launch_bounds__(256) void lt_memory_gru_finish_kernel(const FinishArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // one float4
  const int h4 = a.H / 4;
  if (idx >= (long long)a.N * h4) return;
  const int r = (int)(idx / h4);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!(a.dones && a.dones[r] != 0)) v = *(const f32x4*)(a.in[blockIdx.y] + 4 * idx);
  *(f32x4*)(a.out[blockIdx.y] + 4 * idx) = v;
}

// ---- lt_memory_gru_seq_backward -------------------------------------------------------------------------------------------------------
// lt_memory_seq_bwd_kernel's plan with K = 3H: dh = dhg[t+1] W_hh, an [E x 3H] . [3H x H] product.  A workgroup owns UB = 16 MT OUTPUT
// units and a row block; its W_hh panel - COLUMNS k0 .. k0 + UB - 1 of W_hh, stored as rows [UB][3H + 8] (3H + 8 is an odd multiple of 8
// floats: H is a multiple of 64) - is staged into LDS once; the B operand (dhg[t+1] rows) comes straight from global memory; the gate
// gradients of step t are the epilogue, in registers: lane (n, g) of the D layout owns 4 MT CONSECUTIVE units of row n.  3H / 16 k
// blocks are whole groups of four.  The carry dh * z [E][H] is read and rewritten by the lane that owns the element.  dones[t] cuts the
// recursion: a done row takes neither the GEMM's result nor the carry.
struct BwdNet {
  const float* w_hh; const float* dhg_next; const float* dout; const float* gates; const float* h_prev;
  float* dig; float* dhg; float* carry;
};
struct BwdArgs { BwdNet net[2]; const uint8_t* dones; int E, H, RB; };

struct GradOps { f32x4 dout, hp, g[4]; };  // g: r, z, n, hn

__device__ __forceinline__ GradOps load_grad_ops(const BwdNet& p, long long row, int unit, int H) {
  GradOps e;
  const long long o = row * H + unit;
  e.dout = *(const f32x4*)(p.dout + o);
  e.hp = *(const f32x4*)(p.h_prev + o);
#pragma unroll
  for (int v = 0; v < 4; ++v) e.g[v] = *(const f32x4*)(p.gates + row * 4 * H + v * H + unit);
  return e;
}

// the gate gradients of four consecutive units of one row; `back` is where(done, 0, dhg[t+1] W_hh + carry)
__device__ __forceinline__ void store_gate_grads(const BwdNet& p, long long row, int unit, int H, const GradOps& e, f32x4 back) {
  f32x4 dr, dz, dn, dnr, carry;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float dh = e.dout[v] + back[v];
    const float gr = e.g[0][v], gz = e.g[1][v], gn = e.g[2][v], hn = e.g[3][v];
    dn[v] = dh * (1.f - gz) * (1.f - gn * gn);
    dz[v] = dh * (e.hp[v] - gn) * gz * (1.f - gz);
    dr[v] = dn[v] * hn * gr * (1.f - gr);
    dnr[v] = dn[v] * gr;
    carry[v] = dh * gz;
  }
  float* gi = p.dig + row * 3 * H + unit;
  float* gh = p.dhg + row * 3 * H + unit;
  *(f32x4*)gi = dr; *(f32x4*)(gi + H) = dz; *(f32x4*)(gi + 2 * H) = dn;
  *(f32x4*)gh = dr; *(f32x4*)(gh + H) = dz; *(f32x4*)(gh + 2 * H) = dnr;
  *(f32x4*)(p.carry + row * H + unit) = carry;
}

// opens the recursion at t = T - 1: dh = dout.  grid (ceil(E H / 4 / 256), 2 networks)
__global__ __launch_bounds__(256) void lt_memory_gru_seq_bwd_open_kernel(const BwdArgs a) {
  const BwdNet& p = a.net[blockIdx.y];
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // four units of one row
  const int h4 = a.H / 4;
  if (idx >= (long long)a.E * h4) return;
  const long long row = idx / h4;
  const int unit = 4 * (int)(idx - row * h4);
  store_gate_grads(p, row, unit, a.H, load_grad_ops(p, row, unit, a.H), (f32x4){0.f, 0.f, 0.f, 0.f});
}

__host__ __device__ inline int bwd_panel_stride(int H) { return 3 * H + 8; }

template <int MT>  // 16-unit MFMA tiles per workgroup: 4, 2 or 1
__global__ __launch_bounds__(256) void lt_memory_gru_seq_bwd_kernel(const BwdArgs a) {
  constexpr int UB = 16 * MT;
  extern __shared__ __attribute__((aligned(16))) float panel[];  // [UB][KP]
  const BwdNet& p = a.net[blockIdx.z];
  const int E = a.E, H = a.H, K = 3 * H, KP = bwd_panel_stride(H);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int k0 = blockIdx.x * UB;
  const int r0 = blockIdx.y * a.RB;
  const int r1 = min(E, r0 + a.RB);

  // ---- 1. the panel, once: W_hh[j][k0 + u] (consecutive u: coalesced) -> panel row 16 mt + 4 g + v with u = 4 MT g + 4 mt + v
  for (int idx = tid; idx < K * UB; idx += 256) {
    const int j = idx / UB, u = idx - j * UB;
    const int pr = 16 * ((u >> 2) % MT) + 4 * (u / (4 * MT)) + (u & 3);
    panel[pr * KP + j] = p.w_hh[(long long)j * H + k0 + u];
  }
  __syncthreads();

  // ---- 2. the row block, 16 rows per wave and pass
  const int nblk = K / 16;  // 12 (H / 64): whole groups of four k blocks
  const int nsub = (r1 - r0 + 15) / 16;
  for (int s = wave; s < nsub; s += 4) {
    const int row = r0 + 16 * s + i;
    const bool row_ok = row < r1;
    const int rc = row_ok ? row : r0;  // (a clamped lane computes a column of D nobody stores)
    const float* grow = p.dhg_next + (long long)rc * K + 4 * q;
    // the epilogue's operands, requested now: (row, units k0 + 4 MT q .. + 4 MT - 1) of step t
    const int unit0 = k0 + 4 * MT * q;
    const bool done = a.dones && a.dones[rc] != 0;
    GradOps ops[MT];
    f32x4 carry[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      ops[mt] = load_grad_ops(p, rc, unit0 + 4 * mt, H);
      carry[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (!done) carry[mt] = *(const f32x4*)(p.carry + (long long)rc * H + unit0 + 4 * mt);
    }
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
    // ---- 3. epilogue: sum[v] of lane (n, g), tile mt is D[4 g + v][n] = dh of unit k0 + 4 MT g + 4 mt + v, row n
    if (!row_ok) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      f32x4 back = ((acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt])) + carry[mt];
      if (done) back = (f32x4){0.f, 0.f, 0.f, 0.f};
      store_gate_grads(p, row, unit0 + 4 * mt, H, ops[mt], back);
    }
  }
}

// ---- host side: validation before anything is launched --------------------------------------------------------------------------------
int refuse(const char* fn, const char* who, const char* field, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: invalid argument: %s%s must be %s", fn, who, field, what);
  lt_set_error(msg);
  return LT_EINVAL;
}

struct ptr_check { const char* name; const void* p; int align; };

int check_ptr(const char* fn, const char* who, const ptr_check& e) {
  if (!e.p || (uintptr_t)e.p % e.align != 0) return refuse(fn, who, e.name, e.align == 16 ? "non-null and 16-byte aligned" : "non-null and 4-byte aligned");
  return LT_OK;
}

int check_sizes(const char* fn, const char* rows, int N, int H) {
  if (N < 1 || N > 16 * 65535) return refuse(fn, "", rows, "in [1, 16 * 65535]");
  if (H < 64 || H > 512 || (H % 64) != 0) return refuse(fn, "", "H", "a multiple of 64 in [64, 512]");
  return LT_OK;
}

int check_net(const char* fn, const char* who, const lt_memory_gru_net* n, int H) {
  if (!n) return refuse(fn, who, "", "non-null");
  if (n->I < 1 || n->I + H > 1248) return refuse(fn, who, ".I", "at least 1 with I + H <= 1248");
  const ptr_check ptrs[] = {{".x", n->x, 4}, {".w_ih", n->w_ih, 4}, {".w_hh", n->w_hh, 16}, {".b_ih", n->b_ih, 16}, {".b_hh", n->b_hh, 16},
                            {".h_in", n->h_in, 16}, {".h_out", n->h_out, 16}, {".saved_h", n->saved_h, 16}};
  for (const auto& e : ptrs)
    if (const int rc = check_ptr(fn, who, e)) return rc;
  if (n->h_out == n->h_in) return refuse(fn, who, ".h_out", "another buffer than .h_in (ping-pong)");
  return LT_OK;
}

int cu_count() {
  static int cus = 0;  // (every device of a node is the same chip)
  if (cus == 0) {
    int dev = 0, v = 0;
    cus = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
  }
  return cus;
}

// row block: the grid covers the chip about once (one workgroup per CU: the panel takes most of its LDS), whole 64-row passes
int row_block(int N, int tiles) {
  const int cus = cu_count();
  const int blocks = cus / tiles > 0 ? cus / tiles : 1;
  return round_up((N + blocks - 1) / blocks, 64);
}

// unit tile, LDS bytes, row block (into a.RB) and grid of one step launch
dim3 step_plan(StepArgs& a, int& ut, int& lds) {
  const int kp = a.net[0].KP > a.net[1].KP ? a.net[0].KP : a.net[1].KP;
  ut = 64 * kp * (int)sizeof(float) <= kLdsBytes ? 16 : 8;  // 32 x 1280 floats fill the LDS exactly: I + H <= 1248 always fits
  lds = 4 * ut * kp * (int)sizeof(float);
  a.RB = row_block(a.N, 2 * (a.H / ut));
  return dim3((unsigned)(a.H / ut), (unsigned)((a.N + a.RB - 1) / a.RB), 2);
}

int check_seq_sizes(const char* fn, int T, int E, int H, const uint8_t* dones, int64_t dones_stride) {
  if (T < 1) return refuse(fn, "", "T", "at least 1");
  if (const int rc = check_sizes(fn, "E", E, H)) return rc;
  if (dones && dones_stride < E) return refuse(fn, "", "dones_stride", "at least E");
  return LT_OK;
}

bool overlaps(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}

int check_seq_net(const char* fn, const char* who, const lt_memory_gru_seq_net* n, const lt_memory_gru_seq_net* other, int T, int E, int H) {
  if (!n) return refuse(fn, who, "", "non-null");
  if (n->I < 1 || n->I + H > 1248) return refuse(fn, who, ".I", "at least 1 with I + H <= 1248");
  if (n->x_stride < (int64_t)E * n->I) return refuse(fn, who, ".x_stride", "at least E * I");
  const long long EH = (long long)E * H, TEH = (long long)T * EH;
  const ptr_check ptrs[] = {{".x", n->x, 4}, {".w_ih", n->w_ih, 4}, {".w_hh", n->w_hh, 16}, {".b_ih", n->b_ih, 16}, {".b_hh", n->b_hh, 16},
                            {".h0", n->h0, 16}, {".out", n->out, 16}, {".gates", n->gates, 16}, {".h_prev", n->h_prev, 16}};
  for (const auto& e : ptrs)
    if (const int rc = check_ptr(fn, who, e)) return rc;
  const struct { const char* name; const void* p; long long floats; } outs[] = {{".out", n->out, TEH}, {".gates", n->gates, 4 * TEH}, {".h_prev", n->h_prev, TEH}};
  for (const auto& e : outs)
    for (const lt_memory_gru_seq_net* m : {n, other})
      if (m && m->h0 && overlaps(e.p, e.floats, m->h0, EH)) return refuse(fn, who, e.name, "a buffer that does not overlap h0 of either network");
  return LT_OK;
}

int check_seq_grad(const char* fn, const char* who, const lt_memory_gru_seq_grad* n) {
  if (!n) return refuse(fn, who, "", "non-null");
  const ptr_check ptrs[] = {{".dout", n->dout, 16}, {".w_hh", n->w_hh, 16}, {".gates", n->gates, 16}, {".h_prev", n->h_prev, 16},
                            {".dig", n->dig, 16}, {".dhg", n->dhg, 16}, {".dh_carry", n->dh_carry, 16}};
  for (const auto& e : ptrs)
    if (const int rc = check_ptr(fn, who, e)) return rc;
  return LT_OK;
}

// output units per workgroup of the backward step: the widest panel (64, 32 or 16 columns of W_hh) that fits the LDS and still leaves
// the grid at least half a workgroup per CU (64-row passes), else narrower.  The choice moves work between workgroups, never a sum's order.
int bwd_units(int E, int H) {
  const int kp = bwd_panel_stride(H);
  int ub = 16;
  for (const int cand : {64, 32, 16}) {
    if (cand * kp * (int)sizeof(float) > kLdsBytes) continue;
    const int tiles = 2 * (H / cand);
    const int rb = row_block(E, tiles);
    ub = cand;
    if (2LL * tiles * ((E + rb - 1) / rb) >= cu_count()) break;
  }
  return ub;
}

int launch_status() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  return LT_OK;
}

template <bool TRAIN> const void* step_kernel(int ut) {
  return ut == 16 ? (const void*)lt_memory_gru_step_kernel<16, TRAIN> : (const void*)lt_memory_gru_step_kernel<8, TRAIN>;
}

}  // namespace

extern "C" {

int lt_memory_gru_step(const lt_memory_gru_net* actor, const lt_memory_gru_net* critic, const uint8_t* dones, int N, int H, void* stream) {
  const char* fn = "lt_memory_gru_step";
  if (const int rc = check_sizes(fn, "N", N, H)) return rc;
  if (const int rc = check_net(fn, "actor", actor, H)) return rc;
  if (const int rc = check_net(fn, "critic", critic, H)) return rc;
  const lt_memory_gru_net* nets[2] = {actor, critic};
  StepArgs a;
  for (int k = 0; k < 2; ++k) {
    NetArgs& r = a.net[k];
    const lt_memory_gru_net* n = nets[k];
    r.x = n->x; r.w_ih = n->w_ih; r.w_hh = n->w_hh; r.b_ih = n->b_ih; r.b_hh = n->b_hh; r.h_in = n->h_in; r.h_out = n->h_out;
    r.saved_h = n->saved_h; r.I = n->I; r.IP = round_up(n->I, 16); r.KP = panel_stride(n->I, H);
  }
  a.dones = dones; a.N = N; a.H = H;
  int ut, lds;
  const dim3 grid = step_plan(a, ut, lds);
  if (const int e = lt_ensure_dynamic_lds(step_kernel<false>(ut), kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  if (ut == 16) hipLaunchKernelGGL(lt_memory_gru_step_kernel<16>, grid, dim3(256), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(lt_memory_gru_step_kernel<8>, grid, dim3(256), lds, (hipStream_t)stream, a);
  return launch_status();
}

int lt_memory_gru_finish(const float* h_a, const float* h_c, const uint8_t* dones, int N, int H, float* out_h_a, float* out_h_c, void* stream) {
  const char* fn = "lt_memory_gru_finish";
  if (const int rc = check_sizes(fn, "N", N, H)) return rc;
  const ptr_check ptrs[] = {{"h_a", h_a, 16}, {"h_c", h_c, 16}, {"out_h_a", out_h_a, 16}, {"out_h_c", out_h_c, 16}};
  for (const auto& e : ptrs)
    if (const int rc = check_ptr(fn, "", e)) return rc;
  FinishArgs a;
  a.in[0] = h_a; a.in[1] = h_c; a.out[0] = out_h_a; a.out[1] = out_h_c;
  a.dones = dones; a.N = N; a.H = H;
  const long long n4 = (long long)N * (H / 4);
  hipLaunchKernelGGL(lt_memory_gru_finish_kernel, dim3((unsigned)((n4 + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status();
}

int lt_memory_gru_seq_forward(const lt_memory_gru_seq_net* actor, const lt_memory_gru_seq_net* critic, const uint8_t* dones,
                              int64_t dones_stride, int T, int E, int H, void* stream) {
  const char* fn = "lt_memory_gru_seq_forward";
  if (const int rc = check_seq_sizes(fn, T, E, H, dones, dones_stride)) return rc;
  if (const int rc = check_seq_net(fn, "actor", actor, critic, T, E, H)) return rc;
  if (const int rc = check_seq_net(fn, "critic", critic, actor, T, E, H)) return rc;
  const lt_memory_gru_seq_net* nets[2] = {actor, critic};
  SeqStepArgs a;
  for (int k = 0; k < 2; ++k) {
    NetArgs& r = a.net[k];
    const lt_memory_gru_seq_net* n = nets[k];
    r.w_ih = n->w_ih; r.w_hh = n->w_hh; r.b_ih = n->b_ih; r.b_hh = n->b_hh;
    r.I = n->I; r.IP = round_up(n->I, 16); r.KP = panel_stride(n->I, H);
  }
  a.N = E; a.H = H;
  int ut, lds;
  const dim3 grid = step_plan(a, ut, lds);
  if (const int e = lt_ensure_dynamic_lds(step_kernel<true>(ut), kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  const long long EH = (long long)E * H;
  for (int t = 0; t < T; ++t) {
    for (int k = 0; k < 2; ++k) {
      NetArgs& r = a.net[k];
      const lt_memory_gru_seq_net* n = nets[k];
      r.x = n->x + t * n->x_stride;
      r.h_in = t == 0 ? n->h0 : n->out + (t - 1) * EH;
      r.h_out = n->out + t * EH;
      r.saved_h = n->h_prev + t * EH;
      a.gates[k] = n->gates + 4 * t * EH;
    }
    a.dones = dones && t > 0 ? dones + (t - 1) * dones_stride : nullptr;
    if (ut == 16) hipLaunchKernelGGL((lt_memory_gru_step_kernel<16, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((lt_memory_gru_step_kernel<8, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
  }
  return launch_status();
}

int lt_memory_gru_seq_backward_units(int E, int H) {
  if (E < 1 || E > 16 * 65535 || H < 64 || H > 512 || (H % 64) != 0) return 0;
  return bwd_units(E, H);
}

int lt_memory_gru_seq_backward(const lt_memory_gru_seq_grad* actor, const lt_memory_gru_seq_grad* critic, const uint8_t* dones,
                               int64_t dones_stride, int T, int E, int H, void* stream) {
  const char* fn = "lt_memory_gru_seq_backward";
  if (const int rc = check_seq_sizes(fn, T, E, H, dones, dones_stride)) return rc;
  if (const int rc = check_seq_grad(fn, "actor", actor)) return rc;
  if (const int rc = check_seq_grad(fn, "critic", critic)) return rc;
  const lt_memory_gru_seq_grad* nets[2] = {actor, critic};
  const int kp = bwd_panel_stride(H);
  const int ub = bwd_units(E, H);
  const int rb = row_block(E, 2 * (H / ub));
  const int lds = ub * kp * (int)sizeof(float);
  const void* kernel = ub == 64 ? (const void*)lt_memory_gru_seq_bwd_kernel<4> : ub == 32 ? (const void*)lt_memory_gru_seq_bwd_kernel<2>
                                                                                           : (const void*)lt_memory_gru_seq_bwd_kernel<1>;
  if (T > 1)
    if (const int e = lt_ensure_dynamic_lds(kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  const long long EH = (long long)E * H;
  BwdArgs a;
  a.E = E; a.H = H; a.RB = rb; a.dones = nullptr;
  auto at = [&](int t) {
    for (int k = 0; k < 2; ++k) {
      BwdNet& r = a.net[k];
      const lt_memory_gru_seq_grad* n = nets[k];
      r.w_hh = n->w_hh; r.dhg_next = t + 1 < T ? n->dhg + 3 * (t + 1) * EH : nullptr;
      r.dout = n->dout + t * EH; r.gates = n->gates + 4 * t * EH; r.h_prev = n->h_prev + t * EH;
      r.dig = n->dig + 3 * t * EH; r.dhg = n->dhg + 3 * t * EH; r.carry = n->dh_carry;
    }
  };
  at(T - 1);
  hipLaunchKernelGGL(lt_memory_gru_seq_bwd_open_kernel, dim3((unsigned)((EH / 4 + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream, a);
  const dim3 grid((unsigned)(H / ub), (unsigned)((E + rb - 1) / rb), 2);
  for (int t = T - 2; t >= 0; --t) {
    at(t);
    a.dones = dones ? dones + t * dones_stride : nullptr;
    switch (ub) {
      case 64: hipLaunchKernelGGL(lt_memory_gru_seq_bwd_kernel<4>, grid, dim3(256), lds, (hipStream_t)stream, a); break;
      case 32: hipLaunchKernelGGL(lt_memory_gru_seq_bwd_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, a); break;
      default: hipLaunchKernelGGL(lt_memory_gru_seq_bwd_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, a); break;
    }
  }
  return launch_status();
}

}  // extern "C"
