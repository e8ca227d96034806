// One rollout step of the two LSTM memories of a recurrent policy in one launch (include/lt_memory.h).
//
// Shape: B = num_envs rows (4096 and up), K = I + H (observation width + hidden size), 4H gate rows, two networks.  lt_lstm.hip's step
// kernel is laid out for the update (B ~ 47: a 16 x 16 tile per workgroup, weights streamed once per tile); at the rollout's shape that
// re-reads all of W_hh once per 16 rows and leaves the input GEMM to a library call.  Here a workgroup owns UT hidden units (4 UT gate
// rows of [W_ih | W_hh]) and a ROW BLOCK of RB rows:
//   1. the weight panel [4 UT][I + H] is staged into LDS ONCE (UT = 16: 64 gate rows, up to 160 KiB; UT = 8 when that does not fit);
//   2. the four waves walk the row block in 16-row sub-tiles (wave w takes sub-tiles w, w + 4, ...): the B operand (x_t | h rows) comes
//      straight from global memory, one 16-byte load per lane and 16-wide k block, double-buffered in groups of four blocks; the A
//      operand is one ds_read_b128 per M tile and k block; 4 UT / 16 MFMA tiles share each B load;
//   3. the gate arithmetic is the epilogue, in registers: the M index of a tile is 4 * g + gate, so lane (n, g) of the D layout holds the
//      four gates of ONE unit of row n - no LDS round trip, no second launch.
// grid (H / UT, ceil(N / RB), 2 networks), block 256.  RB is chosen on the host so that the grid covers the chip once.
//
// The reset mask (`PolicyMemory.reset(dones)`) is applied WHERE THE OPERAND IS LOADED: h and c of the previous step are read as
// where(done, 0, .) by every workgroup that needs them and the buffers themselves are never rewritten, so no workgroup reads what another
// writes in the same launch.  The new raw state goes to the other ping-pong buffer.  The workgroups of unit tile 0 also copy the masked
// pre-step state of their row block into the storage slot (`saved_hidden_states`).
//
// Arithmetic: v_mfma_f32_16x16x4_f32, exact f32 products, f32 accumulation, k blocks in index order (x side first, then h) dealt to four
// partial sums that are added pairwise: one fixed order, no atomics.  Operand trick as lt_lstm.hip: MFMA step s of a 16-wide k block consumes the k-set {kb + 4 q + s}, so lane (i, q)
// supplies component s of ONE 16-byte load.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "lt_env.h"
#include "lt_internal.h"
#include "lt_memory.h"
#include "lt_memory_seq.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { const float e = __expf(-2.f * fabsf(x)); const float t = (1.f - e) / (1.f + e); return x < 0.f ? -t : t; }

struct NetArgs {
  const float* x; const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; const float* h_in; const float* c_in;
  float* h_out; float* c_out; float* saved_h; float* saved_c;
  int I, IP, KP;  // IP: I rounded up to 16 (the x side's k blocks; the panel holds zeros in [I, IP)); KP: LDS row stride in floats
};
struct StepArgs { NetArgs net[2]; const uint8_t* dones; int N, H, RB; };

constexpr int kLdsBytes = 160 * 1024;

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// LDS row stride: IP + H + 8 is an odd multiple of 8 floats (IP, H multiples of 16): the 16 lanes of a ds_read_b128 lane group (rows
// {0-3, 12-15} at one q, rows 4-11 at the next) then start at 16 distinct multiples of 4 banks
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
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int MT> __device__ __forceinline__ void load_units(const float* __restrict__ src, float* dst) {
  if constexpr (MT == 4) { const f32x4 v = *(const f32x4*)src; dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3]; }
  else { const f32x2 v = *(const f32x2*)src; dst[0] = v[0]; dst[1] = v[1]; }
}
template <int MT> __device__ __forceinline__ void store_units(float* __restrict__ dst, const float* src) {
  if constexpr (MT == 4) *(f32x4*)dst = (f32x4){src[0], src[1], src[2], src[3]};
  else *(f32x2*)dst = (f32x2){src[0], src[1]};
}

// TRAIN (lt_memory_seq_forward, the update): the activated gates i, f, g, o of every (row, unit) also go to `gates` ([N][4H] per network,
// PyTorch's order) - what the backward pass reads.  The rollout's kernels are the !TRAIN instantiations: their arguments and code are
// what they were before the parameter existed.
struct SeqStepArgs : StepArgs { float* gates[2]; };

template <int UT, bool TRAIN = false>  // UT: hidden units per workgroup, 16 or 8
__global__ __launch_bounds__(256) void lt_memory_step_kernel(const std::conditional_t<TRAIN, SeqStepArgs, StepArgs> a) {
  constexpr int MT = UT / 4;  // 16-row MFMA tiles of the panel; lane (n, g) of the D layout owns units g * MT .. + MT - 1 of its row
  extern __shared__ __attribute__((aligned(16))) float panel[];  // [4 UT][KP]
  const NetArgs& p = a.net[blockIdx.z];
  const int N = a.N, H = a.H, I = p.I, IP = p.IP, KP = p.KP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * UT;
  const int r0 = blockIdx.y * a.RB;
  const int r1 = min(N, r0 + a.RB);

  // ---- 1. the weight panel, once.  Panel row pr = 16 mt + 4 g + v holds gate v of unit j0 + g * MT + mt: [W_ih row | 0 | W_hh row]
  for (int idx = tid; idx < 4 * UT * IP; idx += 256) {
    const int pr = idx / IP, k = idx - pr * IP;
    const int unit = j0 + ((pr >> 2) & 3) * MT + (pr >> 4), wrow = (pr & 3) * H + unit;
    panel[pr * KP + k] = k < I ? p.w_ih[(long long)wrow * I + k] : 0.f;
  }
  const int h4 = H / 4;
  for (int idx = tid; idx < 4 * UT * h4; idx += 256) {
    const int pr = idx / h4, k4 = idx - pr * h4;
    const int unit = j0 + ((pr >> 2) & 3) * MT + (pr >> 4), wrow = (pr & 3) * H + unit;
    *(f32x4*)(panel + pr * KP + IP + 4 * k4) = *(const f32x4*)(p.w_hh + (long long)wrow * H + 4 * k4);
  }

  // ---- the masked pre-step state of this row block -> the storage slot (unit tile 0 alone; every element of the slot's rows)
  if (blockIdx.x == 0) {
    for (int idx = tid; idx < (r1 - r0) * h4; idx += 256) {
      const int r = r0 + idx / h4;
      const long long o = (long long)r * H + 4 * (idx % h4);
      const bool done = a.dones && a.dones[r] != 0;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(p.saved_h + o) = done ? z : *(const f32x4*)(p.h_in + o);
      *(f32x4*)(p.saved_c + o) = done ? z : *(const f32x4*)(p.c_in + o);
    }
  }

  // ---- the biases of this lane's units (lane (n, g): units j0 + g * MT + mt, gate v), b_ih + b_hh
  float bias[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int wrow = v * H + j0 + q * MT + mt;
      bias[mt][v] = p.b_ih[wrow] + p.b_hh[wrow];
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
    // the epilogue's operand, requested now: c of (row, units j0 + q * MT .. + MT - 1)
    float cp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) cp[mt] = 0.f;
    if (!done) load_units<MT>(p.c_in + (long long)rc * H + j0 + q * MT, cp);
    // four partial sums per gate (k block b goes to chain b % 4), added pairwise at the end: chains of K / 4 terms round less than one of
    // K terms - measured, one chain was twice as far from f64 as the eager composition, whose four waves split K - and four independent
    // MFMA chains per tile never wait for the 40-cycle dependent latency
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
    // ---- 3. epilogue: sum[v] of lane (n, g) is D[4 g + v][n] = gate v of unit j0 + g * MT + mt, row n
    if (!row_ok) continue;
    float hn[MT], cn[MT];
    [[maybe_unused]] float act[4][MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 sum = (acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt]);
      const float gi = sigmoidf_(sum[0] + bias[mt][0]);
      const float gf = sigmoidf_(sum[1] + bias[mt][1]);
      const float gg = tanhf_(sum[2] + bias[mt][2]);
      const float go = sigmoidf_(sum[3] + bias[mt][3]);
      cn[mt] = gf * cp[mt] + gi * gg;
      hn[mt] = go * tanhf_(cn[mt]);
      if constexpr (TRAIN) { act[0][mt] = gi; act[1][mt] = gf; act[2][mt] = gg; act[3][mt] = go; }
    }
    const long long o = (long long)row * H + j0 + q * MT;
    store_units<MT>(p.h_out + o, hn);
    store_units<MT>(p.c_out + o, cn);
    if constexpr (TRAIN) {
      float* g = a.gates[blockIdx.z] + (long long)row * 4 * H + j0 + q * MT;
#pragma unroll
      for (int v = 0; v < 4; ++v) store_units<MT>(g + v * H, act[v]);
    }
  }
}


// out = where(dones, 0, raw) for the four state arrays; grid (ceil(N H / 4 / 256), 4 arrays)
struct FinishArgs { const float* in[4]; float* out[4]; const uint8_t* dones; int N, H; };

__global__ __launch_bounds__(256) void lt_memory_finish_kernel(const FinishArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // one float4
  const int h4 = a.H / 4;
  if (idx >= (long long)a.N * h4) return;
  const int r = (int)(idx / h4);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!(a.dones && a.dones[r] != 0)) v = *(const f32x4*)(a.in[blockIdx.y] + 4 * idx);
  *(f32x4*)(a.out[blockIdx.y] + 4 * idx) = v;
}

// ---- lt_memory_seq_backward --------------------------------------------------------------------------------------------------------
// The recurrent GEMM of the backward pass at the update's shape (E rows of an env block, more than 1000): dh = dgates[t+1] W_hh, an
// [E x 4H] . [4H x H] product, K = 4H.  The plan is the forward kernel's, transposed: a workgroup owns UB = 16 MT OUTPUT units and a row
// block of RB rows;
//   1. its W_hh panel - COLUMNS k0 .. k0 + UB - 1 of W_hh, stored as rows [UB][4H + 8] - is staged into LDS once (H = 512: 16 units,
//      128.5 KiB; H = 256: 32 units; H <= 128: 64 units where the grid still covers the chip);
//   2. the four waves walk the row block in 16-row sub-tiles; the B operand (dgates[t+1] rows) comes straight from global memory, one
//      16-byte load per lane and 16-wide k block, double-buffered in groups of four; the A operand is one ds_read_b128 per M tile and k
//      block (the row stride 4H + 8 is an odd multiple of 8 floats, as the forward panel's);
//   3. the gate gradients of step t are the epilogue, in registers: panel row 16 mt + 4 g + v holds unit k0 + 4 MT g + 4 mt + v, so lane
//      (n, g) of the D layout owns 4 MT CONSECUTIVE units of row n - 16-byte accesses, no LDS round trip, no dh array.
// Sum order: k blocks in index order dealt to four partial sums (block b to chain b % 4), added pairwise - whatever UB and RB are.
// The dc carry [E][H] is read and rewritten by the lane that owns the element.  dones[t] cuts the recursion: a done row takes neither
// the GEMM's result nor the carry (the state behind a done is a constant zero).
struct BwdNet {
  const float* w_hh; const float* dg_next; const float* dout; const float* cell; const float* gates; const float* c_prev;
  float* dg; float* dc;
};
struct BwdArgs { BwdNet net[2]; const uint8_t* dones; int E, H, RB; };

// The gate gradients of four consecutive units of one row (lt_lstm.hip's formula; tanh(c_t) recomputed): reads gates / cell / c_prev /
// dout at element offset o of [E][H] (gates: row * 4H + unit), writes dgates and the new carry dc_t * f_t.
struct GradOps { f32x4 dout, ct, cp, g[4]; };

__device__ __forceinline__ GradOps load_grad_ops(const BwdNet& p, long long row, int unit, int H) {
  GradOps e;
  const long long o = row * H + unit;
  e.dout = *(const f32x4*)(p.dout + o);
  e.ct = *(const f32x4*)(p.cell + o);
  e.cp = *(const f32x4*)(p.c_prev + o);
#pragma unroll
  for (int v = 0; v < 4; ++v) e.g[v] = *(const f32x4*)(p.gates + row * 4 * H + v * H + unit);
  return e;
}

__device__ __forceinline__ void store_gate_grads(const BwdNet& p, long long row, int unit, int H, const GradOps& e, f32x4 dh_next, f32x4 dc_in) {
  f32x4 d[4], dc;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float dh = e.dout[v] + dh_next[v];
    const float tc = tanhf_(e.ct[v]);
    const float gi = e.g[0][v], gf = e.g[1][v], gg = e.g[2][v], go = e.g[3][v];
    const float dcv = dc_in[v] + dh * go * (1.f - tc * tc);
    d[0][v] = dcv * gg * gi * (1.f - gi);
    d[1][v] = dcv * e.cp[v] * gf * (1.f - gf);
    d[2][v] = dcv * gi * (1.f - gg * gg);
    d[3][v] = dh * tc * go * (1.f - go);
    dc[v] = dcv * gf;
  }
  float* g = p.dg + row * 4 * H + unit;
#pragma unroll
  for (int v = 0; v < 4; ++v) *(f32x4*)(g + v * H) = d[v];
  *(f32x4*)(p.dc + row * H + unit) = dc;
}

// opens the recursion at t = T - 1: dh = dout, no carry.  grid (ceil(E H / 4 / 256), 2 networks)
__global__ __launch_bounds__(256) void lt_memory_seq_bwd_open_kernel(const BwdArgs a) {
  const BwdNet& p = a.net[blockIdx.y];
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // four units of one row
  const int h4 = a.H / 4;
  if (idx >= (long long)a.E * h4) return;
  const long long row = idx / h4;
  const int unit = 4 * (int)(idx - row * h4);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  store_gate_grads(p, row, unit, a.H, load_grad_ops(p, row, unit, a.H), z, z);
}

__host__ __device__ inline int bwd_panel_stride(int H) { return 4 * H + 8; }

template <int MT>  // 16-unit MFMA tiles per workgroup: 4, 2 or 1
__global__ __launch_bounds__(256) void lt_memory_seq_bwd_kernel(const BwdArgs a) {
  constexpr int UB = 16 * MT;
  extern __shared__ __attribute__((aligned(16))) float panel[];  // [UB][KP]
  const BwdNet& p = a.net[blockIdx.z];
  const int E = a.E, H = a.H, K = 4 * H, KP = bwd_panel_stride(H);
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
  const int nblk = K / 16;  // a multiple of 16 (H is one of 64): whole groups of four k blocks
  const int nsub = (r1 - r0 + 15) / 16;
  for (int s = wave; s < nsub; s += 4) {
    const int row = r0 + 16 * s + i;
    const bool row_ok = row < r1;
    const int rc = row_ok ? row : r0;  // (a clamped lane computes a column of D nobody stores)
    const float* grow = p.dg_next + (long long)rc * K + 4 * q;
    // the epilogue's operands, requested now: (row, units k0 + 4 MT q .. + 4 MT - 1) of step t
    const int unit0 = k0 + 4 * MT * q;
    const bool done = a.dones && a.dones[rc] != 0;
    GradOps ops[MT];
    f32x4 dc_in[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      ops[mt] = load_grad_ops(p, rc, unit0 + 4 * mt, H);
      dc_in[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (!done) dc_in[mt] = *(const f32x4*)(p.dc + (long long)rc * H + unit0 + 4 * mt);
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
      f32x4 sum = (acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt]);
      if (done) sum = (f32x4){0.f, 0.f, 0.f, 0.f};
      store_gate_grads(p, row, unit0 + 4 * mt, H, ops[mt], sum, dc_in[mt]);
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

int check_sizes(const char* fn, int N, int H) {
  if (N < 1 || N > 16 * 65535) return refuse(fn, "", "N", "in [1, 16 * 65535]");
  if (H < 64 || H > 512 || (H % 64) != 0) return refuse(fn, "", "H", "a multiple of 64 in [64, 512]");
  return LT_OK;
}

int check_net(const char* fn, const char* who, const lt_memory_net* n, int H) {
  if (!n) return refuse(fn, who, "", "non-null");
  if (n->I < 1 || n->I + H > 1248) return refuse(fn, who, ".I", "at least 1 with I + H <= 1248");
  const struct { const char* name; const void* p; int align; } ptrs[] = {
      {".x", n->x, 4}, {".w_ih", n->w_ih, 4}, {".w_hh", n->w_hh, 16}, {".b_ih", n->b_ih, 16}, {".b_hh", n->b_hh, 16}, {".h_in", n->h_in, 16},
      {".c_in", n->c_in, 16}, {".h_out", n->h_out, 16}, {".c_out", n->c_out, 16}, {".saved_h", n->saved_h, 16}, {".saved_c", n->saved_c, 16}};
  for (const auto& e : ptrs)
    if (!e.p || (uintptr_t)e.p % e.align != 0) return refuse(fn, who, e.name, e.align == 16 ? "non-null and 16-byte aligned" : "non-null and 4-byte aligned");
  if (n->h_out == n->h_in || n->c_out == n->c_in) return refuse(fn, who, ".h_out / .c_out", "another buffer than .h_in / .c_in (ping-pong)");
  return LT_OK;
}

NetArgs net_args(const lt_memory_net* n, int H) {
  NetArgs r;
  r.x = n->x; r.w_ih = n->w_ih; r.w_hh = n->w_hh; r.b_ih = n->b_ih; r.b_hh = n->b_hh; r.h_in = n->h_in; r.c_in = n->c_in;
  r.h_out = n->h_out; r.c_out = n->c_out; r.saved_h = n->saved_h; r.saved_c = n->saved_c;
  r.I = n->I; r.IP = round_up(n->I, 16); r.KP = panel_stride(n->I, H);
  return r;
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
  if (E < 1 || E > 16 * 65535) return refuse(fn, "", "E", "in [1, 16 * 65535]");
  if (H < 64 || H > 512 || (H % 64) != 0) return refuse(fn, "", "H", "a multiple of 64 in [64, 512]");
  if (dones && dones_stride < E) return refuse(fn, "", "dones_stride", "at least E");
  return LT_OK;
}

struct seq_ptr { const char* name; const void* p; int align; long long floats; };  // floats > 0: an output of that many elements

bool overlaps(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}

int check_seq_net(const char* fn, const char* who, const lt_memory_seq_net* n, const lt_memory_seq_net* other, int T, int E, int H) {
  if (!n) return refuse(fn, who, "", "non-null");
  if (n->I < 1 || n->I + H > 1248) return refuse(fn, who, ".I", "at least 1 with I + H <= 1248");
  if (n->x_stride < (int64_t)E * n->I) return refuse(fn, who, ".x_stride", "at least E * I");
  const long long EH = (long long)E * H, TEH = (long long)T * EH;
  const seq_ptr ptrs[] = {{".x", n->x, 4, 0}, {".w_ih", n->w_ih, 4, 0}, {".w_hh", n->w_hh, 16, 0}, {".b_ih", n->b_ih, 16, 0}, {".b_hh", n->b_hh, 16, 0},
                          {".h0", n->h0, 16, 0}, {".c0", n->c0, 16, 0}, {".out", n->out, 16, TEH}, {".cell", n->cell, 16, TEH},
                          {".gates", n->gates, 16, 4 * TEH}, {".h_prev", n->h_prev, 16, TEH}, {".c_prev", n->c_prev, 16, TEH}};
  for (const auto& e : ptrs)
    if (!e.p || (uintptr_t)e.p % e.align != 0) return refuse(fn, who, e.name, e.align == 16 ? "non-null and 16-byte aligned" : "non-null and 4-byte aligned");
  for (const auto& e : ptrs) {
    if (e.floats == 0) continue;
    for (const lt_memory_seq_net* m : {n, other})
      if (m && ((m->h0 && overlaps(e.p, e.floats, m->h0, EH)) || (m->c0 && overlaps(e.p, e.floats, m->c0, EH))))
        return refuse(fn, who, e.name, "a buffer that does not overlap h0 / c0 of either network");
  }
  return LT_OK;
}

int check_seq_grad(const char* fn, const char* who, const lt_memory_seq_grad* n) {
  if (!n) return refuse(fn, who, "", "non-null");
  const struct { const char* name; const void* p; } ptrs[] = {{".dout", n->dout}, {".w_hh", n->w_hh}, {".cell", n->cell}, {".gates", n->gates},
                                                             {".c_prev", n->c_prev}, {".dgates", n->dgates}, {".dc_carry", n->dc_carry}};
  for (const auto& e : ptrs)
    if (!e.p || (uintptr_t)e.p % 16 != 0) return refuse(fn, who, e.name, "non-null and 16-byte aligned");
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

}  // namespace

extern "C" {

int lt_memory_step(const lt_memory_net* actor, const lt_memory_net* critic, const uint8_t* dones, int N, int H, void* stream) {
  const char* fn = "lt_memory_step";
  if (const int rc = check_sizes(fn, N, H)) return rc;
  if (const int rc = check_net(fn, "actor", actor, H)) return rc;
  if (const int rc = check_net(fn, "critic", critic, H)) return rc;
  StepArgs a;
  a.net[0] = net_args(actor, H);
  a.net[1] = net_args(critic, H);
  a.dones = dones; a.N = N; a.H = H;
  int ut, lds;
  const dim3 grid = step_plan(a, ut, lds);
  const void* kernel = ut == 16 ? (const void*)lt_memory_step_kernel<16> : (const void*)lt_memory_step_kernel<8>;
  if (const int e = lt_ensure_dynamic_lds(kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  if (ut == 16) hipLaunchKernelGGL(lt_memory_step_kernel<16>, grid, dim3(256), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(lt_memory_step_kernel<8>, grid, dim3(256), lds, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  return LT_OK;
}

int lt_memory_finish(const float* h_a, const float* c_a, const float* h_c, const float* c_c, const uint8_t* dones, int N, int H,
                     float* out_h_a, float* out_c_a, float* out_h_c, float* out_c_c, void* stream) {
  const char* fn = "lt_memory_finish";
  if (const int rc = check_sizes(fn, N, H)) return rc;
  const struct { const char* name; const void* p; } ptrs[] = {{"h_a", h_a}, {"c_a", c_a}, {"h_c", h_c}, {"c_c", c_c}, {"out_h_a", out_h_a},
                                                             {"out_c_a", out_c_a}, {"out_h_c", out_h_c}, {"out_c_c", out_c_c}};
  for (const auto& e : ptrs)
    if (!e.p || (uintptr_t)e.p % 16 != 0) return refuse(fn, "", e.name, "non-null and 16-byte aligned");
  FinishArgs a;
  a.in[0] = h_a; a.in[1] = c_a; a.in[2] = h_c; a.in[3] = c_c;
  a.out[0] = out_h_a; a.out[1] = out_c_a; a.out[2] = out_h_c; a.out[3] = out_c_c;
  a.dones = dones; a.N = N; a.H = H;
  const long long n4 = (long long)N * (H / 4);
  hipLaunchKernelGGL(lt_memory_finish_kernel, dim3((unsigned)((n4 + 255) / 256), 4), dim3(256), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  return LT_OK;
}

int lt_memory_seq_forward(const lt_memory_seq_net* actor, const lt_memory_seq_net* critic, const uint8_t* dones, int64_t dones_stride,
                          int T, int E, int H, void* stream) {
  const char* fn = "lt_memory_seq_forward";
  if (const int rc = check_seq_sizes(fn, T, E, H, dones, dones_stride)) return rc;
  if (const int rc = check_seq_net(fn, "actor", actor, critic, T, E, H)) return rc;
  if (const int rc = check_seq_net(fn, "critic", critic, actor, T, E, H)) return rc;
  const lt_memory_seq_net* nets[2] = {actor, critic};
  SeqStepArgs a;
  for (int k = 0; k < 2; ++k) {
    NetArgs& r = a.net[k];
    const lt_memory_seq_net* n = nets[k];
    r.w_ih = n->w_ih; r.w_hh = n->w_hh; r.b_ih = n->b_ih; r.b_hh = n->b_hh;
    r.I = n->I; r.IP = round_up(n->I, 16); r.KP = panel_stride(n->I, H);
  }
  a.N = E; a.H = H;
  int ut, lds;
  const dim3 grid = step_plan(a, ut, lds);
  const void* kernel = ut == 16 ? (const void*)lt_memory_step_kernel<16, true> : (const void*)lt_memory_step_kernel<8, true>;
  if (const int e = lt_ensure_dynamic_lds(kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  const long long EH = (long long)E * H;
  for (int t = 0; t < T; ++t) {
    for (int k = 0; k < 2; ++k) {
      NetArgs& r = a.net[k];
      const lt_memory_seq_net* n = nets[k];
      r.x = n->x + t * n->x_stride;
      r.h_in = t == 0 ? n->h0 : n->out + (t - 1) * EH;
      r.c_in = t == 0 ? n->c0 : n->cell + (t - 1) * EH;
      r.h_out = n->out + t * EH; r.c_out = n->cell + t * EH;
      r.saved_h = n->h_prev + t * EH; r.saved_c = n->c_prev + t * EH;
      a.gates[k] = n->gates + 4 * t * EH;
    }
    a.dones = dones && t > 0 ? dones + (t - 1) * dones_stride : nullptr;
    if (ut == 16) hipLaunchKernelGGL((lt_memory_step_kernel<16, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((lt_memory_step_kernel<8, true>), grid, dim3(256), lds, (hipStream_t)stream, a);
  }
  return launch_status();
}

int lt_memory_seq_backward_units(int E, int H) {
  if (E < 1 || E > 16 * 65535 || H < 64 || H > 512 || (H % 64) != 0) return 0;
  return bwd_units(E, H);
}

int lt_memory_seq_backward(const lt_memory_seq_grad* actor, const lt_memory_seq_grad* critic, const uint8_t* dones, int64_t dones_stride,
                           int T, int E, int H, void* stream) {
  const char* fn = "lt_memory_seq_backward";
  if (const int rc = check_seq_sizes(fn, T, E, H, dones, dones_stride)) return rc;
  if (const int rc = check_seq_grad(fn, "actor", actor)) return rc;
  if (const int rc = check_seq_grad(fn, "critic", critic)) return rc;
  const lt_memory_seq_grad* nets[2] = {actor, critic};
  const int kp = bwd_panel_stride(H);
  const int ub = bwd_units(E, H);
  const int rb = row_block(E, 2 * (H / ub));
  const int lds = ub * kp * (int)sizeof(float);
  const void* kernel = ub == 64 ? (const void*)lt_memory_seq_bwd_kernel<4> : ub == 32 ? (const void*)lt_memory_seq_bwd_kernel<2> : (const void*)lt_memory_seq_bwd_kernel<1>;
  if (T > 1)
    if (const int e = lt_ensure_dynamic_lds(kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  const long long EH = (long long)E * H;
  BwdArgs a;
  a.E = E; a.H = H; a.RB = rb; a.dones = nullptr;
  auto at = [&](int t) {
    for (int k = 0; k < 2; ++k) {
      BwdNet& r = a.net[k];
      const lt_memory_seq_grad* n = nets[k];
      r.w_hh = n->w_hh; r.dg_next = t + 1 < T ? n->dgates + 4 * (t + 1) * EH : nullptr;
      r.dout = n->dout + t * EH; r.cell = n->cell + t * EH; r.gates = n->gates + 4 * t * EH; r.c_prev = n->c_prev + t * EH;
      r.dg = n->dgates + 4 * t * EH; r.dc = n->dc_carry;
    }
  };
  at(T - 1);
  hipLaunchKernelGGL(lt_memory_seq_bwd_open_kernel, dim3((unsigned)((EH / 4 + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream, a);
  const dim3 grid((unsigned)(H / ub), (unsigned)((E + rb - 1) / rb), 2);
  for (int t = T - 2; t >= 0; --t) {
    at(t);
    a.dones = dones ? dones + t * dones_stride : nullptr;
    switch (ub) {
      case 64: hipLaunchKernelGGL(lt_memory_seq_bwd_kernel<4>, grid, dim3(256), lds, (hipStream_t)stream, a); break;
      case 32: hipLaunchKernelGGL(lt_memory_seq_bwd_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, a); break;
      default: hipLaunchKernelGGL(lt_memory_seq_bwd_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, a); break;
    }
  }
  return launch_status();
}

}  // extern "C"
