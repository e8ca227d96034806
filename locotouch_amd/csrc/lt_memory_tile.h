// The row-block GEMM skeleton of the memory kernels, once: lt_memory.hip (LSTM) and lt_memory_gru.hip (GRU) instantiate it with a `Cell`,
// a stateless struct of constants and `static __device__ __forceinline__` functions that holds everything cell-specific:
//   step kernel      NS (state tensors: 2 = h, c; 1 = h; the epilogue's operand is the LAST one), ih_gate(v) / hh_gate(v) (which gate row
//                    of w_ih / w_hh panel row kind v = 0..3 of a unit holds) and ih_used(v) / hh_used(v) (false: that side of the row
//                    is zeros), load_bias, gates (the epilogue's arithmetic)
//   backward kernel  KG (K = KG H gate columns), BwdNet (with the fields w_hh, dg_next, carry), GradOps, load_grad_ops, store_gate_grads
// The two cells live in lt_memory_cells.h.  Internal to the translation units that include it: everything is in an unnamed namespace.
//
// Step kernel.  Shape: B = num_envs rows (4096 and up), K = I + H (observation width + hidden size), four panel rows per hidden unit, two
// networks.  lt_lstm.hip's step kernel is laid out for the update (B ~ 47: a 16 x 16 tile per workgroup, weights streamed once per tile);
// at the rollout's shape that re-reads all of W_hh once per 16 rows and leaves the input GEMM to a library call.  Here a workgroup owns UT
// hidden units (4 UT rows of [W_ih | W_hh]) and a ROW BLOCK of RB rows:
//   1. the weight panel [4 UT][I + H] is staged into LDS ONCE (UT = 16: 64 rows, up to 160 KiB; UT = 8 when that does not fit);
//   2. the four waves walk the row block in 16-row sub-tiles (wave w takes sub-tiles w, w + 4, ...): the B operand (x_t | h rows) comes
//      straight from global memory, one 16-byte load per lane and 16-wide k block, double-buffered in groups of four blocks; the A
//      operand is one ds_read_b128 per M tile and k block; 4 UT / 16 MFMA tiles share each B load;
//   3. the gate arithmetic is the epilogue, in registers: the M index of a tile is 4 * g + v, so lane (n, g) of the D layout holds the
//      four sums of ONE unit of row n - no LDS round trip, no second launch.
// grid (H / UT, ceil(N / RB), 2 networks), block 256.  RB is chosen on the host so that the grid covers the chip once.
//
// The reset mask (`PolicyMemory.reset(dones)`) is applied WHERE THE OPERAND IS LOADED: the state of the previous step is read as
// where(done, 0, .) by every workgroup that needs it and the buffers themselves are never rewritten, so no workgroup reads what another
// writes in the same launch.  The new raw state goes to the other ping-pong buffer.  The workgroups of unit tile 0 also copy the masked
// pre-step state of their row block into the storage slot (`saved_hidden_states`).
//
// Arithmetic: v_mfma_f32_16x16x4_f32, exact f32 products, f32 accumulation, k blocks in index order (x side first, then h) dealt to four
// partial sums that are added pairwise: one fixed order, no atomics.  Operand trick as lt_seq_tile.h: MFMA step s of a 16-wide k block
// consumes the k-set {kb + 4 q + s}, so lane (i, q) supplies component s of ONE 16-byte load.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "lt_device_prims.h"
#include "lt_env.h"
#include "lt_host_check.h"
#include "lt_internal.h"

namespace {

using lt::f32x4;
using lt::sigmoidf_;
using lt::tanhf_;
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int NS> struct NetArgs {
  const float* x; const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; const float* s_in[NS];
  float* s_out[NS]; float* saved[NS];
  long long XS;    // floats between two x rows (I: contiguous rows; more: the rows are columns of wider ones, include/lt_rnn_encoder.h)
  int I, IP, KP;  // IP: I rounded up to 16 (the x side's k blocks; the panel holds zeros in [I, IP)); KP: LDS row stride in floats
};
template <int NS> struct StepArgs { NetArgs<NS> net[2]; const uint8_t* dones; int N, H, RB; };
// TRAIN (the sequence forward of the update): the four `act` values of every (row, unit) also go to `gates` ([N][4H] per network, four
// planes of H) - what the backward pass reads.  The rollout's kernels are the !TRAIN instantiations, without the argument and its code.
template <int NS> struct SeqStepArgs : StepArgs<NS> { float* gates[2]; };
template <class Cell, bool TRAIN> using step_args = std::conditional_t<TRAIN, SeqStepArgs<Cell::NS>, StepArgs<Cell::NS>>;

constexpr int kLdsBytes = 160 * 1024;

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The IEEE quotient (v_div_scale / v_div_fmas / v_div_fixup): the build's -freciprocal-math turns `/` - and `__fdiv_rn`, which this
// toolchain defines as `/` - into a multiplication by v_rcp_f32, one ulp off where torch's normaliser is not.
__device__ __forceinline__ float ieee_div(float a, float b) {
#pragma clang fp reciprocal(off)
  return a / b;
}

// LDS row stride: IP + H + 8 is an odd multiple of 8 floats (IP, H multiples of 16): the 16 lanes of a ds_read_b128 lane group (rows
// {0-3, 12-15} at one q, rows 4-11 at the next) then start at 16 distinct multiples of 4 banks
__host__ __device__ inline int panel_stride(int I, int H) { return round_up(I, 16) + H + 8; }

// The B operand of k block `blk` for lane (row, q): x[row][16 blk + 4 q .. + 3] (zeros past I; rows are only 4-byte aligned unless
// `xvec`: x, I and the row stride all multiples of 16 bytes), or behind the x side's blocks where(done, 0, h[row][...]).
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

template <class Cell, int UT, bool TRAIN = false>  // UT: hidden units per workgroup, 16 or 8
__global__ __launch_bounds__(256) void lt_memory_step_kernel(const step_args<Cell, TRAIN> a) {
  constexpr int MT = UT / 4;  // 16-row MFMA tiles of the panel; lane (n, g) of the D layout owns units g * MT .. + MT - 1 of its row
  constexpr int NS = Cell::NS;
  extern __shared__ __attribute__((aligned(16))) float panel[];  // [4 UT][KP]
  const NetArgs<NS>& p = a.net[blockIdx.z];
  const int N = a.N, H = a.H, I = p.I, IP = p.IP, KP = p.KP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * UT;
  const int r0 = blockIdx.y * a.RB;
  const int r1 = min(N, r0 + a.RB);

  // ---- 1. the weight panel, once.  Panel row pr = 16 mt + 4 g + v holds row kind v of unit j0 + g * MT + mt: [W_ih row | 0 | W_hh row],
  // either side the gate row the cell names or zeros
  for (int idx = tid; idx < 4 * UT * IP; idx += 256) {
    const int pr = idx / IP, k = idx - pr * IP, v = pr & 3;
    const int unit = j0 + ((pr >> 2) & 3) * MT + (pr >> 4), wrow = Cell::ih_gate(v) * H + unit;
    panel[pr * KP + k] = Cell::ih_used(v) && k < I ? p.w_ih[(long long)wrow * I + k] : 0.f;
  }
  const int h4 = H / 4;
  for (int idx = tid; idx < 4 * UT * h4; idx += 256) {
    const int pr = idx / h4, k4 = idx - pr * h4, v = pr & 3;
    const int unit = j0 + ((pr >> 2) & 3) * MT + (pr >> 4), wrow = Cell::hh_gate(v) * H + unit;
    f32x4 w = {0.f, 0.f, 0.f, 0.f};
    if (Cell::hh_used(v)) w = *(const f32x4*)(p.w_hh + (long long)wrow * H + 4 * k4);
    *(f32x4*)(panel + pr * KP + IP + 4 * k4) = w;
  }

  // ---- the masked pre-step state of this row block -> the storage slot (unit tile 0 alone; every element of the slot's rows)
  if (blockIdx.x == 0) {
    for (int idx = tid; idx < (r1 - r0) * h4; idx += 256) {
      const int r = r0 + idx / h4;
      const long long o = (long long)r * H + 4 * (idx % h4);
      const bool done = a.dones && a.dones[r] != 0;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(p.saved[0] + o) = done ? z : *(const f32x4*)(p.s_in[0] + o);
      if constexpr (NS == 2) *(f32x4*)(p.saved[1] + o) = done ? z : *(const f32x4*)(p.s_in[1] + o);
    }
  }

  // ---- the four biases of this lane's units (lane (n, g): units j0 + g * MT + mt; the cell adds the three parts of the index itself)
  float bias[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) Cell::load_bias(p.b_ih, p.b_hh, H, j0, q * MT, mt, bias[mt]);
  __syncthreads();

  // ---- 2. the row block, 16 rows per wave and pass
  const int xblks = IP / 16, nblk = xblks + H / 16;
  const bool xvec = (I & 3) == 0 && (p.XS & 3) == 0 && ((uintptr_t)p.x & 15) == 0;
  const int nsub = (r1 - r0 + 15) / 16;
  for (int s = wave; s < nsub; s += 4) {
    const int row = r0 + 16 * s + i;  // the row this lane feeds as the B operand, and (n = i) the row it owns in the epilogue
    const bool row_ok = row < r1;
    const int rc = row_ok ? row : r0;  // (a clamped lane computes a column of D nobody stores)
    const bool done = a.dones && a.dones[rc] != 0;
    const float* xrow = p.x + (long long)rc * p.XS;
    const float* hrow = p.s_in[0] + (long long)rc * H;
    // the epilogue's operand, requested now: the last state tensor at (row, units j0 + q * MT .. + MT - 1)
    float prev[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) prev[mt] = 0.f;
    if (!done) load_units<MT>(p.s_in[NS - 1] + (long long)rc * H + j0 + q * MT, prev);
    // four partial sums per panel row (k block b goes to chain b % 4), added pairwise at the end: chains of K / 4 terms round less than
    // one of K terms - measured, one chain was twice as far from f64 as the eager composition, whose four waves split K - and four
    // independent MFMA chains per tile never wait for the 40-cycle dependent latency
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
    float next[NS][MT];
    [[maybe_unused]] float act[4][MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 sum = (acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt]);
      float sn[NS], ga[4];
      Cell::gates(sum, bias[mt], prev[mt], sn, ga);
#pragma unroll
      for (int k = 0; k < NS; ++k) next[k][mt] = sn[k];
      if constexpr (TRAIN) { act[0][mt] = ga[0]; act[1][mt] = ga[1]; act[2][mt] = ga[2]; act[3][mt] = ga[3]; }
    }
    const long long o = (long long)row * H + j0 + q * MT;
    store_units<MT>(p.s_out[0] + o, next[0]);
    if constexpr (NS == 2) store_units<MT>(p.s_out[1] + o, next[1]);
    if constexpr (TRAIN) {
      float* g = a.gates[blockIdx.z] + (long long)row * 4 * H + j0 + q * MT;
#pragma unroll
      for (int v = 0; v < 4; ++v) store_units<MT>(g + v * H, act[v]);
    }
  }
}

// out = where(dones, 0, raw) for NA state arrays; grid (ceil(N H / 4 / 256), NA arrays)
template <int NA> struct FinishArgs { const float* in[NA]; float* out[NA]; const uint8_t* dones; int N, H; };

template <int NA> __global__ __launch_bounds__(256) void lt_memory_finish_kernel(const FinishArgs<NA> a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // one float4
  const int h4 = a.H / 4;
  if (idx >= (long long)a.N * h4) return;
  const int r = (int)(idx / h4);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!(a.dones && a.dones[r] != 0)) v = *(const f32x4*)(a.in[blockIdx.y] + 4 * idx);
  *(f32x4*)(a.out[blockIdx.y] + 4 * idx) = v;
}

// ---- the backward pass over a rollout ------------------------------------------------------------------------------------------------
// The recurrent GEMM of the backward pass at the update's shape (E rows of an env block, more than 1000): dh = dg[t+1] W_hh, an
// [E x K] . [K x H] product, K = KG H (the cell's dg has KG gate planes per row).  The plan is the forward kernel's, transposed: a
// workgroup owns UB = 16 MT OUTPUT units and a row block of RB rows;
//   1. its W_hh panel - COLUMNS k0 .. k0 + UB - 1 of W_hh, stored as rows [UB][K + 8] - is staged into LDS once (LSTM, H = 512: 16
//      units, 128.5 KiB; H = 256: 32 units; H <= 128: 64 units where the grid still covers the chip);
//   2. the four waves walk the row block in 16-row sub-tiles; the B operand (dg[t+1] rows) comes straight from global memory, one
//      16-byte load per lane and 16-wide k block, double-buffered in groups of four; the A operand is one ds_read_b128 per M tile and k
//      block (the row stride K + 8 is an odd multiple of 8 floats, as the forward panel's: H is a multiple of 64);
//   3. the gate gradients of step t are the epilogue, in registers: panel row 16 mt + 4 g + v holds unit k0 + 4 MT g + 4 mt + v, so lane
//      (n, g) of the D layout owns 4 MT CONSECUTIVE units of row n - 16-byte accesses, no LDS round trip, no dh array.
// Sum order: k blocks in index order dealt to four partial sums (block b to chain b % 4), added pairwise - whatever UB and RB are.
// The carry [E][H] is read and rewritten by the lane that owns the element.  dones[t] cuts the recursion: a done row takes neither the
// GEMM's result nor the carry (the state behind a done is a constant zero).  The carry reaches the cell already masked; how the sum is
// masked and joins it is the cell's: Cell::store_gate_grads(net, row, unit, H, ops, sum, carry, done).
template <class Cell> struct BwdArgs { typename Cell::BwdNet net[2]; const uint8_t* dones; int E, H, RB; };

// opens the recursion at t = T - 1: dh = dout, no carry.  grid (ceil(E H / 4 / 256), 2 networks)
template <class Cell> __global__ __launch_bounds__(256) void lt_memory_seq_bwd_open_kernel(const BwdArgs<Cell> a) {
  const typename Cell::BwdNet& p = a.net[blockIdx.y];
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // four units of one row
  const int h4 = a.H / 4;
  if (idx >= (long long)a.E * h4) return;
  const long long row = idx / h4;
  const int unit = 4 * (int)(idx - row * h4);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  Cell::store_gate_grads(p, row, unit, a.H, Cell::load_grad_ops(p, row, unit, a.H), z, z, false);
}

__host__ __device__ inline int bwd_panel_stride(int KG, int H) { return KG * H + 8; }

template <class Cell, int MT>  // 16-unit MFMA tiles per workgroup: 4, 2 or 1
__global__ __launch_bounds__(256) void lt_memory_seq_bwd_kernel(const BwdArgs<Cell> a) {
  constexpr int UB = 16 * MT;
  extern __shared__ __attribute__((aligned(16))) float panel[];  // [UB][KP]
  const typename Cell::BwdNet& p = a.net[blockIdx.z];
  const int E = a.E, H = a.H, K = Cell::KG * H, KP = bwd_panel_stride(Cell::KG, H);
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
  const int nblk = K / 16;  // 4 KG (H / 64): whole groups of four k blocks
  const int nsub = (r1 - r0 + 15) / 16;
  for (int s = wave; s < nsub; s += 4) {
    const int row = r0 + 16 * s + i;
    const bool row_ok = row < r1;
    const int rc = row_ok ? row : r0;  // (a clamped lane computes a column of D nobody stores)
    const float* grow = p.dg_next + (long long)rc * K + 4 * q;
    // the epilogue's operands, requested now: (row, units k0 + 4 MT q .. + 4 MT - 1) of step t
    const int unit0 = k0 + 4 * MT * q;
    const bool done = a.dones && a.dones[rc] != 0;
    typename Cell::GradOps ops[MT];
    f32x4 carry[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      ops[mt] = Cell::load_grad_ops(p, rc, unit0 + 4 * mt, H);
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
      const f32x4 sum = (acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt]);
      Cell::store_gate_grads(p, row, unit0 + 4 * mt, H, ops[mt], sum, carry[mt], done);
    }
  }
}

// ---- host side: validation before anything is launched (refuse, check_ptr(s), launch_status: lt_host_check.h) -------------------------
int check_sizes(const char* fn, const char* rows, int N, int H) {
  if (N < 1 || N > 16 * 65535) return refuse(fn, "", rows, "in [1, 16 * 65535]");
  if (H < 64 || H > 512 || (H % 64) != 0) return refuse(fn, "", "H", "a multiple of 64 in [64, 512]");
  return LT_OK;
}

int check_seq_sizes(const char* fn, int T, int E, int H, const uint8_t* dones, int64_t dones_stride) {
  if (T < 1) return refuse(fn, "", "T", "at least 1");
  if (const int rc = check_sizes(fn, "E", E, H)) return rc;
  if (dones && dones_stride < E) return refuse(fn, "", "dones_stride", "at least E");
  return LT_OK;
}

// what the check of every step / sequence net struct opens with: the struct is there and its width fits the panel
template <class Net> int check_net_head(const char* fn, const char* who, const Net* n, int H) {
  if (!n) return refuse(fn, who, "", "non-null");
  if (n->I < 1 || n->I + H > 1248) return refuse(fn, who, ".I", "at least 1 with I + H <= 1248");
  return LT_OK;
}

bool overlaps(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
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
template <int NS> dim3 step_plan(StepArgs<NS>& a, int& ut, int& lds) {
  const int kp = a.net[0].KP > a.net[1].KP ? a.net[0].KP : a.net[1].KP;
  ut = 64 * kp * (int)sizeof(float) <= kLdsBytes ? 16 : 8;  // 32 x 1280 floats fill the LDS exactly: I + H <= 1248 always fits
  lds = 4 * ut * kp * (int)sizeof(float);
  a.RB = row_block(a.N, 2 * (a.H / ut));
  return dim3((unsigned)(a.H / ut), (unsigned)((a.N + a.RB - 1) / a.RB), 2);
}

// output units per workgroup of the backward step: the widest panel (64, 32 or 16 columns of W_hh) that fits the LDS and still leaves
// the grid at least half a workgroup per CU (64-row passes), else narrower.  The choice moves work between workgroups, never a sum's order.
int bwd_units(int E, int H, int panel_stride) {
  int ub = 16;
  for (const int cand : {64, 32, 16}) {
    if (cand * panel_stride * (int)sizeof(float) > kLdsBytes) continue;
    const int tiles = 2 * (H / cand);
    const int rb = row_block(E, tiles);
    ub = cand;
    if (2LL * tiles * ((E + rb - 1) / rb) >= cu_count()) break;
  }
  return ub;
}

// the value behind lt_memory_*_seq_backward_units: 0 where the entry point would refuse E or H
int bwd_units_or_zero(int E, int H, int KG) {
  if (E < 1 || E > 16 * 65535 || H < 64 || H > 512 || (H % 64) != 0) return 0;
  return bwd_units(E, H, bwd_panel_stride(KG, H));
}

// ---- host side: launches ------------------------------------------------------------------------------------------------------------
template <class A> using kernel_fn = void (*)(A);

// allows a panel kernel the whole LDS as dynamic shared memory (set once per kernel and device)
template <class A> int allow_lds(kernel_fn<A> kernel) {
  if (const int e = lt_ensure_dynamic_lds((const void*)kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  return LT_OK;
}

// the weights and widths of one network (every net struct of the three headers names them alike)
template <int NS, class Net> void set_weights(NetArgs<NS>& r, const Net* n, int H) {
  r.w_ih = n->w_ih; r.w_hh = n->w_hh; r.b_ih = n->b_ih; r.b_hh = n->b_hh;
  r.I = n->I; r.IP = round_up(n->I, 16); r.KP = panel_stride(n->I, H); r.XS = n->I;
}

// T step launches of one plan: picks the unit tile for a (weights, N and H set), allows its kernel the LDS, then `at(t)` puts step t's
// pointers and dones into `a` in front of launch t
template <class Cell, bool TRAIN, class At> int launch_steps(step_args<Cell, TRAIN>& a, int T, void* stream, At at) {
  int ut, lds;
  const dim3 grid = step_plan<Cell::NS>(a, ut, lds);
  const kernel_fn<step_args<Cell, TRAIN>> kernel = ut == 16 ? lt_memory_step_kernel<Cell, 16, TRAIN> : lt_memory_step_kernel<Cell, 8, TRAIN>;
  if (const int rc = allow_lds(kernel)) return rc;
  for (int t = 0; t < T; ++t) {
    at(t);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, (hipStream_t)stream, a);
  }
  return launch_status();
}

template <int NA> int launch_finish(const char* fn, const char* const (&names)[2 * NA], const float* const (&in)[NA], float* const (&out)[NA],
                                    const uint8_t* dones, int N, int H, void* stream) {
  if (const int rc = check_sizes(fn, "N", N, H)) return rc;
  for (int k = 0; k < 2 * NA; ++k)
    if (const int rc = check_ptr(fn, "", {names[k], k < NA ? (const void*)in[k] : (const void*)out[k - NA], 16})) return rc;
  FinishArgs<NA> a;
  for (int k = 0; k < NA; ++k) { a.in[k] = in[k]; a.out[k] = out[k]; }
  a.dones = dones; a.N = N; a.H = H;
  const long long n4 = (long long)N * (H / 4);
  hipLaunchKernelGGL(lt_memory_finish_kernel<NA>, dim3((unsigned)((n4 + 255) / 256), NA), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status();
}

// The backward pass over T steps: picks the panel width, allows its kernel the LDS, one pointwise launch opens the recursion at
// t = T - 1, then one GEMM launch per step t = T - 2 .. 0.  `net_at(k, t)` gives network k's operands of step t.
template <class Cell, class NetAt> int launch_backward(const uint8_t* dones, int64_t dones_stride, int T, int E, int H, void* stream, NetAt net_at) {
  const int kp = bwd_panel_stride(Cell::KG, H);
  const int ub = bwd_units(E, H, kp);
  const int rb = row_block(E, 2 * (H / ub));
  const int lds = ub * kp * (int)sizeof(float);
  const kernel_fn<BwdArgs<Cell>> kernel = ub == 64 ? lt_memory_seq_bwd_kernel<Cell, 4> : ub == 32 ? lt_memory_seq_bwd_kernel<Cell, 2> : lt_memory_seq_bwd_kernel<Cell, 1>;
  if (T > 1)
    if (const int rc = allow_lds(kernel)) return rc;
  BwdArgs<Cell> a;
  a.E = E; a.H = H; a.RB = rb; a.dones = nullptr;
  for (int k = 0; k < 2; ++k) a.net[k] = net_at(k, T - 1);
  hipLaunchKernelGGL(lt_memory_seq_bwd_open_kernel<Cell>, dim3((unsigned)(((long long)E * H / 4 + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream, a);
  const dim3 grid((unsigned)(H / ub), (unsigned)((E + rb - 1) / rb), 2);
  for (int t = T - 2; t >= 0; --t) {
    for (int k = 0; k < 2; ++k) a.net[k] = net_at(k, t);
    a.dones = dones ? dones + t * dones_stride : nullptr;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, (hipStream_t)stream, a);
  }
  return launch_status();
}

}  // namespace
