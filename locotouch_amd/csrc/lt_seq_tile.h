// The step-kernel skeleton of the whole-trajectory recurrences, once: lt_lstm.hip and lt_gru.hip instantiate it with a `Cell`, a stateless
// struct of constants and `static __device__ __forceinline__` functions that holds everything cell-specific:
//   NG   gate planes of a row of `ig` and of the gate gradients the backward GEMM reduces over: the forward kernel's accumulators and the
//        backward kernel's K = NG H (LSTM 4, GRU 3)
//   NS   state tensors (LSTM 2 = h, c; GRU 1 = h); the forward epilogue's operand is the LAST one.  NS == 2: the carry of the backward
//        pass is the gradient of the second state (dc); NS == 1: it is a part of dh and joins the GEMM's sum
//   gates(ig, bi, bh, sum, prev, next, act)       one element of the forward epilogue: the NG sums -> the new state(s) and the four saved `ws`
//   gate_grads(dh, carry, w, after, before, d)    one element of the backward epilogue: the four gate gradients `d`; returns the new carry
//   store_grads<T>(dg, dg_in, row, unit, H, d)    where the four `d` of (row, unit .. + sizeof(T) / 4 - 1) go
// The kernels take the union of the two cells' arrays as plain `__restrict__` pointers (a by-value struct of them cost registers and an
// occupancy step in the fused backward kernel); what a cell does not have (NS == 1: c, c_out, s_after, dc0; the LSTM: dg_in) is NULL
// and never touched.
// The memory kernels (lt_memory_tile.h) are the same idea at the rollout's shape; their cells associate the forward formulas differently,
// so the two sets of cells stay apart.
//
// The recurrence is L dependent steps of one small GEMM ([B, H] x [H, NG H]) and a gate formula.  A step is ONE launch whose grid covers
// the chip: a workgroup owns a 16 x 16 (hidden unit x batch row) tile, its four waves split the reduction (K = H forward, NG H backward)
// and meet in LDS, and the gate arithmetic is wave 0's epilogue.  The time loops run on the host side of the C ABI (seq_forward /
// seq_backward below): no Python between steps.
// Arithmetic: v_mfma_f32_16x16x4_f32, exact f32 products, f32 accumulation; a wave adds its k-blocks in index order, wave 0 adds the four
// waves' partials in wave order: one fixed order, no atomics, the same bits on every run.
//
// Operand trick: a 16 x 16 x 4 MFMA wants lane (i = l % 16, q = l / 16) to supply A[i][k0 + q] and B[k0 + q][n = i].  Summation over k
// is order-free, so MFMA step s of a 16-wide k block consumes the k-set {kb + 4 q + s}: lane (i, q) then supplies component s of ONE
// float4 load A[i][kb + 4q .. + 3] - 16-byte loads, four MFMAs per load.
//
// The epilogue's operands are requested BEFORE the GEMM: wave 0's lane (n, g) owns units 4 g .. + 3 of batch row n of the tile, and what
// it needs there (this step's input-gate pre-activations - first touch, HBM -, biases, the previous state; backward: the carry, dout and
// the saved gates of the previous step) is loaded first, so the round trip overlaps the GEMM instead of following it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lt_device_prims.h"
#include "lt_env.h"
#include "lt_host_check.h"
#include "lt_internal.h"

namespace {

using lt::f32x4;
using lt::mfma_16x16x4;
using lt::sigmoidf_;
using lt::tanhf_;

// ---- forward step: s' = Cell(ig_t, s) for a 16-unit x 16-row tile; ws = what the backward pass reads back (four planes of H per row) --
// grid (H / 16, ceil(B / 16)), block 256 (4 waves, wave w reduces k in [w * H / 4, (w + 1) * H / 4)); NG accumulators, one per gate:
// gate g's rows of w_hh start at g * H * H.
// KB > 0: H = 64 KB known at compile time - the wave's KB k-blocks are fully unrolled so that all (1 + NG) KB operand loads (16 bytes
// each) are in flight before the first MFMA; with a runtime trip count every k-block exposed an L2 round trip (GRU: 9.0 us per step at
// H = 512 against ~2 us of loads + MFMAs).  KB == 0: any H that is a multiple of 64.
template <class Cell, int KB>
__global__ __launch_bounds__(256) void lt_seq_step_fwd(const float* __restrict__ ig, const float* __restrict__ h, const float* __restrict__ c,
                                                       const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                       const float* __restrict__ b_hh, float* __restrict__ h_out, float* __restrict__ c_out,
                                                       float* __restrict__ ws, int B, int H_rt) {
  constexpr int NG = Cell::NG, NS = Cell::NS;
  const int H = KB > 0 ? 64 * KB : H_rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int row = b0 + i;  // batch row this lane feeds as the B operand
  const bool row_ok = row < B;
  const float* hrow = h + (long long)(row_ok ? row : 0) * H;
  const float* wr = w_hh + (long long)(j0 + i) * H;  // A operand rows: unit j0 + i of gate 0; + g * H * H for gate g
  const long long gate = (long long)H * H;
  f32x4 acc[NG] = {};
  // epilogue lanes (wave 0): lane (n, g) owns units j0 + 4 g .. + 3 of batch row b0 + n; their operands are requested NOW
  const int be = b0 + (lane & 15), je = j0 + 4 * (lane >> 4);
  const bool ep = wave == 0 && be < B;
  f32x4 e_ig[NG], e_bi[NG], e_bh[NG], e_prev;
  if (ep) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      e_ig[g] = *(const f32x4*)(ig + (long long)be * NG * H + g * H + je);
      e_bi[g] = *(const f32x4*)(b_ih + g * H + je);
      e_bh[g] = *(const f32x4*)(b_hh + g * H + je);
    }
    e_prev = *(const f32x4*)((NS == 2 ? c : h) + (long long)be * H + je);
  }
  const int kq = H / 4, k_begin = wave * kq, k_end = k_begin + kq;
  if constexpr (KB > 0) {
    f32x4 hv[KB], wv[KB][NG];
#pragma unroll
    for (int it = 0; it < KB; ++it) {
      const int k = k_begin + 16 * it + 4 * q;
      hv[it] = *(const f32x4*)(hrow + k);
#pragma unroll
      for (int g = 0; g < NG; ++g) wv[it][g] = *(const f32x4*)(wr + g * gate + k);
    }
    lt::sched_fence();  // keep every load above the first MFMA (the scheduler would re-serialise them to save registers)
#pragma unroll
    for (int it = 0; it < KB; ++it) {
      if (!row_ok) hv[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = mfma_16x16x4(wv[it][g][s], hv[it][s], acc[g]);
    }
  } else {
    for (int kb = k_begin; kb < k_end; kb += 16) {
      const int k = kb + 4 * q;
      f32x4 hv = *(const f32x4*)(hrow + k), wv[NG];
      if (!row_ok) hv = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < NG; ++g) wv[g] = *(const f32x4*)(wr + g * gate + k);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = mfma_16x16x4(wv[g][s], hv[s], acc[g]);
    }
  }
  // D layout: acc[v] of lane (n = l % 16, g = l / 16) is D[unit 4 g + v][row n]
  __shared__ float red[NG][4][4][64];  // [gate][wave][v][lane]
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int g = 0; g < NG; ++g) red[g][wave][v][lane] = acc[g][v];
  __syncthreads();
  if (!ep) return;
  f32x4 o_s[NS], o_w[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    float gi[NG], bi[NG], bh[NG], sum[NG], next[NS], act[4];
#pragma unroll
    for (int g = 0; g < NG; ++g) sum[g] = red[g][0][v][lane] + red[g][1][v][lane] + red[g][2][v][lane] + red[g][3][v][lane];
#pragma unroll
    for (int g = 0; g < NG; ++g) { gi[g] = e_ig[g][v]; bi[g] = e_bi[g][v]; bh[g] = e_bh[g][v]; }
    Cell::gates(gi, bi, bh, sum, e_prev[v], next, act);
#pragma unroll
    for (int k = 0; k < NS; ++k) o_s[k][v] = next[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) o_w[k][v] = act[k];
  }
  const long long o = (long long)be * H + je;
  *(f32x4*)(h_out + o) = o_s[0];
  if constexpr (NS == 2) *(f32x4*)(c_out + o) = o_s[1];
  float* w = ws + (long long)be * 4 * H + je;
#pragma unroll
  for (int k = 0; k < 4; ++k) *(f32x4*)(w + k * H) = o_w[k];
}

// ---- backward, opening the recursion: the gate gradients of the LAST step from dh' = dout_{L-1} + dhn and, NS == 2, dc' = dcn (each may
// be NULL = 0).  Pointwise, grid ceil(B * H / 256).  ws, s_after (NS == 2), s_before: the saved gates of that step and the last state
// tensor after / before it; writes the gate gradients (dg [B][NG H]: the hidden side, the first fused launch's operand; dg_in: the
// input side where the cell keeps one) and the carry [B][H].
template <class Cell>
__global__ __launch_bounds__(256) void lt_seq_step_bwd_open(const float* __restrict__ dout, const float* __restrict__ dhn, const float* __restrict__ dcn,
                                                            const float* __restrict__ ws, const float* __restrict__ s_after,
                                                            const float* __restrict__ s_before, float* __restrict__ dg, float* __restrict__ dg_in,
                                                            float* __restrict__ carry, int B, int H) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)B * H) return;
  const int b = (int)(idx / H), j = (int)(idx - (long long)b * H);
  const float* wb = ws + (long long)b * 4 * H;
  const float w[4] = {wb[j], wb[H + j], wb[2 * H + j], wb[3 * H + j]};
  const float dh = dout[idx] + (dhn ? dhn[idx] : 0.f);
  float d[4];
  carry[idx] = Cell::gate_grads(dh, dcn ? dcn[idx] : 0.f, w, Cell::NS == 2 ? s_after[idx] : 0.f, s_before[idx], d);
  Cell::template store_grads<float>(dg, dg_in, b, j, H, d);
}

// ---- backward step, recurrent part + the PREVIOUS step's pointwise part ------------------------------------------------------------
// dh_prev = dg_t W_hh for a 16-k x 16-row tile, then - same lanes, same (row, unit) elements - the gate gradients of step t - 1 from
// dh' = dout_{t-1} + dh_prev and the carry (what lt_seq_step_bwd_open computes for the last step): one launch per backward step.
// `carry` is read and rewritten element-wise by its owning lane; NS == 1: it is the direct part of dh_prev and joins the sum first.
// grid (H / 16, ceil(B / 16)), block 256 (wave w reduces j in [w * NG H / 4, (w + 1) * NG H / 4)).  t == 0 (dout_prev NULL): writes
// dh0 (and, NS == 2, dc0) instead.
// KB > 0 -> H = 64 KB, the wave's NG KB j-blocks unrolled in groups of 8 with their loads issued first (the GRU's 3 KB leaves a partial
// last group at H = 128 and 256; with the LSTM's 4 KB the guard folds away).
template <class Cell, int KB>
__global__ __launch_bounds__(256) void lt_seq_step_bwd_fused(const float* __restrict__ dg_t, const float* __restrict__ w_hh, float* __restrict__ carry,
                                                             const float* __restrict__ dout_prev, const float* __restrict__ ws_prev,
                                                             const float* __restrict__ s_after, const float* __restrict__ s_before,
                                                             float* __restrict__ dg_prev, float* __restrict__ dg_in_prev, float* __restrict__ dh0,
                                                             float* __restrict__ dc0, int B, int H_rt) {
  constexpr int NG = Cell::NG, NS = Cell::NS;
  const int H = KB > 0 ? 64 * KB : H_rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int k0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int row = b0 + i;
  const bool row_ok = row < B;
  const float* grow = dg_t + (long long)(row_ok ? row : 0) * NG * H;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // epilogue operands of wave 0's lanes (row b0 + n, units k0 + 4 g .. + 3), requested before the GEMM
  const int be = b0 + (lane & 15), je = k0 + 4 * (lane >> 4);
  const bool ep = wave == 0 && be < B;
  f32x4 e_carry, e_dout, e_after, e_before, e_w[4];
  if (ep) {
    const long long o = (long long)be * H + je;
    e_carry = *(const f32x4*)(carry + o);
    if (dout_prev) {
      e_dout = *(const f32x4*)(dout_prev + o);
      if constexpr (NS == 2) e_after = *(const f32x4*)(s_after + o);
      e_before = *(const f32x4*)(s_before + o);
#pragma unroll
      for (int k = 0; k < 4; ++k) e_w[k] = *(const f32x4*)(ws_prev + (long long)be * 4 * H + k * H + je);
    }
  }
  const int jq = NG * H / 4, j_begin = wave * jq, j_end = j_begin + jq;
  // A operand: A[out = k0 + i][reduction index j + s] = W[j + s][k0 + i]  (16 consecutive k across the lanes of one q: coalesced)
  if constexpr (KB > 0) {
    constexpr int G = 8;                        // j-blocks per group: 8 x (4 + 4) operand registers in flight
    constexpr bool WHOLE = (NG * KB) % G == 0;  // no partial last group: the guards below are gone before the optimiser sees them
#pragma unroll
    for (int it0 = 0; it0 < NG * KB; it0 += G) {
      f32x4 gv[G], wv[G];
#pragma unroll
      for (int u = 0; u < G; ++u) {
        if (WHOLE || it0 + u < NG * KB) {
          const int j = j_begin + 16 * (it0 + u) + 4 * q;
          gv[u] = *(const f32x4*)(grow + j);
          const float* wp = w_hh + (long long)j * H + k0 + i;
          wv[u] = (f32x4){wp[0], wp[H], wp[2 * (long long)H], wp[3 * (long long)H]};
        }
      }
      lt::sched_fence();  // loads of the group first, then its MFMAs
#pragma unroll
      for (int u = 0; u < G; ++u) {
        if (WHOLE || it0 + u < NG * KB) {
          if (!row_ok) gv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = mfma_16x16x4(wv[u][s], gv[u][s], acc);
        }
      }
    }
  } else {
    for (int jb = j_begin; jb < j_end; jb += 16) {
      const int j = jb + 4 * q;
      f32x4 gv = *(const f32x4*)(grow + j);
      if (!row_ok) gv = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* wp = w_hh + (long long)j * H + k0 + i;
      const f32x4 wv = {wp[0], wp[H], wp[2 * (long long)H], wp[3 * (long long)H]};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma_16x16x4(wv[s], gv[s], acc);
    }
  }
  __shared__ float red[4][4][64];
#pragma unroll
  for (int v = 0; v < 4; ++v) red[wave][v][lane] = acc[v];
  __syncthreads();
  if (!ep) return;
  f32x4 dhp;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    if constexpr (NS == 1) dhp[v] = e_carry[v] + red[0][v][lane] + red[1][v][lane] + red[2][v][lane] + red[3][v][lane];
    else dhp[v] = red[0][v][lane] + red[1][v][lane] + red[2][v][lane] + red[3][v][lane];
  }
  const long long o = (long long)be * H + je;
  if (!dout_prev) {  // t == 0
    *(f32x4*)(dh0 + o) = dhp;
    if constexpr (NS == 2) *(f32x4*)(dc0 + o) = e_carry;
    return;
  }
  f32x4 d[4], d_carry;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float w[4] = {e_w[0][v], e_w[1][v], e_w[2][v], e_w[3][v]};
    float dv[4];
    d_carry[v] = Cell::gate_grads(e_dout[v] + dhp[v], e_carry[v], w, NS == 2 ? e_after[v] : 0.f, e_before[v], dv);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k][v] = dv[k];
  }
  Cell::template store_grads<f32x4>(dg_prev, dg_in_prev, be, je, H, d);
  *(f32x4*)(carry + o) = d_carry;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// LT_OK, or LT_EINVAL with "<fn>: invalid argument: <what>".  Pointers first (a float4 moves 16 bytes: alignment is part of the
// contract), then the sizes (B: the grid's y limit).
template <int n> int check_seq_args(const char* fn, const ptr_check (&ptrs)[n], int L, int B, int H) {
  if (const int rc = check_ptrs(fn, "", ptrs)) return rc;
  if (L < 1) return refuse(fn, "", "L", "at least 1");
  if (B < 1 || B > 16 * 65535) return refuse(fn, "", "B", "in [1, 16 * 65535]");
  if (H < 64 || (H % 64) != 0) return refuse(fn, "", "H", "a multiple of 64");
  return LT_OK;
}

// the instantiation of a step kernel template for H: the student's encoder is H = 512; the other compile-time sizes cover the usual
// powers of two
#define LT_SEQ_KERNEL_FOR(kernel, Cell, H) \
  ((H) == 512 ? kernel<Cell, 8> : (H) == 256 ? kernel<Cell, 4> : (H) == 128 ? kernel<Cell, 2> : kernel<Cell, 0>)

// L forward launches.  ig [L][B][NG H]; h0, c0: the initial state [B][H]; out, cell: the state of every step [L][B][H] (outputs);
// ws [L][B][4H] (output).  NS == 1: c0 and cell are NULL.
template <class Cell>
int seq_forward(const float* ig, const float* h0, const float* c0, const float* w_hh, const float* b_ih, const float* b_hh, int L, int B, int H,
                float* out, float* cell, float* ws, void* stream) {
  const dim3 grid((unsigned)(H / 16), (unsigned)((B + 15) / 16));
  const long long BH = (long long)B * H;
  const auto kernel = LT_SEQ_KERNEL_FOR(lt_seq_step_fwd, Cell, H);
  const float* h = h0;
  const float* c = c0;
  for (int t = 0; t < L; ++t) {
    float* ht = out + t * BH;
    float* ct = cell ? cell + t * BH : nullptr;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, ig + t * Cell::NG * BH, h, c, w_hh, b_ih, b_hh, ht, ct, ws + t * 4 * BH, B, H);
    h = ht;
    c = ct;
  }
  return launch_status();
}

// The backward pass: launch t = L opens the recursion, launches t = L - 1 .. 0 are the fused steps; launch t forms the gate gradients of
// step u = t - 1 (t == 0: none - it leaves dh0 / dc0).  s0 / s_seq: the LAST state tensor as seq_forward read / left it (LSTM: c0, cell;
// GRU: h0, out); dg, dg_in [L][B][NG H] (outputs; dg_in NULL where the cell keeps none); scratch [B][H]: the carry.
template <class Cell>
int seq_backward(const float* dout, const float* dhn, const float* dcn, const float* s0, const float* s_seq, const float* ws, const float* w_hh,
                 int L, int B, int H, float* dg, float* dg_in, float* scratch, float* dh0, float* dc0, void* stream) {
  const dim3 grid((unsigned)(H / 16), (unsigned)((B + 15) / 16));
  const long long BH = (long long)B * H;
  const auto kernel = LT_SEQ_KERNEL_FOR(lt_seq_step_bwd_fused, Cell, H);
  for (int t = L; t >= 0; --t) {
    const int u = t - 1;
    const bool none = u < 0;
    const float* dout_u = none ? nullptr : dout + u * BH;
    const float* ws_u = none ? nullptr : ws + u * 4 * BH;
    const float* after = none || Cell::NS == 1 ? nullptr : s_seq + u * BH;        // the state AFTER step u
    const float* before = none ? nullptr : (u > 0 ? s_seq + (u - 1) * BH : s0);  // the state BEFORE step u
    float* dg_u = none ? nullptr : dg + u * Cell::NG * BH;
    float* dg_in_u = none || !dg_in ? nullptr : dg_in + u * Cell::NG * BH;
    if (t == L)
      hipLaunchKernelGGL(lt_seq_step_bwd_open<Cell>, dim3((unsigned)((BH + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dout_u, dhn, dcn, ws_u, after,
                         before, dg_u, dg_in_u, scratch, B, H);
    else
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, dg + t * Cell::NG * BH, w_hh, scratch, dout_u, ws_u, after, before, dg_u,
                         dg_in_u, dh0, dc0, B, H);
  }
  return launch_status();
}

}  // namespace
