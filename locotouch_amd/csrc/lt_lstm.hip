// Single-layer LSTM over a padded batch of whole trajectories (include/lt_lstm.h): the recurrence of `Memory` / `PolicyMemory` with
// rnn_type "lstm" (reference loco_rl/loco_rl/models/memory_module.py:6 -> nn.LSTM; the default of ActorCriticRecurrent).
//
// The plan is lt_gru.hip's.  The recurrence is L dependent steps of one small GEMM ([B, H] x [H, 4H]) and a gate formula; a step is ONE
// launch whose grid covers the chip: a workgroup owns a 16 x 16 (hidden unit x batch row) tile, its four waves split the reduction
// (K = H forward, 4H backward - a wave per gate) and meet in LDS, and the gate arithmetic is the epilogue.  The time loop runs on the
// host side of the C ABI (lt_lstm_forward / lt_lstm_backward): no Python between steps.
// Arithmetic: v_mfma_f32_16x16x4_f32, exact f32 products, f32 accumulation; a wave adds its k-blocks in index order, wave 0 adds the
// four waves' partials in wave order: one fixed order, no atomics, the same bits on every run.
//
// Operand trick (as lt_gru.hip): a 16 x 16 x 4 MFMA wants lane (i = l % 16, q = l / 16) to supply A[i][k0 + q] and B[k0 + q][n = i].
// Summation over k is order-free, so MFMA step s of a 16-wide k block consumes the k-set {kb + 4 q + s}: lane (i, q) then supplies
// component s of ONE float4 load A[i][kb + 4q .. + 3] - 16-byte loads, four MFMAs per load.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "lt_device_prims.h"
#include "lt_env.h"
#include "lt_internal.h"
#include "lt_lstm.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

using lt::sigmoidf_;
using lt::tanhf_;

// ---- forward step: (h', c') = LSTM(ig_t, h, c) for a 16-unit x 16-row tile; ws = the activated gates (i, f, g, o) ------------------
// grid (H / 16, ceil(B / 16)), block 256 (4 waves, wave w reduces k in [w * H / 4, (w + 1) * H / 4)); four accumulators, one per gate.
// KB > 0: H = 64 KB known at compile time - the wave's KB k-blocks are fully unrolled so that all 5 KB operand loads (16 bytes each)
// are in flight before the first MFMA.  KB == 0: any H that is a multiple of 64.
template <int KB>
__global__ __launch_bounds__(256) void lt_lstm_step_fwd(const float* __restrict__ ig, const float* __restrict__ h, const float* __restrict__ c,
                                                        const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                        const float* __restrict__ b_hh, float* __restrict__ h_out, float* __restrict__ c_out,
                                                        float* __restrict__ ws, int B, int H_rt) {
  const int H = KB > 0 ? 64 * KB : H_rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int row = b0 + i;                       // batch row this lane feeds as the B operand
  const bool row_ok = row < B;
  const float* hrow = h + (long long)(row_ok ? row : 0) * H;
  const float* wr = w_hh + (long long)(j0 + i) * H;  // A operand rows: unit j0 + i of gate i; + H*H, + 2*H*H, + 3*H*H for f, g, o
  const long long gate = (long long)H * H;
  f32x4 acc_i = {0.f, 0.f, 0.f, 0.f}, acc_f = acc_i, acc_g = acc_i, acc_o = acc_i;
  // epilogue lanes (wave 0): lane (n, g) owns units j0 + 4 g .. + 3 of batch row b0 + n.  Their operands (this step's input-gate
  // pre-activations - first touch, HBM -, biases, c) are requested NOW, so the round trip overlaps the GEMM instead of following it.
  const int be = b0 + (lane & 15), je = j0 + 4 * (lane >> 4);
  const bool ep = wave == 0 && be < B;
  f32x4 e_ig[4], e_bi[4], e_bh[4], e_cp;
  if (ep) {
#pragma unroll
    for (int gt = 0; gt < 4; ++gt) {
      e_ig[gt] = *(const f32x4*)(ig + (long long)be * 4 * H + gt * H + je);
      e_bi[gt] = *(const f32x4*)(b_ih + gt * H + je);
      e_bh[gt] = *(const f32x4*)(b_hh + gt * H + je);
    }
    e_cp = *(const f32x4*)(c + (long long)be * H + je);
  }
  const int kq = H / 4, k_begin = wave * kq, k_end = k_begin + kq;
  if (KB > 0) {
    f32x4 hv[KB > 0 ? KB : 1], wiv[KB > 0 ? KB : 1], wfv[KB > 0 ? KB : 1], wgv[KB > 0 ? KB : 1], wov[KB > 0 ? KB : 1];
#pragma unroll
    for (int it = 0; it < KB; ++it) {
      const int k = k_begin + 16 * it + 4 * q;
      hv[it] = *(const f32x4*)(hrow + k);
      wiv[it] = *(const f32x4*)(wr + k); wfv[it] = *(const f32x4*)(wr + gate + k);
      wgv[it] = *(const f32x4*)(wr + 2 * gate + k); wov[it] = *(const f32x4*)(wr + 3 * gate + k);
    }
    __builtin_amdgcn_sched_barrier(0);  // keep every load above the first MFMA (the scheduler would re-serialise them to save registers)
#pragma unroll
    for (int it = 0; it < KB; ++it) {
      if (!row_ok) hv[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc_i = __builtin_amdgcn_mfma_f32_16x16x4f32(wiv[it][s], hv[it][s], acc_i, 0, 0, 0);
        acc_f = __builtin_amdgcn_mfma_f32_16x16x4f32(wfv[it][s], hv[it][s], acc_f, 0, 0, 0);
        acc_g = __builtin_amdgcn_mfma_f32_16x16x4f32(wgv[it][s], hv[it][s], acc_g, 0, 0, 0);
        acc_o = __builtin_amdgcn_mfma_f32_16x16x4f32(wov[it][s], hv[it][s], acc_o, 0, 0, 0);
      }
    }
  } else {
    for (int kb = k_begin; kb < k_end; kb += 16) {
      const int k = kb + 4 * q;
      f32x4 hv = *(const f32x4*)(hrow + k);
      if (!row_ok) hv = (f32x4){0.f, 0.f, 0.f, 0.f};
      const f32x4 wiv = *(const f32x4*)(wr + k), wfv = *(const f32x4*)(wr + gate + k);
      const f32x4 wgv = *(const f32x4*)(wr + 2 * gate + k), wov = *(const f32x4*)(wr + 3 * gate + k);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc_i = __builtin_amdgcn_mfma_f32_16x16x4f32(wiv[s], hv[s], acc_i, 0, 0, 0);
        acc_f = __builtin_amdgcn_mfma_f32_16x16x4f32(wfv[s], hv[s], acc_f, 0, 0, 0);
        acc_g = __builtin_amdgcn_mfma_f32_16x16x4f32(wgv[s], hv[s], acc_g, 0, 0, 0);
        acc_o = __builtin_amdgcn_mfma_f32_16x16x4f32(wov[s], hv[s], acc_o, 0, 0, 0);
      }
    }
  }
  // D layout: acc[v] of lane (n = l % 16, g = l / 16) is D[unit 4 g + v][row n]
  __shared__ float red[4][4][4][64];  // [gate][wave][v][lane]
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    red[0][wave][v][lane] = acc_i[v]; red[1][wave][v][lane] = acc_f[v]; red[2][wave][v][lane] = acc_g[v]; red[3][wave][v][lane] = acc_o[v];
  }
  __syncthreads();
  if (!ep) return;
  f32x4 o_h, o_c, o_i, o_f, o_g, o_o;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    float s[4];
#pragma unroll
    for (int gt = 0; gt < 4; ++gt) s[gt] = red[gt][0][v][lane] + red[gt][1][v][lane] + red[gt][2][v][lane] + red[gt][3][v][lane];
    const float gi = sigmoidf_(e_ig[0][v] + e_bi[0][v] + s[0] + e_bh[0][v]);
    const float gf = sigmoidf_(e_ig[1][v] + e_bi[1][v] + s[1] + e_bh[1][v]);
    const float gg = tanhf_(e_ig[2][v] + e_bi[2][v] + s[2] + e_bh[2][v]);
    const float go = sigmoidf_(e_ig[3][v] + e_bi[3][v] + s[3] + e_bh[3][v]);
    const float cn = gf * e_cp[v] + gi * gg;
    o_c[v] = cn; o_h[v] = go * tanhf_(cn);
    o_i[v] = gi; o_f[v] = gf; o_g[v] = gg; o_o[v] = go;
  }
  const long long o = (long long)be * H + je;
  *(f32x4*)(h_out + o) = o_h;
  *(f32x4*)(c_out + o) = o_c;
  float* w = ws + (long long)be * 4 * H + je;
  *(f32x4*)w = o_i; *(f32x4*)(w + H) = o_f; *(f32x4*)(w + 2 * H) = o_g; *(f32x4*)(w + 3 * H) = o_o;
}

// The gate gradients of one (row, unit) element of one step from dh' = dout_t + dh_next and the dc carry; returns the new dc carry.
// tanh(c_t) is recomputed (one exp) instead of stored and read back.
__device__ __forceinline__ float lstm_gate_grads(float dh, float dc_in, float gi, float gf, float gg, float go, float ct, float cp, float& dai,
                                                 float& daf, float& dag, float& dao) {
  const float tc = tanhf_(ct);
  const float dc = dc_in + dh * go * (1.f - tc * tc);
  dai = dc * gg * gi * (1.f - gi);
  daf = dc * cp * gf * (1.f - gf);
  dag = dc * gi * (1.f - gg * gg);
  dao = dh * tc * go * (1.f - go);
  return dc * gf;
}

// ---- backward, opening the recursion: gate gradients of the LAST step from dh' = dout_{L-1} + dhn and dc' = dcn -------------------
// grid ceil(B * H / 256); writes dgates_{L-1} [B, 4H] and the dc carry [B, H]
__global__ __launch_bounds__(256) void lt_lstm_step_bwd_gates(const float* __restrict__ dout, const float* __restrict__ dhn,
                                                              const float* __restrict__ dcn, const float* __restrict__ ws,
                                                              const float* __restrict__ cell, const float* __restrict__ c_prev,
                                                              float* __restrict__ dgates, float* __restrict__ dc_carry, int B, int H) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)B * H) return;
  const int b = (int)(idx / H), j = (int)(idx - (long long)b * H);
  const float* w = ws + (long long)b * 4 * H;
  const float dh = dout[idx] + (dhn ? dhn[idx] : 0.f);
  float dai, daf, dag, dao;
  dc_carry[idx] = lstm_gate_grads(dh, dcn ? dcn[idx] : 0.f, w[j], w[H + j], w[2 * H + j], w[3 * H + j], cell[idx], c_prev[idx], dai, daf, dag, dao);
  float* g = dgates + (long long)b * 4 * H;
  g[j] = dai; g[H + j] = daf; g[2 * H + j] = dag; g[3 * H + j] = dao;
}

// ---- backward step, recurrent part + the PREVIOUS step's pointwise part ----------------------------------------------------------
// dh_prev = dgates_t W_hh for a 16-k x 16-row tile, then - same lanes, same (row, unit) elements - the gate gradients of step t - 1 from
// dh' = dout_{t-1} + dh_prev and the dc carry: one launch per backward step.  `dc_carry` is read and rewritten element-wise by its
// owning lane.  grid (H / 16, ceil(B / 16)), block 256 (wave w reduces j in [w * H, (w + 1) * H): gate w).  t == 0 (dout_prev NULL):
// writes dh0 and dc0 instead.
template <int KB>  // as lt_lstm_step_fwd: KB > 0 -> H = 64 KB, the wave's 4 KB j-blocks unrolled in groups of 8 with their loads issued first
__global__ __launch_bounds__(256) void lt_lstm_step_bwd_fused(const float* __restrict__ dg_t, const float* __restrict__ w_hh, float* __restrict__ dc_carry,
                                                              const float* __restrict__ dout_prev, const float* __restrict__ ws_prev,
                                                              const float* __restrict__ cell_prev, const float* __restrict__ cell_prev2,
                                                              float* __restrict__ dg_prev, float* __restrict__ dh0, float* __restrict__ dc0,
                                                              int B, int H_rt) {
  const int H = KB > 0 ? 64 * KB : H_rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int k0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int row = b0 + i;
  const bool row_ok = row < B;
  const float* grow = dg_t + (long long)(row_ok ? row : 0) * 4 * H;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // epilogue operands of wave 0's lanes (row b0 + n, units k0 + 4 g .. + 3), requested before the GEMM (see lt_lstm_step_fwd)
  const int be = b0 + (lane & 15), je = k0 + 4 * (lane >> 4);
  const bool ep = wave == 0 && be < B;
  f32x4 e_dc, e_dout, e_ct, e_cp, e_w[4];
  if (ep) {
    const long long o = (long long)be * H + je;
    e_dc = *(const f32x4*)(dc_carry + o);
    if (dout_prev) {
      e_dout = *(const f32x4*)(dout_prev + o);
      e_ct = *(const f32x4*)(cell_prev + o);
      e_cp = *(const f32x4*)(cell_prev2 + o);
#pragma unroll
      for (int gt = 0; gt < 4; ++gt) e_w[gt] = *(const f32x4*)(ws_prev + (long long)be * 4 * H + gt * H + je);
    }
  }
  const int j_begin = wave * H, j_end = j_begin + H;
  // A operand: A[out = k0 + i][reduction index j + s] = W[j + s][k0 + i]  (16 consecutive k across the lanes of one q: coalesced)
  if (KB > 0) {
    constexpr int G = 8;  // j-blocks per group: 8 x (4 + 4) operand registers in flight
    static_assert(KB == 0 || (4 * KB) % G == 0, "the wave's 4 KB j-blocks come in whole groups");
#pragma unroll
    for (int it0 = 0; it0 < 4 * KB; it0 += G) {
      f32x4 gv[G], wv[G];
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const int j = j_begin + 16 * (it0 + u) + 4 * q;
        gv[u] = *(const f32x4*)(grow + j);
        const float* wp = w_hh + (long long)j * H + k0 + i;
        wv[u] = (f32x4){wp[0], wp[H], wp[2 * (long long)H], wp[3 * (long long)H]};
      }
      __builtin_amdgcn_sched_barrier(0);  // loads of the group first, then its MFMAs
#pragma unroll
      for (int u = 0; u < G; ++u) {
        if (!row_ok) gv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u][s], gv[u][s], acc, 0, 0, 0);
      }
    }
  } else {
    for (int jb = j_begin; jb < j_end; jb += 16) {
      const int j = jb + 4 * q;
      f32x4 gv = *(const f32x4*)(grow + j);
      if (!row_ok) gv = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* wp = w_hh + (long long)j * H + k0 + i;
      const float w0 = wp[0], w1 = wp[H], w2 = wp[2 * (long long)H], w3 = wp[3 * (long long)H];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0, gv[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1, gv[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2, gv[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w3, gv[3], acc, 0, 0, 0);
    }
  }
  __shared__ float red[4][4][64];
#pragma unroll
  for (int v = 0; v < 4; ++v) red[wave][v][lane] = acc[v];
  __syncthreads();
  if (!ep) return;
  f32x4 dhp;
#pragma unroll
  for (int v = 0; v < 4; ++v) dhp[v] = red[0][v][lane] + red[1][v][lane] + red[2][v][lane] + red[3][v][lane];
  const long long o = (long long)be * H + je;
  if (!dout_prev) { *(f32x4*)(dh0 + o) = dhp; *(f32x4*)(dc0 + o) = e_dc; return; }  // t == 0
  f32x4 g_i, g_f, g_g, g_o, d_c;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    float dai, daf, dag, dao;
    d_c[v] = lstm_gate_grads(e_dout[v] + dhp[v], e_dc[v], e_w[0][v], e_w[1][v], e_w[2][v], e_w[3][v], e_ct[v], e_cp[v], dai, daf, dag, dao);
    g_i[v] = dai; g_f[v] = daf; g_g[v] = dag; g_o[v] = dao;
  }
  float* g = dg_prev + (long long)be * 4 * H + je;
  *(f32x4*)g = g_i; *(f32x4*)(g + H) = g_f; *(f32x4*)(g + 2 * H) = g_g; *(f32x4*)(g + 3 * H) = g_o;
  *(f32x4*)(dc_carry + o) = d_c;
}

// ---- host side: validation before anything is launched ----------------------------------------------------------------------------
struct named_ptr { const char* name; const void* p; };

// LT_OK, or LT_EINVAL with "<fn>: <what>".  Pointers first (a float4 moves 16 bytes: alignment is part of the contract), then the sizes.
int check_args(const char* fn, const named_ptr* ptrs, int n, int L, int B, int H) {
  char msg[256];
  const char* what = nullptr;
  for (int k = 0; k < n && !what; ++k) {
    if (!ptrs[k].p || (uintptr_t)ptrs[k].p % 16 != 0) {
      snprintf(msg, sizeof msg, "%s: invalid argument: %s must be non-null and 16-byte aligned", fn, ptrs[k].name);
      lt_set_error(msg);
      return LT_EINVAL;
    }
  }
  if (L < 1) what = "L must be at least 1";
  else if (B < 1 || B > 16 * 65535) what = "B must be in [1, 16 * 65535]";
  else if (H < 64 || (H % 64) != 0) what = "H must be a multiple of 64";
  if (!what) return LT_OK;
  snprintf(msg, sizeof msg, "%s: invalid argument: %s", fn, what);
  lt_set_error(msg);
  return LT_EINVAL;
}

}  // namespace

extern "C" {

int lt_lstm_forward(const float* ig, const float* h0, const float* c0, const float* w_hh, const float* b_ih, const float* b_hh, int L, int B,
                    int H, float* out, float* cell, float* ws, void* stream) {
  const named_ptr ptrs[] = {{"ig", ig}, {"h0", h0}, {"c0", c0}, {"w_hh", w_hh}, {"b_ih", b_ih}, {"b_hh", b_hh}, {"out", out}, {"cell", cell}, {"ws", ws}};
  if (const int rc = check_args("lt_lstm_forward", ptrs, 9, L, B, H)) return rc;
  const dim3 grid((unsigned)(H / 16), (unsigned)((B + 15) / 16));
  const float* h = h0;
  const float* c = c0;
  for (int t = 0; t < L; ++t) {
    float* ht = out + (long long)t * B * H;
    float* ct = cell + (long long)t * B * H;
    const float* igt = ig + (long long)t * B * 4 * H;
    float* wst = ws + (long long)t * B * 4 * H;
    switch (H) {  // the student's encoder is H = 512; the other compile-time sizes cover the usual powers of two
      case 512: hipLaunchKernelGGL(lt_lstm_step_fwd<8>, grid, dim3(256), 0, (hipStream_t)stream, igt, h, c, w_hh, b_ih, b_hh, ht, ct, wst, B, H); break;
      case 256: hipLaunchKernelGGL(lt_lstm_step_fwd<4>, grid, dim3(256), 0, (hipStream_t)stream, igt, h, c, w_hh, b_ih, b_hh, ht, ct, wst, B, H); break;
      case 128: hipLaunchKernelGGL(lt_lstm_step_fwd<2>, grid, dim3(256), 0, (hipStream_t)stream, igt, h, c, w_hh, b_ih, b_hh, ht, ct, wst, B, H); break;
      default: hipLaunchKernelGGL(lt_lstm_step_fwd<0>, grid, dim3(256), 0, (hipStream_t)stream, igt, h, c, w_hh, b_ih, b_hh, ht, ct, wst, B, H); break;
    }
    h = ht;
    c = ct;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  return LT_OK;
}

int lt_lstm_backward(const float* dout, const float* dhn, const float* dcn, const float* out, const float* cell, const float* ws,
                     const float* h0, const float* c0, const float* w_hh, int L, int B, int H, float* dgates, float* scratch, float* dh0,
                     float* dc0, void* stream) {
  // dhn and dcn may each be NULL (= 0); a non-null one is held to the same alignment as the rest
  const named_ptr ptrs[] = {{"dout", dout}, {"dhn", dhn ? dhn : dout}, {"dcn", dcn ? dcn : dout}, {"out", out}, {"cell", cell}, {"ws", ws}, {"h0", h0},
                            {"c0", c0}, {"w_hh", w_hh}, {"dgates", dgates}, {"scratch", scratch}, {"dh0", dh0}, {"dc0", dc0}};
  if (const int rc = check_args("lt_lstm_backward", ptrs, 13, L, B, H)) return rc;
  const dim3 grid((unsigned)(H / 16), (unsigned)((B + 15) / 16));
  const unsigned pw = (unsigned)(((long long)B * H + 255) / 256);
  const long long BH = (long long)B * H;
  // open the recursion: gate gradients of the last step from dh' = dout_{L-1} + dhn, dc' = dcn; then one fused launch per step
  hipLaunchKernelGGL(lt_lstm_step_bwd_gates, dim3(pw), dim3(256), 0, (hipStream_t)stream, dout + (L - 1) * BH, dhn, dcn, ws + (L - 1) * 4 * BH,
                     cell + (L - 1) * BH, L > 1 ? cell + (L - 2) * BH : c0, dgates + (L - 1) * 4 * BH, scratch, B, H);
  for (int t = L - 1; t >= 0; --t) {
    const bool last = t == 0;
    const float* a0 = dgates + t * 4 * BH;
    const float* a3 = last ? (const float*)nullptr : dout + (t - 1) * BH;
    const float* a4 = last ? (const float*)nullptr : ws + (t - 1) * 4 * BH;
    const float* a5 = last ? (const float*)nullptr : cell + (t - 1) * BH;                  // c_{t-1}: the state AFTER step t - 1
    const float* a6 = last ? (const float*)nullptr : (t > 1 ? cell + (t - 2) * BH : c0);  // c_{t-2}: the state BEFORE step t - 1
    float* a7 = last ? (float*)nullptr : dgates + (t - 1) * 4 * BH;
    switch (H) {
      case 512: hipLaunchKernelGGL(lt_lstm_step_bwd_fused<8>, grid, dim3(256), 0, (hipStream_t)stream, a0, w_hh, scratch, a3, a4, a5, a6, a7, dh0, dc0, B, H); break;
      case 256: hipLaunchKernelGGL(lt_lstm_step_bwd_fused<4>, grid, dim3(256), 0, (hipStream_t)stream, a0, w_hh, scratch, a3, a4, a5, a6, a7, dh0, dc0, B, H); break;
      case 128: hipLaunchKernelGGL(lt_lstm_step_bwd_fused<2>, grid, dim3(256), 0, (hipStream_t)stream, a0, w_hh, scratch, a3, a4, a5, a6, a7, dh0, dc0, B, H); break;
      default: hipLaunchKernelGGL(lt_lstm_step_bwd_fused<0>, grid, dim3(256), 0, (hipStream_t)stream, a0, w_hh, scratch, a3, a4, a5, a6, a7, dh0, dc0, B, H); break;
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  return LT_OK;
}

}  // extern "C"
