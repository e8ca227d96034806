// The two cells of the memory kernels, once: stateless structs of constants and `static __device__ __forceinline__` functions that hold
// everything cell-specific of a kernel that is instantiated with them (the members are listed in lt_memory_tile.h).  Three translation
// units take them: lt_memory.hip (LstmCell) and lt_memory_gru.hip (GruCell) through lt_memory_tile.h's row-block skeleton - the rollout
// step and the update's sequence kernels - and lt_policy.hip (both) through its inference-step kernel.  One definition of the gate
// arithmetic is what makes the inference step reproduce the rollout's state bit for bit.
//
// LstmCell: a unit's four panel rows are its gates i, f, g, o (PyTorch's order), each [W_ih row | W_hh row]; the state is (h, c) and the
// epilogue's operand is c.  Backward: K = 4H, the carry is dc_t * f_t.
// GruCell: the n gate needs its x part and its h part as SEPARATE sums (b_hn sits inside r * (...)), so a unit again has four rows:
//     v = 0: [W_ir | W_hr]      v = 1: [W_iz | W_hz]      v = 2: [W_in | 0]      v = 3: [0 | W_hn]
// The state is h alone.  Backward: K = 3H, the carry is dh * z.
#pragma once

#include <hip/hip_runtime.h>

#include "lt_device_prims.h"

namespace {

using lt::f32x4;
using lt::sigmoidf_;
using lt::tanhf_;

struct LstmCell {
  static constexpr int NS = 2;  // h, c
  static constexpr int KG = 4;
  static __device__ __forceinline__ int ih_gate(int v) { return v; }
  static __device__ __forceinline__ int hh_gate(int v) { return v; }
  static __device__ __forceinline__ bool ih_used(int) { return true; }
  static __device__ __forceinline__ bool hh_used(int) { return true; }
  static __device__ __forceinline__ void load_bias(const float* b_ih, const float* b_hh, int H, int j0, int qm, int mt, float* bias) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int wrow = v * H + j0 + qm + mt;
      bias[v] = b_ih[wrow] + b_hh[wrow];
    }
  }
  // next = (h', c'), act = the activated gates i, f, g, o
  static __device__ __forceinline__ void gates(const f32x4& sum, const float* bias, float cp, float* next, float* act) {
    const float gi = sigmoidf_(sum[0] + bias[0]);
    const float gf = sigmoidf_(sum[1] + bias[1]);
    const float gg = tanhf_(sum[2] + bias[2]);
    const float go = sigmoidf_(sum[3] + bias[3]);
    next[1] = gf * cp + gi * gg;
    next[0] = go * tanhf_(next[1]);
    act[0] = gi; act[1] = gf; act[2] = gg; act[3] = go;
  }

  struct BwdNet {
    const float* w_hh; const float* dg_next; const float* dout; const float* cell; const float* gates; const float* c_prev;
    float* dg; float* carry;
  };
  // The gate gradients of four consecutive units of one row (lt_lstm.hip's formula; tanh(c_t) recomputed): reads gates / cell / c_prev /
  // dout at element offset o of [E][H] (gates: row * 4H + unit), writes dgates and the new carry dc_t * f_t.
  struct GradOps { f32x4 dout, ct, cp, g[4]; };

  static __device__ __forceinline__ GradOps load_grad_ops(const BwdNet& p, long long row, int unit, int H) {
    GradOps e;
    const long long o = row * H + unit;
    e.dout = *(const f32x4*)(p.dout + o);
    e.ct = *(const f32x4*)(p.cell + o);
    e.cp = *(const f32x4*)(p.c_prev + o);
#pragma unroll
    for (int v = 0; v < 4; ++v) e.g[v] = *(const f32x4*)(p.gates + row * 4 * H + v * H + unit);
    return e;
  }

  // the GEMM's sum and the dc carry are masked separately and enter at different places
  static __device__ __forceinline__ void store_gate_grads(const BwdNet& p, long long row, int unit, int H, const GradOps& e, f32x4 dh_next, f32x4 dc_in,
                                                          bool done) {
    if (done) dh_next = (f32x4){0.f, 0.f, 0.f, 0.f};
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
    *(f32x4*)(p.carry + row * H + unit) = dc;
  }
};

struct GruCell {
  static constexpr int NS = 1;  // h
  static constexpr int KG = 3;
  static __device__ __forceinline__ int ih_gate(int v) { return v; }
  static __device__ __forceinline__ int hh_gate(int v) { return v == 3 ? 2 : v; }
  static __device__ __forceinline__ bool ih_used(int v) { return v < 3; }
  static __device__ __forceinline__ bool hh_used(int v) { return v != 2; }
  // b_ir + b_hr, b_iz + b_hz, b_in, b_hn
  static __device__ __forceinline__ void load_bias(const float* b_ih, const float* b_hh, int H, int j0, int qm, int mt, float* bias) {
    const int unit = j0 + qm + mt;
    bias[0] = b_ih[unit] + b_hh[unit];
    bias[1] = b_ih[H + unit] + b_hh[H + unit];
    bias[2] = b_ih[2 * H + unit];
    bias[3] = b_hh[2 * H + unit];
  }
  // next = (h'), act = r, z, n, hn
  static __device__ __forceinline__ void gates(const f32x4& sum, const float* bias, float hp, float* next, float* act) {
    const float gr = sigmoidf_(sum[0] + bias[0]);
    const float gz = sigmoidf_(sum[1] + bias[1]);
    const float hn = sum[3] + bias[3];
    const float gn = tanhf_(sum[2] + bias[2] + gr * hn);
    next[0] = (1.f - gz) * gn + gz * hp;
    act[0] = gr; act[1] = gz; act[2] = gn; act[3] = hn;
  }

  struct BwdNet {
    const float* w_hh; const float* dg_next; const float* dout; const float* gates; const float* h_prev;
    float* dig; float* dhg; float* carry;  // dg_next: dhg of step t + 1
  };
  struct GradOps { f32x4 dout, hp, g[4]; };  // g: r, z, n, hn

  static __device__ __forceinline__ GradOps load_grad_ops(const BwdNet& p, long long row, int unit, int H) {
    GradOps e;
    const long long o = row * H + unit;
    e.dout = *(const f32x4*)(p.dout + o);
    e.hp = *(const f32x4*)(p.h_prev + o);
#pragma unroll
    for (int v = 0; v < 4; ++v) e.g[v] = *(const f32x4*)(p.gates + row * 4 * H + v * H + unit);
    return e;
  }

  // the gate gradients of four consecutive units of one row; what comes back is where(done, 0, dhg[t+1] W_hh + carry): the carry joins
  // the GEMM's sum first, then the mask
  static __device__ __forceinline__ void store_gate_grads(const BwdNet& p, long long row, int unit, int H, const GradOps& e, f32x4 sum, f32x4 carry_in,
                                                          bool done) {
    f32x4 back = sum + carry_in;
    if (done) back = (f32x4){0.f, 0.f, 0.f, 0.f};
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
};

}  // namespace
