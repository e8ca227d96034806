// The two LSTM memories of a recurrent policy: one rollout step of both in one launch (include/lt_memory.h), and both over a whole
// rollout of an env block, forward and backward (include/lt_memory_seq.h).  The kernels are lt_memory_tile.h's row-block skeleton with
// the LSTM cell below: this file holds the cell, the checks of its argument structs and the entry points.
//
// Step kernel: a unit's four panel rows are its gates i, f, g, o (PyTorch's order), each [W_ih row | W_hh row]; the state is (h, c) and
// the epilogue's operand is c.  TRAIN stores the activated gates.  Backward: K = 4H, the carry is dc_t * f_t.
#include "lt_memory.h"
#include "lt_memory_seq.h"
#include "lt_memory_tile.h"

namespace {

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

int check_net(const char* fn, const char* who, const lt_memory_net* n, int H) {
  if (const int rc = check_net_head(fn, who, n, H)) return rc;
  if (const int rc = check_ptrs(fn, who, {{".x", n->x, 4}, {".w_ih", n->w_ih, 4}, {".w_hh", n->w_hh, 16}, {".b_ih", n->b_ih, 16}, {".b_hh", n->b_hh, 16},
                                          {".h_in", n->h_in, 16}, {".c_in", n->c_in, 16}, {".h_out", n->h_out, 16}, {".c_out", n->c_out, 16},
                                          {".saved_h", n->saved_h, 16}, {".saved_c", n->saved_c, 16}}))
    return rc;
  if (n->h_out == n->h_in || n->c_out == n->c_in) return refuse(fn, who, ".h_out / .c_out", "another buffer than .h_in / .c_in (ping-pong)");
  return LT_OK;
}

int check_seq_net(const char* fn, const char* who, const lt_memory_seq_net* n, const lt_memory_seq_net* other, int T, int E, int H) {
  if (const int rc = check_net_head(fn, who, n, H)) return rc;
  if (n->x_stride < (int64_t)E * n->I) return refuse(fn, who, ".x_stride", "at least E * I");
  if (const int rc = check_ptrs(fn, who, {{".x", n->x, 4}, {".w_ih", n->w_ih, 4}, {".w_hh", n->w_hh, 16}, {".b_ih", n->b_ih, 16}, {".b_hh", n->b_hh, 16},
                                          {".h0", n->h0, 16}, {".c0", n->c0, 16}, {".out", n->out, 16}, {".cell", n->cell, 16}, {".gates", n->gates, 16},
                                          {".h_prev", n->h_prev, 16}, {".c_prev", n->c_prev, 16}}))
    return rc;
  const long long EH = (long long)E * H, TEH = (long long)T * EH;
  const struct { const char* name; const void* p; long long floats; } outs[] = {
      {".out", n->out, TEH}, {".cell", n->cell, TEH}, {".gates", n->gates, 4 * TEH}, {".h_prev", n->h_prev, TEH}, {".c_prev", n->c_prev, TEH}};
  for (const auto& e : outs)
    for (const lt_memory_seq_net* m : {n, other})
      if (m && ((m->h0 && overlaps(e.p, e.floats, m->h0, EH)) || (m->c0 && overlaps(e.p, e.floats, m->c0, EH))))
        return refuse(fn, who, e.name, "a buffer that does not overlap h0 / c0 of either network");
  return LT_OK;
}

int check_seq_grad(const char* fn, const char* who, const lt_memory_seq_grad* n) {
  if (!n) return refuse(fn, who, "", "non-null");
  return check_ptrs(fn, who, {{".dout", n->dout, 16}, {".w_hh", n->w_hh, 16}, {".cell", n->cell, 16}, {".gates", n->gates, 16}, {".c_prev", n->c_prev, 16},
                              {".dgates", n->dgates, 16}, {".dc_carry", n->dc_carry, 16}});
}

}  // namespace

extern "C" {

int lt_memory_step(const lt_memory_net* actor, const lt_memory_net* critic, const uint8_t* dones, int N, int H, void* stream) {
  const char* fn = "lt_memory_step";
  if (const int rc = check_sizes(fn, "N", N, H)) return rc;
  if (const int rc = check_net(fn, "actor", actor, H)) return rc;
  if (const int rc = check_net(fn, "critic", critic, H)) return rc;
  const lt_memory_net* nets[2] = {actor, critic};
  StepArgs<2> a;
  for (int k = 0; k < 2; ++k) {
    NetArgs<2>& r = a.net[k];
    const lt_memory_net* n = nets[k];
    set_weights(r, n, H);
    r.x = n->x; r.s_in[0] = n->h_in; r.s_in[1] = n->c_in; r.s_out[0] = n->h_out; r.s_out[1] = n->c_out;
    r.saved[0] = n->saved_h; r.saved[1] = n->saved_c;
  }
  a.dones = dones; a.N = N; a.H = H;
  return launch_steps<LstmCell, false>(a, 1, stream, [](int) {});
}

int lt_memory_finish(const float* h_a, const float* c_a, const float* h_c, const float* c_c, const uint8_t* dones, int N, int H,
                     float* out_h_a, float* out_c_a, float* out_h_c, float* out_c_c, void* stream) {
  return launch_finish<4>("lt_memory_finish", {"h_a", "c_a", "h_c", "c_c", "out_h_a", "out_c_a", "out_h_c", "out_c_c"}, {h_a, c_a, h_c, c_c},
                          {out_h_a, out_c_a, out_h_c, out_c_c}, dones, N, H, stream);
}

int lt_memory_seq_forward(const lt_memory_seq_net* actor, const lt_memory_seq_net* critic, const uint8_t* dones, int64_t dones_stride,
                          int T, int E, int H, void* stream) {
  const char* fn = "lt_memory_seq_forward";
  if (const int rc = check_seq_sizes(fn, T, E, H, dones, dones_stride)) return rc;
  if (const int rc = check_seq_net(fn, "actor", actor, critic, T, E, H)) return rc;
  if (const int rc = check_seq_net(fn, "critic", critic, actor, T, E, H)) return rc;
  const lt_memory_seq_net* nets[2] = {actor, critic};
  SeqStepArgs<2> a;
  for (int k = 0; k < 2; ++k) set_weights(a.net[k], nets[k], H);
  a.N = E; a.H = H;
  const long long EH = (long long)E * H;
  return launch_steps<LstmCell, true>(a, T, stream, [&](int t) {
    for (int k = 0; k < 2; ++k) {
      NetArgs<2>& r = a.net[k];
      const lt_memory_seq_net* n = nets[k];
      r.x = n->x + t * n->x_stride;
      r.s_in[0] = t == 0 ? n->h0 : n->out + (t - 1) * EH;
      r.s_in[1] = t == 0 ? n->c0 : n->cell + (t - 1) * EH;
      r.s_out[0] = n->out + t * EH; r.s_out[1] = n->cell + t * EH;
      r.saved[0] = n->h_prev + t * EH; r.saved[1] = n->c_prev + t * EH;
      a.gates[k] = n->gates + 4 * t * EH;
    }
    a.dones = dones && t > 0 ? dones + (t - 1) * dones_stride : nullptr;
  });
}

int lt_memory_seq_backward_units(int E, int H) { return bwd_units_or_zero(E, H, LstmCell::KG); }

int lt_memory_seq_backward(const lt_memory_seq_grad* actor, const lt_memory_seq_grad* critic, const uint8_t* dones, int64_t dones_stride,
                           int T, int E, int H, void* stream) {
  const char* fn = "lt_memory_seq_backward";
  if (const int rc = check_seq_sizes(fn, T, E, H, dones, dones_stride)) return rc;
  if (const int rc = check_seq_grad(fn, "actor", actor)) return rc;
  if (const int rc = check_seq_grad(fn, "critic", critic)) return rc;
  const lt_memory_seq_grad* nets[2] = {actor, critic};
  const long long EH = (long long)E * H;
  return launch_backward<LstmCell>(dones, dones_stride, T, E, H, stream, [&](int k, int t) {
    const lt_memory_seq_grad* n = nets[k];
    LstmCell::BwdNet r;
    r.w_hh = n->w_hh; r.dg_next = t + 1 < T ? n->dgates + 4 * (t + 1) * EH : nullptr;
    r.dout = n->dout + t * EH; r.cell = n->cell + t * EH; r.gates = n->gates + 4 * t * EH; r.c_prev = n->c_prev + t * EH;
    r.dg = n->dgates + 4 * t * EH; r.carry = n->dc_carry;
    return r;
  });
}

}  // extern "C"
