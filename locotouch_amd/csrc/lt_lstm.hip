// Single-layer LSTM over a padded batch of whole trajectories (include/lt_lstm.h): the recurrence of `Memory` / `PolicyMemory` with
// rnn_type "lstm" (reference loco_rl/loco_rl/models/memory_module.py:6 -> nn.LSTM; the default of ActorCriticRecurrent).
//
//
// The kernels, the two time loops and the argument check are lt_seq_tile.h's skeleton (its head comment has the plan and the operand
// trick), shared with lt_gru.hip; this file holds the cell - four gates i, f, g, o (PyTorch's order), the state (h, c), the carry of the
// backward pass is dc - and the entry points.
#include "lt_lstm.h"
#include "lt_seq_tile.h"

namespace {

struct LstmSeqCell {
  static constexpr int NG = 4, NS = 2;
  // next = (h', c'), act = the activated gates i, f, g, o
  static __device__ __forceinline__ void gates(const float* ig, const float* bi, const float* bh, const float* s, float cp, float* next, float* act) {
    const float gi = sigmoidf_(ig[0] + bi[0] + s[0] + bh[0]);
    const float gf = sigmoidf_(ig[1] + bi[1] + s[1] + bh[1]);
    const float gg = tanhf_(ig[2] + bi[2] + s[2] + bh[2]);
    const float go = sigmoidf_(ig[3] + bi[3] + s[3] + bh[3]);
    const float cn = gf * cp + gi * gg;
    next[1] = cn; next[0] = go * tanhf_(cn);
    act[0] = gi; act[1] = gf; act[2] = gg; act[3] = go;
  }
  // The gate gradients of one (row, unit) element of one step from dh' = dout_t + dh_next and the dc carry; returns the new dc carry.
  // tanh(c_t) is recomputed (one exp) instead of stored and read back.
  static __device__ __forceinline__ float gate_grads(float dh, float dc_in, const float* w, float ct, float cp, float* d) {
    const float gi = w[0], gf = w[1], gg = w[2], go = w[3];
    const float tc = tanhf_(ct);
    const float dc = dc_in + dh * go * (1.f - tc * tc);
    d[0] = dc * gg * gi * (1.f - gi);
    d[1] = dc * cp * gf * (1.f - gf);
    d[2] = dc * gi * (1.f - gg * gg);
    d[3] = dh * tc * go * (1.f - go);
    return dc * gf;
  }
  template <class T> static __device__ __forceinline__ void store_grads(float* dgates, float*, long long row, int unit, int H, const T* d) {
    float* g = dgates + row * 4 * H + unit;
    *(T*)g = d[0]; *(T*)(g + H) = d[1]; *(T*)(g + 2 * H) = d[2]; *(T*)(g + 3 * H) = d[3];
  }
};

}  // namespace

extern "C" {

int lt_lstm_forward(const float* ig, const float* h0, const float* c0, const float* w_hh, const float* b_ih, const float* b_hh, int L, int B,
                    int H, float* out, float* cell, float* ws, void* stream) {
  if (const int rc = check_seq_args("lt_lstm_forward", {{"ig", ig, 16}, {"h0", h0, 16}, {"c0", c0, 16}, {"w_hh", w_hh, 16}, {"b_ih", b_ih, 16}, {"b_hh", b_hh, 16},
                                                        {"out", out, 16}, {"cell", cell, 16}, {"ws", ws, 16}}, L, B, H))
    return rc;
  return seq_forward<LstmSeqCell>(ig, h0, c0, w_hh, b_ih, b_hh, L, B, H, out, cell, ws, stream);
}

int lt_lstm_backward(const float* dout, const float* dhn, const float* dcn, const float* out, const float* cell, const float* ws,
                     const float* h0, const float* c0, const float* w_hh, int L, int B, int H, float* dgates, float* scratch, float* dh0,
                     float* dc0, void* stream) {
  // dhn and dcn may each be NULL (= 0); a non-null one is held to the same alignment as the rest
  if (const int rc = check_seq_args("lt_lstm_backward", {{"dout", dout, 16}, {"dhn", dhn ? dhn : dout, 16}, {"dcn", dcn ? dcn : dout, 16}, {"out", out, 16},
                                                         {"cell", cell, 16}, {"ws", ws, 16}, {"h0", h0, 16}, {"c0", c0, 16}, {"w_hh", w_hh, 16},
                                                         {"dgates", dgates, 16}, {"scratch", scratch, 16}, {"dh0", dh0, 16}, {"dc0", dc0, 16}}, L, B, H))
    return rc;
  return seq_backward<LstmSeqCell>(dout, dhn, dcn, c0, cell, ws, w_hh, L, B, H, dgates, nullptr, scratch, dh0, dc0, stream);
}

}  // extern "C"
