// Single-layer GRU over a padded batch of whole trajectories: the recurrence of the student's tactile encoder
// (reference loco_rl/loco_rl/models/memory_module.py:10-14 -> nn.GRU; shapes of BASELINE.json configs[3]: input 64, hidden 512,
// L ~ 500 steps, B ~ 50-100 trajectories).
//
// Issued as library calls a step costs ~36 us of GPU time forward and as much backward on this stack (hipBLASLt puts a 101-row GEMM on
// ~24 workgroups); here a step is ONE launch whose grid covers the chip.  The kernels, the two time loops and the argument check are
// lt_seq_tile.h's skeleton (its head comment has the plan and the operand trick), shared with lt_lstm.hip; this file holds the cell -
// three gates r, z, n (PyTorch's order), the state h, the carry of the backward pass is the direct part dh' * z of dh - and the entry
// points.  (The sum order differs from a library GEMM's.)
#include "lt_seq_tile.h"

namespace {

struct GruSeqCell {
  static constexpr int NG = 3, NS = 1;
  // next = (h'), act = (r, z, n, q = W_hn h + b_hn)
  static __device__ __forceinline__ void gates(const float* ig, const float* bi, const float* bh, const float* s, float hp, float* next, float* act) {
    const float r = sigmoidf_(ig[0] + bi[0] + s[0] + bh[0]);
    const float z = sigmoidf_(ig[1] + bi[1] + s[1] + bh[1]);
    const float qn = s[2] + bh[2];
    const float nn = tanhf_(ig[2] + bi[2] + r * qn);
    next[0] = nn + z * (hp - nn);
    act[0] = r; act[1] = z; act[2] = nn; act[3] = qn;
  }
  // The gate gradients of one (row, unit) element of one step from dh' = dout_t + dh_next: d = (dar, daz, dan, dan * r); returns the
  // direct part of the previous step's dh.  (The carry is already inside dh.)
  static __device__ __forceinline__ float gate_grads(float dh, float, const float* w, float, float hp, float* d) {
    const float r = w[0], z = w[1], nn = w[2], qn = w[3];
    const float dn = dh * (1.f - z), dz = dh * (hp - nn);
    const float dan = dn * (1.f - nn * nn), daz = dz * z * (1.f - z);
    const float dar = dan * qn * r * (1.f - r);
    d[0] = dar; d[1] = daz; d[2] = dan; d[3] = dan * r;
    return dh * z;
  }
  template <class T> static __device__ __forceinline__ void store_grads(float* dhg, float* dig, long long row, int unit, int H, const T* d) {
    float* gi = dig + row * 3 * H + unit;
    float* gh = dhg + row * 3 * H + unit;
    *(T*)gi = d[0]; *(T*)(gi + H) = d[1]; *(T*)(gi + 2 * H) = d[2];
    *(T*)gh = d[0]; *(T*)(gh + H) = d[1]; *(T*)(gh + 2 * H) = d[3];
  }
};

}  // namespace

extern "C" {

// ig: [L][B][3H] input-gate pre-activations WITHOUT bias (X W_ih^T); h0 [B][H]; out [L][B][H]; ws [L][B][4H].
int lt_gru_forward(const float* ig, const float* h0, const float* w_hh, const float* b_ih, const float* b_hh, int L, int B, int H,
                   float* out, float* ws, void* stream) {
  if (const int rc = check_seq_args("lt_gru_forward", {{"ig", ig, 16}, {"h0", h0, 16}, {"w_hh", w_hh, 16}, {"b_ih", b_ih, 16}, {"b_hh", b_hh, 16},
                                                       {"out", out, 16}, {"ws", ws, 16}}, L, B, H))
    return rc;
  return seq_forward<GruSeqCell>(ig, h0, nullptr, w_hh, b_ih, b_hh, L, B, H, out, nullptr, ws, stream);
}

// dout [L][B][H]; dhn [B][H] or NULL (= 0); out / ws / h0 as left by lt_gru_forward; dig, dhg [L][B][3H] (outputs: gate gradients, input
// side and hidden side); scratch [B][H]; dh0 [B][H] (output).
int lt_gru_backward(const float* dout, const float* dhn, const float* out, const float* ws, const float* h0, const float* w_hh, int L, int B,
                    int H, float* dig, float* dhg, float* scratch, float* dh0, void* stream) {
  if (const int rc = check_seq_args("lt_gru_backward", {{"dout", dout, 16}, {"dhn", dhn ? dhn : dout, 16}, {"out", out, 16}, {"ws", ws, 16}, {"h0", h0, 16},
                                                        {"w_hh", w_hh, 16}, {"dig", dig, 16}, {"dhg", dhg, 16}, {"scratch", scratch, 16}, {"dh0", dh0, 16}},
                                     L, B, H))
    return rc;
  return seq_backward<GruSeqCell>(dout, dhn, nullptr, h0, out, ws, w_hh, L, B, H, dhg, dig, scratch, dh0, nullptr, stream);
}

}  // extern "C"
