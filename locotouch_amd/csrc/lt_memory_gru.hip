// The two GRU memories of a recurrent policy: one rollout step of both in one launch, and both over a whole rollout of an env block,
// forward and backward (include/lt_memory_gru.h).  The GRU counterpart of lt_memory.hip: the kernels are lt_memory_tile.h's row-block
// skeleton with the GRU cell of lt_memory_cells.h; this file holds the checks of its argument structs and the entry points.
//
// Step kernel.  The n gate needs its x part and its h part as SEPARATE sums (b_hn sits inside r * (...)), so a unit again has four
// panel rows:
//     v = 0: [W_ir | W_hr]      v = 1: [W_iz | W_hz]      v = 2: [W_in | 0]      v = 3: [0 | W_hn]
// and lane (n, g) of the D layout still holds everything of one unit of row n: (a_r, a_z, the x part of a_n, h W_hn^T).  A quarter of
// the MFMAs multiply zeros; a three-row layout would put the gates of one unit into different lanes (the M index of a 16-row tile is
// 4 g + v: three rows per unit do not divide it) and the epilogue through LDS.  The state is h alone; TRAIN stores r, z, n and hn.
//
// Backward: K = 3H, dh = dhg[t+1] W_hh (3H / 16 k blocks are whole groups of four); the carry is dh * z.
#include "lt_memory_cells.h"
#include "lt_memory_gru.h"
#include "lt_memory_tile.h"
#include "lt_rnn_encoder.h"

namespace {

int check_net(const char* fn, const char* who, const lt_memory_gru_net* n, int H) {
  if (const int rc = check_net_head(fn, who, n, H)) return rc;
  if (const int rc = check_ptrs(fn, who, {{".x", n->x, 4}, {".w_ih", n->w_ih, 4}, {".w_hh", n->w_hh, 16}, {".b_ih", n->b_ih, 16}, {".b_hh", n->b_hh, 16},
                                          {".h_in", n->h_in, 16}, {".h_out", n->h_out, 16}, {".saved_h", n->saved_h, 16}}))
    return rc;
  if (n->h_out == n->h_in) return refuse(fn, who, ".h_out", "another buffer than .h_in (ping-pong)");
  return LT_OK;
}

int check_seq_net(const char* fn, const char* who, const lt_memory_gru_seq_net* n, const lt_memory_gru_seq_net* other, int T, int E, int H) {
  if (const int rc = check_net_head(fn, who, n, H)) return rc;
  if (n->x_stride < (int64_t)E * n->I) return refuse(fn, who, ".x_stride", "at least E * I");
  if (const int rc = check_ptrs(fn, who, {{".x", n->x, 4}, {".w_ih", n->w_ih, 4}, {".w_hh", n->w_hh, 16}, {".b_ih", n->b_ih, 16}, {".b_hh", n->b_hh, 16},
                                          {".h0", n->h0, 16}, {".out", n->out, 16}, {".gates", n->gates, 16}, {".h_prev", n->h_prev, 16}}))
    return rc;
  const long long EH = (long long)E * H, TEH = (long long)T * EH;
  const struct { const char* name; const void* p; long long floats; } outs[] = {{".out", n->out, TEH}, {".gates", n->gates, 4 * TEH}, {".h_prev", n->h_prev, TEH}};
  for (const auto& e : outs)
    for (const lt_memory_gru_seq_net* m : {n, other})
      if (m && m->h0 && overlaps(e.p, e.floats, m->h0, EH)) return refuse(fn, who, e.name, "a buffer that does not overlap h0 of either network");
  return LT_OK;
}

int check_seq_grad(const char* fn, const char* who, const lt_memory_gru_seq_grad* n) {
  if (!n) return refuse(fn, who, "", "non-null");
  return check_ptrs(fn, who, {{".dout", n->dout, 16}, {".w_hh", n->w_hh, 16}, {".gates", n->gates, 16}, {".h_prev", n->h_prev, 16},
                              {".dig", n->dig, 16}, {".dhg", n->dhg, 16}, {".dh_carry", n->dh_carry, 16}});
}

// one step of both memories, the x rows of network k xs_k floats apart (validated operands)
int launch_step(const lt_memory_gru_net* actor, const lt_memory_gru_net* critic, long long xs_a, long long xs_c, const uint8_t* dones, int N,
                int H, void* stream) {
  const lt_memory_gru_net* nets[2] = {actor, critic};
  const long long xs[2] = {xs_a, xs_c};
  StepArgs<1> a;
  for (int k = 0; k < 2; ++k) {
    NetArgs<1>& r = a.net[k];
    const lt_memory_gru_net* n = nets[k];
    set_weights(r, n, H);
    r.x = n->x; r.XS = xs[k]; r.s_in[0] = n->h_in; r.s_out[0] = n->h_out; r.saved[0] = n->saved_h;
  }
  a.dones = dones; a.N = N; a.H = H;
  return launch_steps<GruCell, false>(a, 1, stream, [](int) {});
}

}  // namespace

extern "C" {

int lt_memory_gru_step(const lt_memory_gru_net* actor, const lt_memory_gru_net* critic, const uint8_t* dones, int N, int H, void* stream) {
  const char* fn = "lt_memory_gru_step";
  if (const int rc = check_sizes(fn, "N", N, H)) return rc;
  if (const int rc = check_net(fn, "actor", actor, H)) return rc;
  if (const int rc = check_net(fn, "critic", critic, H)) return rc;
  return launch_step(actor, critic, actor->I, critic->I, dones, N, H, stream);
}

// include/lt_rnn_encoder.h: the same step with each network's x rows x_stride floats apart
int lt_memory_gru_step_strided(const lt_rnn_encoder_memory* actor, const lt_rnn_encoder_memory* critic, const uint8_t* dones, int N, int H,
                               void* stream) {
  const char* fn = "lt_memory_gru_step_strided";
  if (const int rc = check_sizes(fn, "N", N, H)) return rc;
  const lt_rnn_encoder_memory* src[2] = {actor, critic};
  const char* who[2] = {"actor", "critic"};
  lt_memory_gru_net nets[2];
  for (int k = 0; k < 2; ++k) {
    const lt_rnn_encoder_memory* m = src[k];
    if (!m) return refuse(fn, who[k], "", "non-null");
    nets[k] = {m->x, m->I, m->w_ih, m->w_hh, m->b_ih, m->b_hh, m->h_in, m->h_out, m->saved_h};
    if (const int rc = check_net(fn, who[k], &nets[k], H)) return rc;
    if (m->c_in || m->c_out || m->saved_c) return refuse(fn, who[k], ".c_in / .c_out / .saved_c", "NULL (a GRU's state is h alone)");
    if (m->x_stride < m->I) return refuse(fn, who[k], ".x_stride", "at least I");
  }
  return launch_step(&nets[0], &nets[1], actor->x_stride, critic->x_stride, dones, N, H, stream);
}

int lt_memory_gru_finish(const float* h_a, const float* h_c, const uint8_t* dones, int N, int H, float* out_h_a, float* out_h_c, void* stream) {
  return launch_finish<2>("lt_memory_gru_finish", {"h_a", "h_c", "out_h_a", "out_h_c"}, {h_a, h_c}, {out_h_a, out_h_c}, dones, N, H, stream);
}

int lt_memory_gru_seq_forward(const lt_memory_gru_seq_net* actor, const lt_memory_gru_seq_net* critic, const uint8_t* dones,
                              int64_t dones_stride, int T, int E, int H, void* stream) {
  const char* fn = "lt_memory_gru_seq_forward";
  if (const int rc = check_seq_sizes(fn, T, E, H, dones, dones_stride)) return rc;
  if (const int rc = check_seq_net(fn, "actor", actor, critic, T, E, H)) return rc;
  if (const int rc = check_seq_net(fn, "critic", critic, actor, T, E, H)) return rc;
  const lt_memory_gru_seq_net* nets[2] = {actor, critic};
  SeqStepArgs<1> a;
  for (int k = 0; k < 2; ++k) set_weights(a.net[k], nets[k], H);
  a.N = E; a.H = H;
  const long long EH = (long long)E * H;
  return launch_steps<GruCell, true>(a, T, stream, [&](int t) {
    for (int k = 0; k < 2; ++k) {
      NetArgs<1>& r = a.net[k];
      const lt_memory_gru_seq_net* n = nets[k];
      r.x = n->x + t * n->x_stride;
      r.s_in[0] = t == 0 ? n->h0 : n->out + (t - 1) * EH;
      r.s_out[0] = n->out + t * EH;
      r.saved[0] = n->h_prev + t * EH;
      a.gates[k] = n->gates + 4 * t * EH;
    }
    a.dones = dones && t > 0 ? dones + (t - 1) * dones_stride : nullptr;
  });
}

int lt_memory_gru_seq_backward_units(int E, int H) { return bwd_units_or_zero(E, H, GruCell::KG); }

int lt_memory_gru_seq_backward(const lt_memory_gru_seq_grad* actor, const lt_memory_gru_seq_grad* critic, const uint8_t* dones,
                               int64_t dones_stride, int T, int E, int H, void* stream) {
  const char* fn = "lt_memory_gru_seq_backward";
  if (const int rc = check_seq_sizes(fn, T, E, H, dones, dones_stride)) return rc;
  if (const int rc = check_seq_grad(fn, "actor", actor)) return rc;
  if (const int rc = check_seq_grad(fn, "critic", critic)) return rc;
  const lt_memory_gru_seq_grad* nets[2] = {actor, critic};
  const long long EH = (long long)E * H;
  return launch_backward<GruCell>(dones, dones_stride, T, E, H, stream, [&](int k, int t) {
    const lt_memory_gru_seq_grad* n = nets[k];
    GruCell::BwdNet r;
    r.w_hh = n->w_hh; r.dg_next = t + 1 < T ? n->dhg + 3 * (t + 1) * EH : nullptr;
    r.dout = n->dout + t * EH; r.gates = n->gates + 4 * t * EH; r.h_prev = n->h_prev + t * EH;
    r.dig = n->dig + 3 * t * EH; r.dhg = n->dhg + 3 * t * EH; r.carry = n->dh_carry;
    return r;
  });
}

}  // extern "C"
