// lt_policy_encoder.hip - one inference step of an encoder policy (include/lt_policy_encoder.h): for an ActorCriticRNNEncoder the memory
// step of lt_policy.hip on the tail columns of the rows, then - and for an ActorCriticEncoder alone - ONE launch of the kernel below for
// everything that stands between the memory and the action: the normalised head columns, the encoder stack, the concatenation and the
// actor stack.
//
// Plan: lt_encoder_kernel's (csrc/lt_encoder.hip, header comment; the device helpers are lt_encoder_tile.h's).  A four-wave workgroup owns
// a row block of RB rows (16 at play's 1 - 50 envs) and walks ALL layers, encoder then actor, as one list: layer g reads LDS activation
// buffer g & 1 and writes the other one, its weights pass through LDS a panel at a time (at most 64 output features, fewer where a wide
// layer's panel would not fit beside the activations: the height moves work between waves, never a sum's order), a wave takes 16 x 16
// tiles of panel x block.  What differs from the encoder kernel:
//   * the encoder's last layer writes the embedding at column flat_dim of the actor's input rows.  flat_dim is any number (270 in the
//     teacher's rows, 6 in a test), so these are 4-byte LDS stores, not the engine's 16-byte one;
//   * the actor's input rows stand in buffer EL & 1 (EL encoder layers).  That buffer held the input of encoder layer EL - 2, so the head
//     columns are staged - and normalised - only in front of the encoder's last layer, behind a barrier of their own, together with zeros
//     in the columns behind flat_dim + E up to the end of the last 16-wide k block (the buffer held wider activations earlier);
//   * the actor's last layer has any width from 1 (12 actions): its panel is zero-filled behind the last feature and the epilogue
//     guards every feature; it writes `actions_out`;
//   * the encoder's input rows are h_out of the memory launch (already normalised there) or, in the plain form, the tail columns of the
//     row, normalised as they are staged.
// Arithmetic: the engine's - v_mfma_f32_16x16x4_f32, k blocks of 16 in index order dealt to four partial sums added pairwise
// (`tile_sum`), then the bias, then `activate`.  The encoder layers are lt_encoder_kernel's statement by statement, so the embedding has
// its bits; the actor's first layer sums over [head | embedding] in torch's column order by the same rule.
#include "lt_policy_encoder.h"

#include "lt_encoder.h"
#include "lt_encoder_tile.h"
#include "lt_memory_tile.h"  // round_up, overlaps, cu_count, kLdsBytes, allow_lds and the host checks

static_assert(LT_POLICY_ENCODER_MAX_LAYERS == LT_ENCODER_MAX_LAYERS, "lt_policy_encoder.h states its layer limit as lt_encoder.h's");
static_assert(LT_POLICY_ENCODER_MAX_LAYERS == LT_MLP_MAX_LAYERS, "lt_policy_encoder.h states its layer limit as lt_mlp's");

namespace {

constexpr int kMaxL = LT_POLICY_ENCODER_MAX_LAYERS;
constexpr int kMaxWidth = LT_ENCODER_MAX_WIDTH;  // of every layer but the actor's first input
// 16 rows of the two activation buffers and a 16-row panel of the widest input fill the LDS at this width of the actor's input
static_assert(4 * (16 * (LT_POLICY_ENCODER_MAX_ACTOR_IN + 8 + kMaxWidth + 8) + 16 * (LT_POLICY_ENCODER_MAX_ACTOR_IN + 8)) <= kLdsBytes &&
                  4 * (16 * (LT_POLICY_ENCODER_MAX_ACTOR_IN + 16 + 8 + kMaxWidth + 8) + 16 * (LT_POLICY_ENCODER_MAX_ACTOR_IN + 16 + 8)) > kLdsBytes,
              "LT_POLICY_ENCODER_MAX_ACTOR_IN is the widest actor input the LDS holds at a 16-row block and a 16-row panel");

struct PeLayer { const float* w; const float* b; int K, O, act; };  // w [O][K], torch's layout; act: behind this layer
struct PeArgs {
  const float* obs; long long obs_stride;        // rows in place
  const float* enc_x; long long enc_x_stride;    // the encoder's input rows: h_out of the memory launch, or the tail columns of obs
  const float* mean; const float* std; float eps;  // [obs_dim] or both null
  int enc_x_col;                                 // the obs column enc_x starts at (its statistics' place), -1: rows of the memory, taken as they are
  PeLayer layer[2 * kMaxL];                      // EL encoder layers, then the actor's
  float* actions; float* emb;                    // [n][A]; null or [n][E]
  int n, flat, EL, NL, E, A;
  int stride[2];                                 // LDS row strides of the activation buffers (buffer g & 1 holds layer g's input)
  int RB, off_b, off_panel, panel_floats;        // float offsets in LDS; the panel's room
};

// Stages `cols_ok` columns of the block's rows from src (row r at src + r * src_stride; normalised with mean / std [cols_ok] when given)
// into dst rows of dst_stride floats: a [rows][cols] tile, zeros where r >= rows_ok or c >= cols_ok.  Rows are only 4-byte aligned:
// scalar loads, U of them in flight (as `stage`).
template <int U>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, long long src_stride, const float* __restrict__ mean,
                                           const float* __restrict__ std, float eps, int rows_ok, int cols_ok, float* __restrict__ dst,
                                           int dst_stride, int rows, int cols, int tid) {
  if (cols == 0) return;
  const int total = rows * cols;
  const unsigned magic = div_magic(cols);
  for (int base = 0; base < total; base += 256 * U) {
    float v[U], m[U], s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + 256 * u + tid;
      const int r = (int)__umulhi((unsigned)idx, magic), c = idx - r * cols;
      v[u] = 0.f; m[u] = 0.f; s[u] = 1.f;
      if (idx < total && r < rows_ok && c < cols_ok) {
        v[u] = src[(long long)r * src_stride + c];
        if (mean) { m[u] = mean[c]; s[u] = std[c]; }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + 256 * u + tid;
      const int r = (int)__umulhi((unsigned)idx, magic), c = idx - r * cols;
      // (the torch normaliser's statement, bit for bit: two rounded f32 operations and a correctly rounded quotient)
      if (idx < total) dst[r * dst_stride + c] = mean && r < rows_ok && c < cols_ok ? ieee_div(v[u] - m[u], s[u] + eps) : v[u];
    }
  }
}

__global__ __launch_bounds__(256) void lt_policy_encoder_kernel(const PeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int RB = a.RB;
  const int r0 = blockIdx.x * RB;
  const int rows = min(RB, a.n - r0);
  const int nsub = (rows + 15) / 16;
  const int flat = a.flat, E = a.E, A = a.A;
  float* buf[2] = {lds, lds + a.off_b};
  float* panel = lds + a.off_panel;

  // ---- 1. the encoder's input rows -> buffer 0 (whole 16-row sub-tiles and 16-wide k blocks; zeros where there is no row or no column)
  {
    const int K = a.layer[0].K;
    const bool norm = a.mean && a.enc_x_col >= 0;
    stage_rows<16>(a.enc_x + (long long)r0 * a.enc_x_stride, a.enc_x_stride, norm ? a.mean + a.enc_x_col : nullptr,
                   norm ? a.std + a.enc_x_col : nullptr, a.eps, rows, K, buf[0], a.stride[0], 16 * nsub, round_up(K, 16), tid);
  }

  // ---- 2. the layers: encoder 0 .. EL - 1, actor EL .. NL - 1
  for (int g = 0; g < a.NL; ++g) {
    const PeLayer& ly = a.layer[g];
    const int K = ly.K, K16 = round_up(K, 16), O = ly.O, kp = K16 + 8, nblk = K16 / 16;
    const bool to_actor = g == a.EL - 1, last = g == a.NL - 1;
    const float* in = buf[g & 1];
    float* dst = buf[(g + 1) & 1];
    const int sin = a.stride[g & 1], sd = a.stride[(g + 1) & 1];
    const float* __restrict__ w = ly.w;
    const float* __restrict__ bias = ly.b;
    const int kind = ly.act;
    if (to_actor) {
      // dst becomes the actor's input rows [ head | embedding | zeros up to the k blocks' end ].  It was the input of encoder layer
      // EL - 2: every wave has to be through with that layer before the head columns land
      __syncthreads();
      stage_rows<8>(a.obs + (long long)r0 * a.obs_stride, a.obs_stride, a.mean, a.std, a.eps, rows, flat, dst, sd, 16 * nsub, flat, tid);
      const int c0 = flat + E, pad = round_up(c0, 16) - c0;
      for (int idx = tid; idx < 16 * nsub * pad; idx += 256) dst[(idx / pad) * sd + c0 + idx % pad] = 0.f;
    }
    const int PM = min(64, a.panel_floats / kp / 16 * 16);  // (at least 16: the host's plan)
    for (int p0 = 0; p0 < O; p0 += PM) {
      // the panel: rows p0 .. p0 + pm16 - 1 of W_g (zeros behind O and behind K).  The barrier in front keeps it until every wave has
      // left the previous panel - and, for a layer's first panel, until the previous layer's activations are all written
      const int pm16 = min(PM, round_up(O - p0, 16)), mtiles = pm16 / 16;
      __syncthreads();
      // (a workgroup walks the panels alone at play's sizes: twice the encoder kernels' loads in flight, and 8-byte loads for a layer
      // whose width is even but no multiple of 4)
      stage_panel<16, 16, true>(w, K, O, p0, pm16, panel, tid);
      __syncthreads();
      for (int tile = wave; tile < mtiles * nsub; tile += 4) {
        const int mt = tile % mtiles, s = tile / mtiles;
        const float* ap = panel + (16 * mt + i) * kp + 4 * q;
        const float* bp = in + (16 * s + i) * sin + 4 * q;
        // epilogue: sum[v] of lane (i, q) is D[4 q + v][i] = feature f0 + v of row 16 s + i
        const f32x4 sum = tile_sum(ap, bp, nblk);
        const int f0 = p0 + 16 * mt + 4 * q, row = 16 * s + i;
        const bool row_ok = row < rows;
        const long long gr = r0 + row;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (f0 + e < O) v[e] = activate(kind, sum[e] + bias[f0 + e]);
        if (last) {  // the actions: any width, feature by feature
          if (row_ok) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (f0 + e < O) a.actions[gr * A + f0 + e] = v[e];
          }
        } else if (to_actor) {  // the embedding, at column flat_dim of the actor's input rows (only 4-byte aligned there)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (f0 + e < O) {
              dst[row * sd + flat + f0 + e] = v[e];
              if (a.emb && row_ok) a.emb[gr * E + f0 + e] = v[e];
            }
          }
        } else {  // the next layer's input (zeros in the columns behind O up to its k blocks' end)
          *(f32x4*)(dst + row * sd + f0) = v;
        }
      }
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
bool has_memory(const lt_policy_encoder_desc* d) { return d->rnn_type != LT_POLICY_ENCODER_NO_MEMORY; }

bool hidden_act(int a) { return a == LT_ACT_ELU || a == LT_ACT_RELU || a == LT_ACT_TANH; }

int check_desc(const char* fn, const lt_policy_encoder_desc* d) {
  if (!d) return refuse(fn, "", "desc", "non-null");
  if (d->rnn_type != LT_POLICY_RNN_LSTM && d->rnn_type != LT_POLICY_RNN_GRU && d->rnn_type != LT_POLICY_ENCODER_NO_MEMORY)
    return refuse(fn, "", "rnn_type", "LT_POLICY_RNN_LSTM, LT_POLICY_RNN_GRU or LT_POLICY_ENCODER_NO_MEMORY");
  const bool mem = has_memory(d);
  const int H = d->rnn_hidden;
  if (mem) {
    if (d->rnn_layers != 1) return refuse(fn, "", "rnn_layers", "1 (a multi-layer memory is not served)");
    if (H < 64 || H > 512 || (H % 64) != 0) return refuse(fn, "", "rnn_hidden", "a multiple of 64 in [64, 512]");
  } else {
    if (d->rnn_layers != 0) return refuse(fn, "", "rnn_layers", "0 without a memory");
    if (H != 0) return refuse(fn, "", "rnn_hidden", "0 without a memory");
  }
  if (d->obs_dim < 1) return refuse(fn, "", "obs_dim", "at least 1");
  if (d->flat_dim < 0 || d->flat_dim > d->obs_dim) return refuse(fn, "", "flat_dim", "in [0, obs_dim]");
  if (mem && (d->tail_dim < 1 || d->tail_dim > d->obs_dim || d->tail_dim + H > 1248))
    return refuse(fn, "", "tail_dim", "in [1, obs_dim] with tail_dim + rnn_hidden <= 1248");
  if (!mem && (d->tail_dim < 1 || d->tail_dim > d->obs_dim || d->tail_dim > kMaxWidth))
    return refuse(fn, "", "tail_dim", "in [1, obs_dim] and at most LT_ENCODER_MAX_WIDTH (the encoder reads it)");
  if (d->enc_layers < 1 || d->enc_layers > kMaxL) return refuse(fn, "", "enc_layers", "in [1, LT_POLICY_ENCODER_MAX_LAYERS]");
  char field[48];
  for (int l = 0; l < d->enc_layers; ++l)
    if (d->enc_dims[l] < 8 || d->enc_dims[l] > kMaxWidth || d->enc_dims[l] % 8 != 0) {
      snprintf(field, sizeof field, "enc_dims[%d]", l);
      return refuse(fn, "", field, "a multiple of 8 in [8, LT_ENCODER_MAX_WIDTH]");
    }
  if (!hidden_act(d->enc_activation)) return refuse(fn, "", "enc_activation", "LT_ACT_ELU, LT_ACT_RELU or LT_ACT_TANH");
  if (d->enc_final_activation != LT_ACT_NONE && !hidden_act(d->enc_final_activation))
    return refuse(fn, "", "enc_final_activation", "LT_ACT_NONE, LT_ACT_ELU, LT_ACT_RELU or LT_ACT_TANH");
  if (d->actor_layers < 1 || d->actor_layers > kMaxL) return refuse(fn, "", "actor_layers", "in [1, LT_POLICY_ENCODER_MAX_LAYERS]");
  for (int l = 0; l < d->actor_layers; ++l) {
    snprintf(field, sizeof field, "actor_dims[%d]", l);
    const int w = d->actor_dims[l];
    if (l < d->actor_layers - 1 && (w < 8 || w > kMaxWidth || w % 8 != 0)) return refuse(fn, "", field, "a multiple of 8 in [8, 512] (a hidden width)");
    if (l == d->actor_layers - 1 && (w < 1 || w > kMaxWidth)) return refuse(fn, "", field, "in [1, 512] (the action count)");
  }
  if (!hidden_act(d->actor_activation)) return refuse(fn, "", "actor_activation", "LT_ACT_ELU, LT_ACT_RELU or LT_ACT_TANH");
  if (d->flat_dim + d->enc_dims[d->enc_layers - 1] > LT_POLICY_ENCODER_MAX_ACTOR_IN)
    return refuse(fn, "", "flat_dim + enc_dims[enc_layers - 1]", "at most LT_POLICY_ENCODER_MAX_ACTOR_IN (the actor's input rows stay in LDS)");
  return LT_OK;
}

int check_rows(const char* fn, int64_t n) {
  if (n < 1 || n > 16 * 65535) return refuse(fn, "", "n", "in [1, 16 * 65535]");
  return LT_OK;
}

// the layer list and the LDS strides of `d` with the parameters `p`
void set_layers(PeArgs& a, const lt_policy_encoder_desc* d, const lt_policy_encoder_params* p) {
  const int EL = d->enc_layers, AL = d->actor_layers;
  a.EL = EL; a.NL = EL + AL; a.flat = d->flat_dim; a.E = d->enc_dims[EL - 1]; a.A = d->actor_dims[AL - 1];
  a.stride[0] = a.stride[1] = 0;
  for (int g = 0; g < 2 * kMaxL; ++g) {
    PeLayer& ly = a.layer[g];
    ly = PeLayer{nullptr, nullptr, 0, 0, LT_ACT_NONE};
    if (g >= a.NL) continue;
    if (g < EL) {
      ly.w = p->enc_weight[g]; ly.b = p->enc_bias[g];
      ly.K = g ? d->enc_dims[g - 1] : has_memory(d) ? d->rnn_hidden : d->tail_dim;
      ly.O = d->enc_dims[g];
      ly.act = g < EL - 1 ? d->enc_activation : d->enc_final_activation;
    } else {
      const int l = g - EL;
      ly.w = p->actor_weight[l]; ly.b = p->actor_bias[l];
      ly.K = l ? d->actor_dims[l - 1] : a.flat + a.E;
      ly.O = d->actor_dims[l];
      ly.act = l < AL - 1 ? d->actor_activation : LT_ACT_NONE;
    }
    if (lds_stride(ly.K) > a.stride[g & 1]) a.stride[g & 1] = lds_stride(ly.K);  // layer g reads buffer g & 1
  }
}

// Row block and the LDS carve of one launch: the largest row block (64, 32, 16) that still gives every CU a workgroup and leaves a
// 16-row panel of the widest input beside its activations; the panel gets what is left, up to 64 rows of that input.  16 always fits
// (the static_assert above).  Returns the dynamic LDS in bytes.
int plan(PeArgs& a) {
  int kp = 0;
  for (int g = 0; g < a.NL; ++g) kp = lds_stride(a.layer[g].K) > kp ? lds_stride(a.layer[g].K) : kp;
  const int budget = kLdsBytes / (int)sizeof(float), per_row = a.stride[0] + a.stride[1];
  const int cus = cu_count();
  for (const int rb : {64, 32, 16}) {
    if (rb > 16 && (a.n + rb - 1) / rb < cus) continue;
    const int left = budget - rb * per_row;
    if (left < 16 * kp) continue;
    a.RB = rb; a.off_b = rb * a.stride[0]; a.off_panel = rb * per_row;
    a.panel_floats = left < 64 * kp ? left : 64 * kp;
    return (a.off_panel + a.panel_floats) * (int)sizeof(float);
  }
  return 0;  // (unreachable for a validated descriptor)
}

}  // namespace

extern "C" {

int lt_policy_encoder_validate(const lt_policy_encoder_desc* desc) { return check_desc("lt_policy_encoder_validate", desc); }

int lt_policy_encoder_step_launches(const lt_policy_encoder_desc* desc, int64_t n) {
  const char* fn = "lt_policy_encoder_step_launches";
  if (const int rc = check_desc(fn, desc)) return rc;
  if (const int rc = check_rows(fn, n)) return rc;
  return has_memory(desc) ? 2 : 1;
}

int lt_policy_encoder_step(const lt_policy_encoder_desc* desc, const lt_policy_encoder_params* params, const float* obs,
                           int64_t obs_row_stride, const uint8_t* done_mask, const float* h_in, const float* c_in, float* h_out,
                           float* c_out, int64_t n, float* actions_out, float* embedding_out, void* stream) {
  const char* fn = "lt_policy_encoder_step";
  if (const int rc = check_desc(fn, desc)) return rc;
  if (const int rc = check_rows(fn, n)) return rc;
  const bool mem = has_memory(desc), lstm = desc->rnn_type == LT_POLICY_RNN_LSTM;
  const int H = desc->rnn_hidden, D = desc->obs_dim, T = desc->tail_dim;
  if (obs_row_stride < D) return refuse(fn, "", "obs_row_stride", "at least obs_dim");
  if (!params) return refuse(fn, "", "params", "non-null");
  if (mem)
    if (const int rc = check_ptrs(fn, "", {{"params.w_ih", params->w_ih, 4}, {"params.w_hh", params->w_hh, 16}, {"params.b_ih", params->b_ih, 16},
                                           {"params.b_hh", params->b_hh, 16}}))
      return rc;
  char wn[40], bn[40];
  for (int l = 0; l < desc->enc_layers; ++l) {
    snprintf(wn, sizeof wn, "params.enc_weight[%d]", l);
    snprintf(bn, sizeof bn, "params.enc_bias[%d]", l);
    if (const int rc = check_ptrs(fn, "", {{wn, params->enc_weight[l], 4}, {bn, params->enc_bias[l], 4}})) return rc;
  }
  for (int l = 0; l < desc->actor_layers; ++l) {
    snprintf(wn, sizeof wn, "params.actor_weight[%d]", l);
    snprintf(bn, sizeof bn, "params.actor_bias[%d]", l);
    if (const int rc = check_ptrs(fn, "", {{wn, params->actor_weight[l], 4}, {bn, params->actor_bias[l], 4}})) return rc;
  }
  if (!params->norm_mean != !params->norm_std) return refuse(fn, "", "params.norm_mean / params.norm_std", "both NULL or both set");
  if (params->norm_mean)
    if (const int rc = check_ptrs(fn, "", {{"params.norm_mean", params->norm_mean, 4}, {"params.norm_std", params->norm_std, 4}})) return rc;
  if (const int rc = check_ptrs(fn, "", {{"obs", obs, 4}, {"actions_out", actions_out, 4}})) return rc;
  if (embedding_out && (uintptr_t)embedding_out % 4 != 0) return refuse(fn, "", "embedding_out", "NULL or 4-byte aligned");
  if (mem) {
    if (const int rc = check_ptrs(fn, "", {{"h_in", h_in, 16}, {"h_out", h_out, 16}})) return rc;
    if (lstm) {
      if (const int rc = check_ptrs(fn, "", {{"c_in", c_in, 16}, {"c_out", c_out, 16}})) return rc;
    } else {
      if (c_in) return refuse(fn, "", "c_in", "NULL for a GRU");
      if (c_out) return refuse(fn, "", "c_out", "NULL for a GRU");
    }
  } else {
    const struct { const char* name; const void* p; } none[] = {{"done_mask", done_mask}, {"h_in", h_in}, {"c_in", c_in}, {"h_out", h_out}, {"c_out", c_out}};
    for (const auto& e : none)
      if (e.p) return refuse(fn, "", e.name, "NULL without a memory");
  }
  const long long nH = (long long)n * H, nobs = (long long)(n - 1) * obs_row_stride + D;
  const int E = desc->enc_dims[desc->enc_layers - 1], A = desc->actor_dims[desc->actor_layers - 1];
  const struct { const char* name; const float* p; long long floats; } outs[] = {{"h_out", h_out, nH}, {"c_out", c_out, nH},
                                                                                 {"actions_out", actions_out, (long long)n * A},
                                                                                 {"embedding_out", embedding_out, (long long)n * E}};
  for (int k = 0; k < 4; ++k) {
    const auto& e = outs[k];
    if (!e.p) continue;
    if (k < 2)
      for (const float* in : {h_in, c_in})
        if (in && overlaps(e.p, nH, in, nH)) return refuse(fn, "", e.name, "a buffer that does not overlap h_in / c_in (ping-pong)");
    if (overlaps(e.p, e.floats, obs, nobs)) return refuse(fn, "", e.name, "a buffer that does not overlap obs");
    for (int j = 0; j < k; ++j)
      if (outs[j].p && overlaps(e.p, e.floats, outs[j].p, outs[j].floats)) return refuse(fn, "", e.name, "a buffer that does not overlap another output");
  }

  PeArgs a;
  set_layers(a, desc, params);
  a.obs = obs; a.obs_stride = obs_row_stride; a.n = (int)n;
  a.mean = params->norm_mean; a.std = params->norm_std; a.eps = params->norm_eps;
  a.actions = actions_out; a.emb = embedding_out;
  if (mem) {
    lt_policy_memory m;
    m.w_ih = params->w_ih; m.w_hh = params->w_hh; m.b_ih = params->b_ih; m.b_hh = params->b_hh;
    m.norm_mean = params->norm_mean ? params->norm_mean + (D - T) : nullptr;
    m.norm_std = params->norm_std ? params->norm_std + (D - T) : nullptr;
    m.norm_eps = params->norm_eps;
    if (const int rc = lt_policy_memory_launch(desc->rnn_type, &m, T, H, obs + (D - T), obs_row_stride, done_mask, h_in, c_in, h_out, c_out, (int)n, stream))
      return rc;
    a.enc_x = h_out; a.enc_x_stride = H; a.enc_x_col = -1;
  } else {
    a.enc_x = obs + (D - T); a.enc_x_stride = obs_row_stride; a.enc_x_col = D - T;
  }
  const int lds = plan(a);
  if (lds <= 0) return refuse(fn, "the layers do not fit the LDS");
  const kernel_fn<PeArgs> kernel = lt_policy_encoder_kernel;
  if (lds > 64 * 1024)
    if (const int rc = allow_lds(kernel)) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + a.RB - 1) / a.RB)), dim3(256), lds, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // extern "C"
