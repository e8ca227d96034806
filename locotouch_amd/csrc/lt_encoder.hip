// The encoder in front of an ActorCriticEncoder's stacks (include/lt_encoder.h): out[r] = [ obs[r, :flat_dim] | enc(obs[r, -enc_in:]) ]
// for one or two networks in ONE launch - and the same with the encoder's input rows read from a second array, the output of a memory
// (include/lt_rnn_encoder.h: out[r] = [ obs[r, :flat_dim] | enc(h[r, :enc_in]) ]; only where the tail columns are staged from differs).
//
// Shape: n = num_envs rows in the rollout (4096), a minibatch's rows in the update (some 24 k); the reference encoder is
// 78 -> 256 -> 128 -> 64 -> 64, 65 k MACs per row, 260 KB of weights - more than a CU's LDS.  A workgroup of four waves owns a ROW BLOCK
// of RB rows (64, 32 or 16) and walks the layers:
//   1. the head columns of its rows go to `out`, the tail columns into activation buffer A in LDS (zeros behind enc_in up to the next
//      multiple of 16; rows are only 4-byte aligned, so scalar accesses);
//   2. per layer, the weights pass through LDS a PANEL at a time: PM (64, 32 or 16) output features x the layer's input width.  A wave
//      takes 16 x 16 tiles (16 features x 16 rows) of the panel's PM / 16 x RB / 16: the A operand (weights) and the B operand (the
//      block's activations) are one ds_read_b128 each per 16-wide k block;
//   3. the epilogue adds the bias, applies the activation and writes the tile into the OTHER activation buffer (and, in the training
//      form, into acts[l]); the last layer writes the embedding behind the head columns of `out` instead.
// The activations of the row block never leave LDS between layers.  grid (ceil(n / RB), networks), block 256.
//
// Arithmetic: v_mfma_f32_16x16x4_f32, exact f32 products, f32 accumulation, k blocks in index order dealt to four partial sums (block b
// to chain b % 4) that are added pairwise, then the bias.  RB and PM move work between workgroups and waves, never a sum's order: a
// row's bits depend on the row and the parameters alone.  Operand trick as lt_memory_tile.h: MFMA step s of a 16-wide k block consumes
// the k-set {16 b + 4 q + s}, so lane (i, q) supplies component s of ONE 16-byte LDS read for either operand.
//
// LDS strides (rows of both activation buffers and of the panel) are round_up(width, 16) + 8 floats, an odd multiple of 8: the 16 lanes
// of a ds_read_b128 lane group start at 16 distinct multiples of 4 banks.
//
// The backward pass of the second form (include/lt_rnn_encoder_train.h, lt_rnn_encoder_backward_kernel) is the same plan run from the
// embedding's gradient to the memory's: the row block's gradient dz_l lives in the two LDS buffers, layer l's product da_{l-1} = dz_l W_l
// sums over the layer's OUTPUTS, so a panel is PM INPUT features of W_l read TRANSPOSED from torch's [O][K] layout (panel row k holds
// W_l[:, k]), and the epilogue multiplies by the activation's derivative taken from the stored activation, writes dz_{l-1} to global
// memory (for the weight gradients) and into the other buffer; the last product is dh.  Same tiles, same operand reads, same order of
// every sum: 16-wide blocks of the summed index in order, dealt to four partial sums, added pairwise.
#include "lt_encoder.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lt_device_prims.h"
#include "lt_encoder_tile.h"
#include "lt_env.h"
#include "lt_host_check.h"
#include "lt_internal.h"
#include "lt_rnn_encoder.h"
#include "lt_rnn_encoder_train.h"

static_assert(LT_RNN_ENCODER_MAX_LAYERS == LT_ENCODER_MAX_LAYERS, "lt_rnn_encoder.h states its layer limit as lt_encoder.h's");
static_assert(LT_RNN_ENCODER_TRAIN_MAX_LAYERS == LT_RNN_ENCODER_MAX_LAYERS, "lt_rnn_encoder_train.h states its layer limit as lt_rnn_encoder.h's");
static_assert(LT_ENCODER_MAX_LAYERS == LT_MLP_MAX_LAYERS, "lt_encoder.h states its layer limit as lt_mlp's");

namespace {

constexpr int kMaxL = LT_ENCODER_MAX_LAYERS;
constexpr int kLdsBytes = 160 * 1024;

struct EncNet {
  const float* obs; long long obs_stride;
  const float* h; long long h_stride;  // non-null: the encoder reads h[r, :enc_in] instead of the tail columns of obs
  const float* w[kMaxL]; const float* b[kMaxL];
  float* out; float* acts[kMaxL];
  int obs_dim, flat_dim, L;
  int dims[kMaxL + 1];  // dims[0] = enc_in, dims[l + 1] = outputs of layer l
  int act, final_act;
  int stride[2];        // LDS row strides of activation buffers A (inputs of even layers) and B (of odd layers)
};
struct EncArgs { EncNet net[2]; int n, RB, PM, off_b, off_panel; };  // off_*: float offsets of buffer B and the panel in LDS

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// (lds_stride, activate, stage, stage_panel and tile_sum: lt_encoder_tile.h)

__global__ __launch_bounds__(256) void lt_encoder_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const EncNet& p = a.net[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int RB = a.RB, PM = a.PM;
  const int r0 = blockIdx.x * RB;
  const int rows = min(RB, a.n - r0);
  const int nsub = (rows + 15) / 16;
  const int E = p.dims[p.L], ow = p.flat_dim + E;
  float* buf[2] = {lds, lds + a.off_b};
  float* panel = lds + a.off_panel;

  // ---- 1. head columns -> out (copies), tail columns -> buffer A (whole 16-row sub-tiles and 16-wide k blocks; zeros where there is no
  // row or no column)
  for (int base = 0; base < rows * p.flat_dim; base += 256 * 8) {  // (eight independent loads in flight, as in `stage`)
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + 256 * u + tid, r = idx / p.flat_dim, c = idx - r * p.flat_dim;
      v[u] = idx < rows * p.flat_dim ? p.obs[(long long)(r0 + r) * p.obs_stride + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + 256 * u + tid, r = idx / p.flat_dim, c = idx - r * p.flat_dim;
      if (idx < rows * p.flat_dim) p.out[(long long)(r0 + r) * ow + c] = v[u];
    }
  }
  {
    const int K = p.dims[0];
    const float* src = p.h ? p.h + (long long)r0 * p.h_stride : p.obs + (long long)r0 * p.obs_stride + (p.obs_dim - K);
    stage<16, float>(src, p.h ? p.h_stride : p.obs_stride, rows, K, buf[0], p.stride[0], 16 * nsub, round_up(K, 16), tid);
  }

  // ---- 2. the layers
  for (int l = 0; l < p.L; ++l) {
    const int K = p.dims[l], K16 = round_up(K, 16), O = p.dims[l + 1], kp = K16 + 8, nblk = K16 / 16;
    const bool last = l == p.L - 1;
    const float* in = buf[l & 1];
    float* dst = buf[(l + 1) & 1];
    const int sin = p.stride[l & 1], sd = p.stride[(l + 1) & 1];
    const float* __restrict__ w = p.w[l];
    const float* __restrict__ bias = p.b[l];
    float* actl = p.acts[l];
    const int kind = last ? p.final_act : p.act;
    for (int p0 = 0; p0 < O; p0 += PM) {
      // the panel: rows p0 .. p0 + pm16 - 1 of W_l (zeros behind O and behind K).  The barrier in front keeps it until every wave has
      // left the previous panel - and, for a layer's first panel, until the previous layer's activations are all written
      const int pm16 = min(PM, round_up(O - p0, 16)), mtiles = pm16 / 16;
      __syncthreads();
      stage_panel(w, K, O, p0, pm16, panel, tid);
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
        if (f0 < O) {  // (O is a multiple of 8 and f0 of 4: all four features or none)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = sum[e] + bias[f0 + e];
          if (last && actl && row_ok) {  // the pre-activation embedding
#pragma unroll
            for (int e = 0; e < 4; ++e) actl[gr * O + f0 + e] = v[e];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = activate(kind, v[e]);
          if (row_ok) {
            float* g = last ? p.out + gr * ow + p.flat_dim + f0 : actl ? actl + gr * O + f0 : nullptr;
            if (g) {
#pragma unroll
              for (int e = 0; e < 4; ++e) g[e] = v[e];
            }
          }
        }
        // the next layer's input (zeros in the columns behind O up to its k blocks' end)
        if (!last) *(f32x4*)(dst + row * sd + f0) = v;
      }
    }
  }
}

// ---- the backward pass (include/lt_rnn_encoder_train.h) ----------------------------------------------------------------------------------
struct EncGradNet {
  const float* dx; long long dx_stride;
  const float* out;
  const float* w[kMaxL]; const float* acts[kMaxL];
  float* dz[kMaxL]; float* dh;
  int flat_dim, L;
  int dims[kMaxL + 1];  // as EncNet
  int act, final_act;
  int stride[2];        // LDS row strides of gradient buffers A (dz_{L-1}, dz_{L-3}, ...) and B (dz_{L-2}, ...)
};
struct EncGradArgs { EncGradNet net[2]; int n, RB, PM, off_b, off_panel; };

// the derivative of a hidden activation from its stored OUTPUT a
__device__ __forceinline__ float activation_grad(int kind, float a) {
  if (kind == LT_ACT_ELU) return a > 0.f ? 1.f : a + 1.f;
  if (kind == LT_ACT_RELU) return a > 0.f ? 1.f : 0.f;
  return 1.f - a * a;  // LT_ACT_TANH
}

// Stages panel rows kk < pm16 (input features k0 + kk of a layer) x columns o < O16 (its outputs) TRANSPOSED from w [O][K]:
// panel[kk * op + o] = w[o * K + k0 + kk] where o < O and k0 + kk < K, else zeros.  A wave takes an 8 x 8 patch per trip: lane
// (kk = lane % 8, o = lane / 8) reads eight 32-byte runs of w and writes LDS word kk * op + o.  op is an odd multiple of 8, so the
// 64 words are distinct mod 64; a 4-byte LDS write is banked mod 32 per half wave, where the eight kk of a half land on four multiples
// of 8: a 2-way conflict on the write, once per panel element (a 4 x 16 patch would be conflict-free with 16-byte runs of w; not
// measured).  U loads in flight, as `stage`.
template <int U>
__device__ __forceinline__ void stage_transposed(const float* __restrict__ w, int K, int O, int k0, float* __restrict__ panel, int op, int pm16,
                                                 int O16, int tid) {
  const int total = pm16 * O16, nkb = pm16 / 8;
  const unsigned magic = div_magic(nkb);
  for (int base = 0; base < total; base += 256 * U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + 256 * u + tid, patch = idx >> 6, g = idx & 63;
      const int ob = (int)__umulhi((unsigned)patch, magic), kb = patch - ob * nkb;
      const int kk = 8 * kb + (g & 7), o = 8 * ob + (g >> 3);
      v[u] = 0.f;
      if (idx < total && o < O && k0 + kk < K) v[u] = w[(long long)o * K + k0 + kk];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + 256 * u + tid, patch = idx >> 6, g = idx & 63;
      const int ob = (int)__umulhi((unsigned)patch, magic), kb = patch - ob * nkb;
      const int kk = 8 * kb + (g & 7), o = 8 * ob + (g >> 3);
      if (idx < total) panel[kk * op + o] = v[u];
    }
  }
}

__global__ __launch_bounds__(256) void lt_rnn_encoder_backward_kernel(const EncGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const EncGradNet& p = a.net[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int RB = a.RB, PM = a.PM;
  const int r0 = blockIdx.x * RB;
  const int rows = min(RB, a.n - r0);
  const int nsub = (rows + 15) / 16;
  const int L = p.L, E = p.dims[L], flat = p.flat_dim, ow = flat + E;
  float* buf[2] = {lds, lds + a.off_b};
  float* panel = lds + a.off_panel;

  // ---- 1. dz_{L-1} = dx[:, flat : flat + E] * f' -> global memory and buffer A (whole 16-row sub-tiles and 16-wide blocks; zeros where
  // there is no row or no column).  The rows of dx are only 4-byte aligned: scalar loads, four in flight.
  {
    const int E16 = round_up(E, 16), total = 16 * nsub * E16, s0 = p.stride[0];
    const unsigned magic = div_magic(E16);
    const float* __restrict__ pre = p.acts[L - 1];
    float* __restrict__ dzl = p.dz[L - 1];
    for (int base = 0; base < total; base += 256 * 4) {
      float g[4], d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = base + 256 * u + tid;
        const int r = (int)__umulhi((unsigned)idx, magic), c = idx - r * E16;
        const long long gr = r0 + r;
        g[u] = 0.f;
        d[u] = 1.f;
        if (idx < total && r < rows && c < E) {
          g[u] = p.dx[gr * p.dx_stride + flat + c];
          if (p.final_act == LT_ACT_TANH) {
            const float e = p.out[gr * ow + flat + c];
            d[u] = 1.f - e * e;
          } else if (p.final_act == LT_ACT_ELU) {
            const float z = pre[gr * E + c];
            d[u] = z > 0.f ? 1.f : expf(z);
          } else if (p.final_act == LT_ACT_RELU) {
            d[u] = pre[gr * E + c] > 0.f ? 1.f : 0.f;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = base + 256 * u + tid;
        const int r = (int)__umulhi((unsigned)idx, magic), c = idx - r * E16;
        if (idx < total) {
          const float v = p.final_act == LT_ACT_NONE ? g[u] : g[u] * d[u];
          buf[0][r * s0 + c] = v;
          if (r < rows && c < E) dzl[(long long)(r0 + r) * E + c] = v;
        }
      }
    }
  }

  // ---- 2. the layers, last to first: step t reads dz_l (l = L - 1 - t) from buffer t & 1 and writes dz_{l-1} into the other one
  for (int l = L - 1; l >= 0; --l) {
    const int t = L - 1 - l;
    const int K = p.dims[l], O = p.dims[l + 1], O16 = round_up(O, 16), op = O16 + 8, nblk = O16 / 16;
    const float* in = buf[t & 1];
    float* dst = buf[(t + 1) & 1];
    const int sin = p.stride[t & 1], sd = p.stride[(t + 1) & 1];
    const float* __restrict__ w = p.w[l];
    const float* __restrict__ act_out = l > 0 ? p.acts[l - 1] : nullptr;
    float* __restrict__ dzl = l > 0 ? p.dz[l - 1] : p.dh;
    for (int p0 = 0; p0 < K; p0 += PM) {
      // the panel: input features p0 .. p0 + pm16 - 1 of W_l.  The barrier in front keeps it until every wave has left the previous
      // panel - and, for a layer's first panel, until the gradient this layer reads is all written
      const int pm16 = min(PM, round_up(K - p0, 16)), mtiles = pm16 / 16;
      __syncthreads();
      stage_transposed<8>(w, K, O, p0, panel, op, pm16, O16, tid);
      __syncthreads();
      for (int tile = wave; tile < mtiles * nsub; tile += 4) {
        const int mt = tile % mtiles, s = tile / mtiles;
        const float* ap = panel + (16 * mt + i) * op + 4 * q;
        const float* bp = in + (16 * s + i) * sin + 4 * q;
        // epilogue: sum[v] of lane (i, q) is D[4 q + v][i] = input feature f0 + v of row 16 s + i
        const f32x4 sum = tile_sum(ap, bp, nblk);
        const int f0 = p0 + 16 * mt + 4 * q, row = 16 * s + i;
        const bool row_ok = row < rows;
        const long long gr = r0 + row;
        if (l == 0) {  // dh: enc_in is any width, so column by column
          if (row_ok) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (f0 + e < K) dzl[gr * K + f0 + e] = sum[e];
          }
          continue;
        }
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (f0 < K && row_ok) {  // (K is a multiple of 8 and f0 of 4: all four features or none)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = sum[e] * activation_grad(p.act, act_out[gr * K + f0 + e]);
#pragma unroll
          for (int e = 0; e < 4; ++e) dzl[gr * K + f0 + e] = v[e];
        }
        // the next step's gradient (zeros in the rows behind the block's last and in the columns behind K up to its blocks' end)
        *(f32x4*)(dst + row * sd + f0) = v;
      }
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// `tail`: the encoder reads the tail columns of the row (false: a second array, whose width the row does not bound)
int check_desc(const char* fn, const char* who, const lt_encoder_desc* d, bool tail = true) {
  if (!d) return refuse(fn, who, "", "non-null");
  if (d->num_layers < 1 || d->num_layers > kMaxL) return refuse(fn, who, ".num_layers", "in [1, LT_ENCODER_MAX_LAYERS]");
  if (d->obs_dim < 1) return refuse(fn, who, ".obs_dim", "at least 1");
  if (!tail && (d->enc_in < 1 || d->enc_in > LT_ENCODER_MAX_WIDTH)) return refuse(fn, who, ".enc_in", "in [1, LT_ENCODER_MAX_WIDTH]");
  if (tail && (d->enc_in < 1 || d->enc_in > LT_ENCODER_MAX_WIDTH || d->enc_in > d->obs_dim))
    return refuse(fn, who, ".enc_in", "in [1, LT_ENCODER_MAX_WIDTH] and at most obs_dim");
  if (d->flat_dim < 0 || d->flat_dim > d->obs_dim) return refuse(fn, who, ".flat_dim", "in [0, obs_dim]");
  for (int l = 0; l < d->num_layers; ++l)
    if (d->dims[l] < 8 || d->dims[l] > LT_ENCODER_MAX_WIDTH || d->dims[l] % 8 != 0) {
      char field[32];
      snprintf(field, sizeof field, ".dims[%d]", l);
      return refuse(fn, who, field, "a multiple of 8 in [8, LT_ENCODER_MAX_WIDTH]");
    }
  if (d->activation != LT_ACT_ELU && d->activation != LT_ACT_RELU && d->activation != LT_ACT_TANH)
    return refuse(fn, who, ".activation", "LT_ACT_ELU, LT_ACT_RELU or LT_ACT_TANH");
  if (d->final_activation != LT_ACT_NONE && d->final_activation != LT_ACT_ELU && d->final_activation != LT_ACT_RELU && d->final_activation != LT_ACT_TANH)
    return refuse(fn, who, ".final_activation", "LT_ACT_NONE, LT_ACT_ELU, LT_ACT_RELU or LT_ACT_TANH");
  return LT_OK;
}

bool overlaps(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}

int check_net(const char* fn, const char* who, const lt_encoder_net* net, int n) {
  if (!net) return refuse(fn, who, "", "non-null");
  char sub[32];
  snprintf(sub, sizeof sub, "%s.desc", who);
  if (const int rc = check_desc(fn, sub, &net->desc)) return rc;
  const lt_encoder_desc& d = net->desc;
  if (net->obs_stride < d.obs_dim) return refuse(fn, who, ".obs_stride", "at least obs_dim");
  if (const int rc = check_ptrs(fn, who, {{".obs", net->obs, 4}, {".out", net->out, 4}})) return rc;
  const int L = d.num_layers;
  for (int l = 0; l < L; ++l) {
    char wn[32], bn[32];
    snprintf(wn, sizeof wn, ".weight[%d]", l);
    snprintf(bn, sizeof bn, ".bias[%d]", l);
    if (const int rc = check_ptrs(fn, who, {{wn, net->weight[l], 4}, {bn, net->bias[l], 4}})) return rc;
  }
  // the training form: every hidden layer's buffer (and the pre-activation embedding's, with a final activation), or none at all
  bool any = false;
  for (int l = 0; l < kMaxL; ++l) any = any || net->acts[l] != nullptr;
  if (any) {
    const int need = d.final_activation != LT_ACT_NONE ? L : L - 1;
    for (int l = 0; l < kMaxL; ++l) {
      char an[32];
      snprintf(an, sizeof an, ".acts[%d]", l);
      if (l < need) {
        if (const int rc = check_ptr(fn, who, {an, net->acts[l], 4})) return rc;
      } else if (net->acts[l]) {
        return refuse(fn, who, an, "NULL (only hidden layers, and the embedding with a final activation, have a buffer)");
      }
    }
  }
  const long long ow = d.flat_dim + d.dims[L - 1];
  if (overlaps(net->out, (long long)n * ow, net->obs, (long long)(n - 1) * net->obs_stride + d.obs_dim))
    return refuse(fn, who, ".out", "a buffer that does not overlap obs");
  return LT_OK;
}

void set_net(EncNet& r, const lt_encoder_net* net) {
  const lt_encoder_desc& d = net->desc;
  r.obs = net->obs; r.obs_stride = net->obs_stride; r.out = net->out;
  r.h = nullptr; r.h_stride = 0;
  r.obs_dim = d.obs_dim; r.flat_dim = d.flat_dim; r.L = d.num_layers;
  r.act = d.activation; r.final_act = d.final_activation;
  r.dims[0] = d.enc_in;
  r.stride[0] = r.stride[1] = 0;
  for (int l = 0; l < kMaxL; ++l) {
    const bool used = l < d.num_layers;
    r.w[l] = used ? net->weight[l] : nullptr; r.b[l] = used ? net->bias[l] : nullptr; r.acts[l] = used ? net->acts[l] : nullptr;
    r.dims[l + 1] = used ? d.dims[l] : 0;
    if (used && lds_stride(r.dims[l]) > r.stride[l & 1]) r.stride[l & 1] = lds_stride(r.dims[l]);  // layer l reads buffer l & 1
  }
}

// the widths of an lt_rnn_encoder_net as the descriptor the kernel's checks and plan read
lt_encoder_desc desc_of(const lt_rnn_encoder_net* net) {
  lt_encoder_desc d;
  d.obs_dim = net->obs_dim; d.flat_dim = net->flat_dim; d.enc_in = net->enc_in; d.num_layers = net->num_layers;
  for (int l = 0; l < kMaxL; ++l) d.dims[l] = net->dims[l];
  d.activation = net->activation; d.final_activation = net->final_activation;
  return d;
}

// checks an lt_rnn_encoder_net and hands it back as the lt_encoder_net of the same widths and operands (its obs tail is never read).
// `train`: the training form - the buffers of every hidden layer (and the pre-activation embedding's, with a final activation) are
// asked for; without it any buffer is refused
int check_rnn_net(const char* fn, const char* who, const lt_rnn_encoder_net* net, int n, lt_encoder_net& e, bool train = false) {
  if (!net) return refuse(fn, who, "", "non-null");
  e.desc = desc_of(net);
  if (const int rc = check_desc(fn, who, &e.desc, false)) return rc;
  if (net->obs_stride < net->obs_dim) return refuse(fn, who, ".obs_stride", "at least obs_dim");
  if (net->h_stride < net->enc_in || net->h_stride % 4 != 0) return refuse(fn, who, ".h_stride", "at least enc_in and a multiple of 4");
  if (const int rc = check_ptrs(fn, who, {{".obs", net->obs, 4}, {".h", net->h, 16}, {".out", net->out, 4}})) return rc;
  const int L = net->num_layers;
  for (int l = 0; l < kMaxL; ++l) {
    char wn[32], bn[32], an[32];
    snprintf(wn, sizeof wn, ".weight[%d]", l);
    snprintf(bn, sizeof bn, ".bias[%d]", l);
    snprintf(an, sizeof an, ".acts[%d]", l);
    if (l < L)
      if (const int rc = check_ptrs(fn, who, {{wn, net->weight[l], 4}, {bn, net->bias[l], 4}})) return rc;
    if (!train && net->acts[l]) return refuse(fn, who, an, "NULL (this launch has the inference form alone)");
    if (train) {
      if (l < (net->final_activation != LT_ACT_NONE ? L : L - 1)) {
        if (const int rc = check_ptr(fn, who, {an, net->acts[l], 4})) return rc;
      } else if (net->acts[l]) {
        return refuse(fn, who, an, "NULL (only hidden layers, and the embedding with a final activation, have a buffer)");
      }
    }
    e.weight[l] = l < L ? net->weight[l] : nullptr; e.bias[l] = l < L ? net->bias[l] : nullptr; e.acts[l] = train ? net->acts[l] : nullptr;
  }
  const long long ow = net->flat_dim + net->dims[L - 1];
  if (overlaps(net->out, (long long)n * ow, net->obs, (long long)(n - 1) * net->obs_stride + net->obs_dim))
    return refuse(fn, who, ".out", "a buffer that does not overlap obs");
  if (overlaps(net->out, (long long)n * ow, net->h, (long long)(n - 1) * net->h_stride + net->enc_in))
    return refuse(fn, who, ".out", "a buffer that does not overlap h");
  e.obs = net->obs; e.obs_stride = net->obs_stride; e.out = net->out;
  return LT_OK;
}

int cu_count() {
  static int cus = 0;  // (every device of a node is the same chip)
  if (cus == 0) {
    int dev = 0, v = 0;
    cus = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
  }
  return cus;
}

// Row block, panel height and the LDS carve of one launch (nets networks set in a.net): the largest row block that still gives every
// CU a workgroup, then the highest panel that fits beside its activations.  RB = PM = 16 always fits: 2 x 16 x 520 + 16 x 520 floats.
int plan(EncArgs& a, int nets) {
  int sa = 0, sb = 0, kp = 0, omax = 0;
  for (int k = 0; k < nets; ++k) {
    const EncNet& r = a.net[k];
    sa = r.stride[0] > sa ? r.stride[0] : sa;
    sb = r.stride[1] > sb ? r.stride[1] : sb;
    for (int l = 0; l < r.L; ++l) {
      kp = lds_stride(r.dims[l]) > kp ? lds_stride(r.dims[l]) : kp;
      omax = r.dims[l + 1] > omax ? r.dims[l + 1] : omax;
    }
  }
  const int cus = cu_count();
  for (const int rb : {64, 32, 16}) {
    if (rb > 16 && (long long)((a.n + rb - 1) / rb) * nets < cus) continue;
    for (const int pm : {64, 32, 16}) {
      if (pm > 16 && pm >= 2 * round_up(omax, 16)) continue;  // (higher than the widest layer: rows nobody reads)
      const int floats = rb * (sa + sb) + pm * kp;
      if (floats * (int)sizeof(float) > kLdsBytes) continue;
      a.RB = rb; a.PM = pm; a.off_b = rb * sa; a.off_panel = rb * (sa + sb);
      return floats * (int)sizeof(float);
    }
  }
  return 0;  // (unreachable for a validated descriptor)
}

// lt_rnn_encoder_forward and its training form: one body, `train` says which
int rnn_forward(const char* fn, const lt_rnn_encoder_net* actor, const lt_rnn_encoder_net* critic, int n, void* stream, bool train) {
  if (n < 1 || n > 16 * 65535) return refuse(fn, "", "n", "in [1, 16 * 65535]");
  lt_encoder_net ea, ec;
  if (const int rc = check_rnn_net(fn, "actor", actor, n, ea, train)) return rc;
  if (critic)
    if (const int rc = check_rnn_net(fn, "critic", critic, n, ec, train)) return rc;
  EncArgs a;
  const int nets = critic ? 2 : 1;
  set_net(a.net[0], &ea);
  set_net(a.net[1], critic ? &ec : &ea);
  a.net[0].h = actor->h; a.net[0].h_stride = actor->h_stride;
  a.net[1].h = critic ? critic->h : actor->h; a.net[1].h_stride = critic ? critic->h_stride : actor->h_stride;
  a.n = n;
  const int lds = plan(a, nets);
  if (lds <= 0) return refuse(fn, "the layers do not fit the LDS");
  if (const int e = lt_ensure_dynamic_lds((const void*)lt_encoder_kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  hipLaunchKernelGGL(lt_encoder_kernel, dim3((unsigned)((n + a.RB - 1) / a.RB), (unsigned)nets), dim3(256), lds, (hipStream_t)stream, a);
  return launch_status(fn);
}

// ---- the backward pass: checks, plan ----
int check_grad_widths(const char* fn, const char* who, const lt_rnn_encoder_grad* g) {
  if (!g) return refuse(fn, who, "", "non-null");
  if (g->flat_dim < 0) return refuse(fn, who, ".flat_dim", "at least 0");
  lt_encoder_desc d;
  d.obs_dim = g->flat_dim + 1; d.flat_dim = g->flat_dim; d.enc_in = g->enc_in; d.num_layers = g->num_layers;  // (no row bounds these widths)
  for (int l = 0; l < kMaxL; ++l) d.dims[l] = g->dims[l];
  d.activation = g->activation; d.final_activation = g->final_activation;
  return check_desc(fn, who, &d, false);
}

int check_grad(const char* fn, const char* who, const lt_rnn_encoder_grad* g, int n) {
  if (const int rc = check_grad_widths(fn, who, g)) return rc;
  const int L = g->num_layers, E = g->dims[L - 1];
  const long long ow = g->flat_dim + E;
  if (g->dx_stride < ow) return refuse(fn, who, ".dx_stride", "at least flat_dim + the embedding width");
  if (const int rc = check_ptrs(fn, who, {{".dx", g->dx, 4}, {".dh", g->dh, 16}})) return rc;
  if (g->final_activation == LT_ACT_TANH)
    if (const int rc = check_ptr(fn, who, {".out", g->out, 4})) return rc;
  const int need = g->final_activation != LT_ACT_NONE ? L : L - 1;
  for (int l = 0; l < L; ++l) {
    char wn[32], an[32], zn[32];
    snprintf(wn, sizeof wn, ".weight[%d]", l);
    snprintf(an, sizeof an, ".acts[%d]", l);
    snprintf(zn, sizeof zn, ".dz[%d]", l);
    if (const int rc = check_ptrs(fn, who, {{wn, g->weight[l], 4}, {zn, g->dz[l], 4}})) return rc;
    if (l < need)
      if (const int rc = check_ptr(fn, who, {an, g->acts[l], 4})) return rc;
  }
  // no output may overlap an array the launch reads, or another output of this network
  for (int k = 0; k <= L; ++k) {
    char on[32];
    if (k < L) snprintf(on, sizeof on, ".dz[%d]", k); else snprintf(on, sizeof on, ".dh");
    const float* o = k < L ? g->dz[k] : g->dh;
    const long long no = (long long)n * (k < L ? g->dims[k] : g->enc_in);
    for (int l = 0; l < L; ++l)
      if (overlaps(o, no, g->weight[l], (long long)g->dims[l] * (l ? g->dims[l - 1] : g->enc_in)))
        return refuse(fn, who, on, "a buffer that does not overlap a weight");
    for (int j = 0; j < k; ++j)
      if (overlaps(o, no, g->dz[j], (long long)n * g->dims[j])) return refuse(fn, who, on, "a buffer that does not overlap another output");
    if (overlaps(o, no, g->dx, (long long)(n - 1) * g->dx_stride + ow)) return refuse(fn, who, on, "a buffer that does not overlap dx");
    if (g->final_activation == LT_ACT_TANH && overlaps(o, no, g->out, (long long)n * ow)) return refuse(fn, who, on, "a buffer that does not overlap out");
    for (int l = 0; l < need; ++l)
      if (overlaps(o, no, g->acts[l], (long long)n * g->dims[l])) return refuse(fn, who, on, "a buffer that does not overlap acts");
  }
  return LT_OK;
}

void set_grad_net(EncGradNet& r, const lt_rnn_encoder_grad* g) {
  const int L = g->num_layers;
  r.dx = g->dx; r.dx_stride = g->dx_stride; r.out = g->out; r.dh = g->dh;
  r.flat_dim = g->flat_dim; r.L = L; r.act = g->activation; r.final_act = g->final_activation;
  r.dims[0] = g->enc_in;
  r.stride[0] = r.stride[1] = 0;
  for (int l = 0; l < kMaxL; ++l) {
    const bool used = l < L;
    r.w[l] = used ? g->weight[l] : nullptr; r.acts[l] = used ? g->acts[l] : nullptr; r.dz[l] = used ? g->dz[l] : nullptr;
    r.dims[l + 1] = used ? g->dims[l] : 0;
  }
  for (int t = 0; t < L; ++t)  // step t reads dz_{L-1-t}, dims[L - t] wide, from buffer t & 1
    if (lds_stride(r.dims[L - t]) > r.stride[t & 1]) r.stride[t & 1] = lds_stride(r.dims[L - t]);
}

// as `plan`: the panel holds PM INPUT features of a layer, each op = lds_stride(the layer's outputs) floats long
int plan_grad(EncGradArgs& a, int nets) {
  int sa = 0, sb = 0, op = 0, kmax = 0;
  for (int k = 0; k < nets; ++k) {
    const EncGradNet& r = a.net[k];
    sa = r.stride[0] > sa ? r.stride[0] : sa;
    sb = r.stride[1] > sb ? r.stride[1] : sb;
    for (int l = 0; l < r.L; ++l) {
      op = lds_stride(r.dims[l + 1]) > op ? lds_stride(r.dims[l + 1]) : op;
      kmax = r.dims[l] > kmax ? r.dims[l] : kmax;
    }
  }
  const int cus = cu_count();
  for (const int rb : {64, 32, 16}) {
    if (rb > 16 && (long long)((a.n + rb - 1) / rb) * nets < cus) continue;
    for (const int pm : {64, 32, 16}) {
      if (pm > 16 && pm >= 2 * round_up(kmax, 16)) continue;
      const int floats = rb * (sa + sb) + pm * op;
      if (floats * (int)sizeof(float) > kLdsBytes) continue;
      a.RB = rb; a.PM = pm; a.off_b = rb * sa; a.off_panel = rb * (sa + sb);
      return floats * (int)sizeof(float);
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int lt_encoder_validate(const lt_encoder_desc* desc) { return check_desc("lt_encoder_validate", "desc", desc); }

int lt_encoder_forward_launches(const lt_encoder_desc* actor, const lt_encoder_desc* critic) {
  const char* fn = "lt_encoder_forward_launches";
  if (const int rc = check_desc(fn, "actor", actor)) return rc;
  if (critic)
    if (const int rc = check_desc(fn, "critic", critic)) return rc;
  return 1;
}

int lt_encoder_forward(const lt_encoder_net* actor, const lt_encoder_net* critic, int n, void* stream) {
  const char* fn = "lt_encoder_forward";
  if (n < 1 || n > 16 * 65535) return refuse(fn, "", "n", "in [1, 16 * 65535]");
  if (const int rc = check_net(fn, "actor", actor, n)) return rc;
  if (critic)
    if (const int rc = check_net(fn, "critic", critic, n)) return rc;
  EncArgs a;
  const int nets = critic ? 2 : 1;
  set_net(a.net[0], actor);
  set_net(a.net[1], critic ? critic : actor);
  a.n = n;
  const int lds = plan(a, nets);
  if (lds <= 0) return refuse(fn, "the layers do not fit the LDS");
  if (const int e = lt_ensure_dynamic_lds((const void*)lt_encoder_kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  hipLaunchKernelGGL(lt_encoder_kernel, dim3((unsigned)((n + a.RB - 1) / a.RB), (unsigned)nets), dim3(256), lds, (hipStream_t)stream, a);
  return launch_status(fn);
}

int lt_rnn_encoder_forward_launches(const lt_rnn_encoder_net* actor, const lt_rnn_encoder_net* critic) {
  const char* fn = "lt_rnn_encoder_forward_launches";
  if (!actor) return refuse(fn, "actor", "", "non-null");
  const lt_encoder_desc da = desc_of(actor);
  if (const int rc = check_desc(fn, "actor", &da, false)) return rc;
  if (critic) {
    const lt_encoder_desc dc = desc_of(critic);
    if (const int rc = check_desc(fn, "critic", &dc, false)) return rc;
  }
  return 1;
}

int lt_rnn_encoder_forward(const lt_rnn_encoder_net* actor, const lt_rnn_encoder_net* critic, int n, void* stream) {
  return rnn_forward("lt_rnn_encoder_forward", actor, critic, n, stream, false);
}

int lt_rnn_encoder_forward_train(const lt_rnn_encoder_net* actor, const lt_rnn_encoder_net* critic, int n, void* stream) {
  return rnn_forward("lt_rnn_encoder_forward_train", actor, critic, n, stream, true);
}

int lt_rnn_encoder_backward_launches(const lt_rnn_encoder_grad* actor, const lt_rnn_encoder_grad* critic) {
  const char* fn = "lt_rnn_encoder_backward_launches";
  if (const int rc = check_grad_widths(fn, "actor", actor)) return rc;
  if (critic)
    if (const int rc = check_grad_widths(fn, "critic", critic)) return rc;
  return 1;
}

int lt_rnn_encoder_backward(const lt_rnn_encoder_grad* actor, const lt_rnn_encoder_grad* critic, int n, void* stream) {
  const char* fn = "lt_rnn_encoder_backward";
  if (n < 1 || n > 16 * 65535) return refuse(fn, "", "n", "in [1, 16 * 65535]");
  if (const int rc = check_grad(fn, "actor", actor, n)) return rc;
  if (critic)
    if (const int rc = check_grad(fn, "critic", critic, n)) return rc;
  EncGradArgs a;
  const int nets = critic ? 2 : 1;
  set_grad_net(a.net[0], actor);
  set_grad_net(a.net[1], critic ? critic : actor);
  a.n = n;
  const int lds = plan_grad(a, nets);
  if (lds <= 0) return refuse(fn, "the layers do not fit the LDS");
  if (const int e = lt_ensure_dynamic_lds((const void*)lt_rnn_encoder_backward_kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  hipLaunchKernelGGL(lt_rnn_encoder_backward_kernel, dim3((unsigned)((n + a.RB - 1) / a.RB), (unsigned)nets), dim3(256), lds, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // extern "C"
