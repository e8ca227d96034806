// lt_student.hip - one fused inference step of the deployed student policy (include/lt_student.h).
//
// `Student.forward` on one env step is ~25 library launches (three MIOpen convolutions, a pool, ReLUs, torch.gru_cell, nine Linear +
// ELU, a cat, the masked reset); the arithmetic is ~1.6 M multiply-adds per env.  Here the step is THREE launches on the caller's
// stream, all f32 (exact products, f32 accumulation), every sum in one fixed order that depends neither on n nor on a row's place:
//   launch 1  lt_student_encoder_kernel: a workgroup owns 8 envs.  Their tactile rows are staged in LDS and the conv stack runs map
//             to map between two LDS buffers (conv + bias + ReLU, the 2 x 2 max-pool folded into the conv that feeds it); the Linear
//             head writes the embedding to the scratch.  Direct convolution on the VALU: a lane owns one (env, output position), a
//             wave owns six output channels, so a weight is WAVE-UNIFORM - it arrives through the scalar cache into an SGPR and costs
//             neither LDS space nor a vector load (the packed weights are transposed so that the six lie side by side).  An im2col
//             form on the matrix cores would have to build its 16-row operand tiles in LDS first (conv 1 has K = 32: two thirds of
//             the work would be the gather), for 215 k MACs per env.
//   launch 2  lt_student_gru_kernel: grid (H / 64, row tiles of 16).  The tile's [x | h] rows are staged in LDS - the done mask
//             zeroes h as it is read - and each of the four waves owns 16 hidden units: gates r, z and the two halves of n against
//             [W_ih | W_hh] on v_mfma_f32_16x16x4_f32 (the operand trick of lt_seq_tile.h: MFMA step s of a 16-wide k block consumes
//             k = kb + 4 q + s, one 16-byte load per four MFMAs), four accumulator chains per gate (independent MFMAs back to back,
//             and a shorter rounding chain).  The gate arithmetic is the epilogue.  The new state goes to the scratch, NOT to h:
//             the other seven workgroups of the row tile are still reading the old one.
//   launch 3  lt_student_mlp_kernel: a workgroup owns 16 rows.  It copies the new state into h (in place from the caller's view),
//             runs the encoder MLP between two LDS buffers, lets its last layer write the embedding BESIDE the proprioception columns
//             (read in place through the row stride) so that the concatenation never exists in memory, runs the backbone and writes
//             the actions.  Same MFMA scheme; weights zero-padded to multiples of 16 by the pack, so tails take the same arithmetic.
// lt_student_pack is one launch: a table of (source, destination, shape, transpose) segments.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "lt_cnn_device.h"
#include "lt_device_prims.h"
#include "lt_host_check.h"
#include "lt_internal.h"

static_assert(LT_STUDENT_MAX_MLP_LAYERS == LT_MLP_MAX_LAYERS, "lt_student.h mirrors lt_env.h");

namespace {

using lt::f32x4;

using lt_cnn::EncArgs;
using lt_cnn::ET;
using lt_cnn::MAX_LDS;
using lt_cnn::MAXC;
using lt_cnn::pad4;
using lt_cnn::TPB;
constexpr int RT = LT_STUDENT_ROW_TILE;
constexpr int UT = LT_STUDENT_GRU_TILE;
constexpr int MLP_TPB = 1024;     // launch 3: 16 waves, a layer's 16-unit column tiles spread over them
constexpr int KU = 8;             // k blocks of 16 whose operand loads are in flight together (launches 2: 4, 3: 8)
constexpr int GU = 4;
constexpr int MAXL = LT_STUDENT_MAX_MLP_LAYERS;
constexpr int MAX_SEGS = 6 * MAXC + 8 + 4 * MAXL;

__host__ __device__ constexpr int pad16(int x) { return (x + 15) & ~15; }

__device__ __forceinline__ float sigmoid_(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float elu_(float x) { return x > 0.f ? x : expm1f(x); }

// ---- launch 1: tactile encoder (lt_cnn_device.h: the conv stack is shared with the training form of the CNN head) -------------------------
__global__ __launch_bounds__(TPB) void lt_student_encoder_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  lt_cnn::encoder_tile(a, lds);
}

// ---- launch 2: GRU cell ---------------------------------------------------------------------------------------------------------
struct GruArgs {
  const float *emb, *h;
  const unsigned char* done;
  const float *w, *bi, *bh;  // packed [3H][D + H] = [W_ih | W_hh], [3H], [3H]
  float* hnew;               // [n][H] (scratch)
  long long n;
  int D, H;
};

__device__ __forceinline__ f32x4 sum4(const f32x4 a[4]) { return (a[0] + a[1]) + (a[2] + a[3]); }

__global__ __launch_bounds__(TPB) void lt_student_gru_kernel(const GruArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = lt::wave_uniform(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int D = a.D, H = a.H, K = D + H, S = K + 4;
  const long long row0 = (long long)blockIdx.y * RT;
  for (int idx = tid; idx < RT * K; idx += TPB) {
    const int r = idx / K, c = idx - r * K;
    const long long row = row0 + r;
    float v = 0.f;
    if (row < a.n) {
      if (c < D) v = a.emb[row * D + c];
      else if (!(a.done && a.done[row])) v = a.h[row * H + (c - D)];
    }
    lds[r * S + c] = v;
  }
  __syncthreads();
  const int u0 = blockIdx.x * UT + wave * 16;
  const float* wr = a.w + (long long)(u0 + i) * K + 4 * q;
  const long long gate = (long long)H * K;
  const float* xr = lds + i * S + 4 * q;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 ar[4] = {zero, zero, zero, zero}, az[4] = {zero, zero, zero, zero}, ax[4] = {zero, zero, zero, zero}, ah[4] = {zero, zero, zero, zero};
  // k blocks [0, D) feed r, z and the input half of n; [D, K) feed r, z and the hidden half.  GU blocks' loads are in flight together.
  for (int part = 0; part < 2; ++part) {
    const int k0 = part ? D : 0, k1 = part ? K : D;
    for (int kb0 = k0; kb0 < k1; kb0 += 16 * GU) {
      f32x4 wrv[GU], wzv[GU], wnv[GU], xv[GU];
#pragma unroll
      for (int j = 0; j < GU; ++j) {
        const int kb = kb0 + 16 * j < k1 ? kb0 + 16 * j : k0;
        wrv[j] = *(const f32x4*)(wr + kb); wzv[j] = *(const f32x4*)(wr + gate + kb); wnv[j] = *(const f32x4*)(wr + 2 * gate + kb);
        xv[j] = *(const f32x4*)(xr + kb);
      }
      lt::sched_fence();
#pragma unroll
      for (int j = 0; j < GU; ++j) {
        if (kb0 + 16 * j < k1) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            ar[s] = lt::mfma_16x16x4(wrv[j][s], xv[j][s], ar[s]);
            az[s] = lt::mfma_16x16x4(wzv[j][s], xv[j][s], az[s]);
            if (part) ah[s] = lt::mfma_16x16x4(wnv[j][s], xv[j][s], ah[s]);
            else ax[s] = lt::mfma_16x16x4(wnv[j][s], xv[j][s], ax[s]);
          }
        }
      }
    }
  }
  // acc[v] of lane (i, q): unit u0 + 4 q + v of row row0 + i
  const f32x4 sr = sum4(ar), sz = sum4(az), sx = sum4(ax), sh = sum4(ah);
  const int u = u0 + 4 * q;
  const f32x4 hp = *(const f32x4*)(lds + i * S + D + u);
  f32x4 o;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float r = sigmoid_((sr[v] + a.bi[u + v]) + a.bh[u + v]);
    const float z = sigmoid_((sz[v] + a.bi[H + u + v]) + a.bh[H + u + v]);
    const float nn = tanhf((sx[v] + a.bi[2 * H + u + v]) + r * (sh[v] + a.bh[2 * H + u + v]));
    o[v] = nn + z * (hp[v] - nn);
  }
  if (row0 + i < a.n) *(f32x4*)(a.hnew + (row0 + i) * H + u) = o;
}

// ---- launch 3: encoder MLP, concatenation, backbone ----------------------------------------------------------------------------------
struct Mlp {
  int L, kpad[MAXL], n[MAXL], npad[MAXL];
  const float *w[MAXL], *b[MAXL];  // packed [npad][kpad], [npad]
};
struct MlpArgs {
  const float* hnew;
  float* h;
  const float* proprio;
  long long pstride, n;
  float* actions;
  int H, P, S, cat_pad;  // S: row stride of both LDS buffers; cat_pad: padded width of the backbone's input row
  Mlp enc, bb;
};

// out[r][col0 + u] = act(sum_k W[u][k] in[r][k] + b[u]) for the tile's 16 rows and u < npad; GLOBAL: rows < n and u < N go to gout.
template <bool GLOBAL>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ W, const float* __restrict__ bias, int kpad, int N, int npad, bool act,
                                          const float* in, float* out, int S, int col0, float* gout, long long row0, long long n) {
  const int lane = threadIdx.x & 63, wave = lt::wave_uniform(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const float* xr = in + i * S + 4 * q;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int ut = wave; ut < npad / 16; ut += MLP_TPB / 64) {
    const float* wr = W + (long long)(ut * 16 + i) * kpad + 4 * q;
    f32x4 acc[4] = {zero, zero, zero, zero};
    for (int kb0 = 0; kb0 < kpad; kb0 += 16 * KU) {  // KU weight loads in flight before the first MFMA: one L2 round trip per KU k-blocks
      f32x4 wv[KU], xv[KU];
#pragma unroll
      for (int j = 0; j < KU; ++j) {
        const int kb = kb0 + 16 * j < kpad ? kb0 + 16 * j : 0;  // past the end: a valid address, its MFMAs are skipped
        wv[j] = *(const f32x4*)(wr + kb);
        xv[j] = *(const f32x4*)(xr + kb);
      }
      lt::sched_fence();
#pragma unroll
      for (int j = 0; j < KU; ++j) {
        if (kb0 + 16 * j < kpad) {
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[s] = lt::mfma_16x16x4(wv[j][s], xv[j][s], acc[s]);
        }
      }
    }
    const f32x4 sum = sum4(acc);
    const int u = ut * 16 + 4 * q;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float y = sum[v] + bias[u + v];
      if (act) y = elu_(y);
      if (GLOBAL) {
        if (u + v < N && row0 + i < n) gout[(row0 + i) * N + u + v] = y;
      } else {
        out[i * S + col0 + u + v] = y;
      }
    }
  }
}

__global__ __launch_bounds__(MLP_TPB) void lt_student_mlp_kernel(const MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, S = a.S, H = a.H, P = a.P;
  const long long row0 = (long long)blockIdx.x * RT;
  for (int idx = tid; idx < RT * (H / 4); idx += MLP_TPB) {
    const int r = idx / (H / 4), c = 4 * (idx - r * (H / 4));
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + r < a.n) {
      v = *(const f32x4*)(a.hnew + (row0 + r) * H + c);
      *(f32x4*)(a.h + (row0 + r) * H + c) = v;
    }
    *(f32x4*)(lds + r * S + c) = v;
  }
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < a.enc.L; ++l) {
    const bool last = l == a.enc.L - 1;
    float* out = lds + (cur ^ 1) * RT * S;
    if (last) {  // the backbone's input row: proprioception | embedding | zeros up to cat_pad
      for (int idx = tid; idx < RT * P; idx += MLP_TPB) {
        const int r = idx / P, c = idx - r * P;
        out[r * S + c] = row0 + r < a.n ? a.proprio[(row0 + r) * a.pstride + c] : 0.f;
      }
      const int z0 = P + a.enc.npad[l], zn = a.cat_pad - z0;
      for (int idx = tid; idx < RT * zn; idx += MLP_TPB) {
        const int r = idx / zn, c = idx - r * zn;
        out[r * S + z0 + c] = 0.f;
      }
    }
    mlp_layer<false>(a.enc.w[l], a.enc.b[l], a.enc.kpad[l], a.enc.n[l], a.enc.npad[l], !last, lds + cur * RT * S, out, S, last ? P : 0, nullptr, row0, a.n);
    __syncthreads();
    cur ^= 1;
  }
  for (int l = 0; l < a.bb.L; ++l) {
    const bool last = l == a.bb.L - 1;
    if (last) mlp_layer<true>(a.bb.w[l], a.bb.b[l], a.bb.kpad[l], a.bb.n[l], a.bb.npad[l], false, lds + cur * RT * S, nullptr, S, 0, a.actions, row0, a.n);
    else mlp_layer<false>(a.bb.w[l], a.bb.b[l], a.bb.kpad[l], a.bb.n[l], a.bb.npad[l], true, lds + cur * RT * S, lds + (cur ^ 1) * RT * S, S, 0, nullptr, row0, a.n);
    __syncthreads();
    cur ^= 1;
  }
}

// ---- pack ---------------------------------------------------------------------------------------------------------------------------
// dst[r][coff + c] (r < dr, c < dc, row stride ld) = src[r][c] of the [sr][sc] source, or src[c][r] when transposed; 0 outside it
struct Seg {
  const float* src;
  float* dst;
  int sr, sc, dr, dc, ld, coff, transpose;
};
struct PackArgs {
  int nseg;
  Seg seg[MAX_SEGS];
};

__global__ __launch_bounds__(TPB) void lt_student_pack_kernel(const PackArgs a) {
  const Seg& s = a.seg[blockIdx.y];
  const long long total = (long long)s.dr * s.dc;
  for (long long idx = (long long)blockIdx.x * TPB + threadIdx.x; idx < total; idx += (long long)gridDim.x * TPB) {
    const int r = (int)(idx / s.dc), c = (int)(idx - (long long)r * s.dc);
    float v = 0.f;
    if (s.transpose) { if (r < s.sc && c < s.sr) v = s.src[(long long)c * s.sc + r]; }
    else if (r < s.sr && c < s.sc) v = s.src[(long long)r * s.sc + c];
    s.dst[(long long)r * s.ld + s.coff + c] = v;
  }
}

// ---- host: validation and layout -----------------------------------------------------------------------------------------------------
struct Layout : lt_cnn::Geometry {
  size_t conv_w[MAXC], conv_b[MAXC], head_w, head_b, gru_w, gru_bi, gru_bh, enc_w[MAXL], enc_b[MAXL], bb_w[MAXL], bb_b[MAXL], total;
  int S, cat_pad, gru_bytes, mlp_bytes;
};

int check_mlp(const lt_mlp_desc& m, const char* name, int in_width, int max_in) {
  char msg[160];
  const char* bad = nullptr;
  if (m.num_layers < 1 || m.num_layers > LT_MLP_MAX_LAYERS) bad = "num_layers must be in [1, LT_MLP_MAX_LAYERS]";
  else if (m.input_format != LT_ROWS_F32) bad = "input_format must be LT_ROWS_F32 (bf16 rows are not served)";
  else if (m.activation != LT_ACT_ELU) bad = "activation must be LT_ACT_ELU";
  else if (m.dims[0] != in_width) bad = "dims[0] does not match what feeds the network";
  else if (m.dims[0] < 1 || m.dims[0] > max_in) bad = "dims[0] is outside the served input widths";
  else
    for (int l = 1; l <= m.num_layers; ++l)
      if (m.dims[l] < 1 || m.dims[l] > 512) bad = "dims[l + 1] must be in [1, 512] (lt_mlp_desc's limit)";
  if (!bad) return LT_OK;
  snprintf(msg, sizeof msg, "%s.%s", name, bad);
  return refuse("lt_student_desc", msg);
}

int layout_of(const lt_student_desc* d, Layout* L) {
  if (!d) return refuse("lt_student_desc", "desc is NULL");
  if (d->rnn_type != LT_STUDENT_RNN_GRU) return refuse("lt_student_desc", "rnn_type must be LT_STUDENT_RNN_GRU (an LSTM is not served)");
  if (d->rnn_layers != 1) return refuse("lt_student_desc", "rnn_layers must be 1");
  if (const char* why = lt_cnn::geometry_of(d, L)) return refuse("lt_student_desc", why);
  if (d->rnn_hidden < UT || d->rnn_hidden > 512 || d->rnn_hidden % UT) return refuse("lt_student_desc", "rnn_hidden must be a multiple of LT_STUDENT_GRU_TILE (64), at most 512");
  if (d->proprio_dim < 0 || d->proprio_dim > 512) return refuse("lt_student_desc", "proprio_dim must be in [0, 512]");
  if (const int rc = check_mlp(d->encoder, "encoder", d->rnn_hidden, 512)) return rc;
  const int enc_out = d->encoder.dims[d->encoder.num_layers];
  if (const int rc = check_mlp(d->backbone, "backbone", d->proprio_dim + enc_out, 512)) return rc;
  // packed layout: every block starts on a multiple of 4 floats
  size_t off = 0;
  auto take = [&](size_t floats) { const size_t at = off; off += (floats + 3) & ~(size_t)3; return at; };
  for (int l = 0; l < d->num_convs; ++l) {
    const int kk = d->conv_kernel[l] * d->conv_kernel[l];
    L->conv_w[l] = take((size_t)L->c[l] * kk * L->c[l + 1]);
    L->conv_b[l] = take(L->c[l + 1]);
  }
  const int D = d->head_out, H = d->rnn_hidden;
  L->head_w = take((size_t)L->flat * D); L->head_b = take(D);
  L->gru_w = take((size_t)3 * H * (D + H)); L->gru_bi = take(3 * H); L->gru_bh = take(3 * H);
  int widest = pad16(H);
  for (int l = 0; l < d->encoder.num_layers; ++l) {
    const int kp = pad16(d->encoder.dims[l]), np = pad16(d->encoder.dims[l + 1]);
    L->enc_w[l] = take((size_t)np * kp); L->enc_b[l] = take(np);
    if (np > widest) widest = np;
  }
  L->cat_pad = pad16(d->proprio_dim + pad16(enc_out));
  if (L->cat_pad > widest) widest = L->cat_pad;
  for (int l = 0; l < d->backbone.num_layers; ++l) {
    const int kp = l == 0 ? L->cat_pad : pad16(d->backbone.dims[l]), np = pad16(d->backbone.dims[l + 1]);
    L->bb_w[l] = take((size_t)np * kp); L->bb_b[l] = take(np);
    if (np > widest) widest = np;
  }
  L->total = off;
  L->S = widest + 4;
  L->mlp_bytes = 2 * RT * L->S * (int)sizeof(float);
  L->gru_bytes = RT * (D + H + 4) * (int)sizeof(float);
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_student_validate(const lt_student_desc* desc) {
  Layout L;
  return layout_of(desc, &L);
}

int lt_student_packed_floats(const lt_student_desc* desc, size_t* floats) {
  Layout L;
  if (const int rc = layout_of(desc, &L)) return rc;
  if (!floats) return einval("lt_student_packed_floats: floats is NULL");
  *floats = L.total;
  return LT_OK;
}

int lt_student_ws_floats(const lt_student_desc* desc, int64_t n, size_t* floats) {
  Layout L;
  if (const int rc = layout_of(desc, &L)) return rc;
  if (!floats || n <= 0 || n > INT32_MAX) return einval("lt_student_ws_floats: floats non-null and n in [1, 2^31)");
  *floats = (size_t)n * (size_t)(desc->head_out + desc->rnn_hidden);
  return LT_OK;
}

int lt_student_step_launches(const lt_student_desc* desc, int64_t n) {
  Layout L;
  if (const int rc = layout_of(desc, &L)) return rc;
  if (n <= 0 || n > INT32_MAX) return einval("lt_student_step_launches: n must be in [1, 2^31)");
  return 3;
}

int lt_student_pack(const lt_student_desc* desc, const lt_student_params* p, float* packed, void* stream) {
  Layout L;
  if (const int rc = layout_of(desc, &L)) return rc;
  if (!p || !packed || (uintptr_t)packed % 16) return einval("lt_student_pack: params and a 16-byte aligned packed buffer are required");
  PackArgs a;
  a.nseg = 0;
  bool missing = false;
  auto seg = [&](const float* src, size_t dst, int sr, int sc, int dr, int dc, int ld, int coff, int transpose) {
    missing = missing || !src;
    a.seg[a.nseg++] = Seg{src, packed + dst, sr, sc, dr, dc, ld, coff, transpose};
  };
  for (int l = 0; l < desc->num_convs; ++l) {
    const int kk = L.c[l] * desc->conv_kernel[l] * desc->conv_kernel[l], co = L.c[l + 1];
    seg(p->conv_w[l], L.conv_w[l], co, kk, kk, co, co, 0, 1);
    seg(p->conv_b[l], L.conv_b[l], 1, co, 1, co, co, 0, 0);
  }
  const int D = desc->head_out, H = desc->rnn_hidden;
  seg(p->head_w, L.head_w, D, L.flat, L.flat, D, D, 0, 1);
  seg(p->head_b, L.head_b, 1, D, 1, D, D, 0, 0);
  seg(p->gru_w_ih, L.gru_w, 3 * H, D, 3 * H, D, D + H, 0, 0);
  seg(p->gru_w_hh, L.gru_w, 3 * H, H, 3 * H, H, D + H, D, 0);
  seg(p->gru_b_ih, L.gru_bi, 1, 3 * H, 1, 3 * H, 3 * H, 0, 0);
  seg(p->gru_b_hh, L.gru_bh, 1, 3 * H, 1, 3 * H, 3 * H, 0, 0);
  for (int l = 0; l < desc->encoder.num_layers; ++l) {
    const int k = desc->encoder.dims[l], n = desc->encoder.dims[l + 1], kp = pad16(k), np = pad16(n);
    seg(p->enc_w[l], L.enc_w[l], n, k, np, kp, kp, 0, 0);
    seg(p->enc_b[l], L.enc_b[l], 1, n, 1, np, np, 0, 0);
  }
  for (int l = 0; l < desc->backbone.num_layers; ++l) {
    const int k = desc->backbone.dims[l], n = desc->backbone.dims[l + 1], kp = l == 0 ? L.cat_pad : pad16(k), np = pad16(n);
    seg(p->bb_w[l], L.bb_w[l], n, k, np, kp, kp, 0, 0);
    seg(p->bb_b[l], L.bb_b[l], 1, n, 1, np, np, 0, 0);
  }
  if (missing) return einval("lt_student_pack: a parameter pointer the descriptor needs is NULL");
  hipLaunchKernelGGL(lt_student_pack_kernel, dim3(64, (unsigned)a.nseg), dim3(TPB), 0, (hipStream_t)stream, a);
  return launch_status("lt_student_pack");
}

int lt_student_step(const lt_student_desc* desc, const float* packed, const float* proprio, int64_t proprio_row_stride, const float* tactile,
                    int64_t tactile_row_stride, const uint8_t* done_mask, float* h, int64_t n, float* actions_out, float* ws, void* stream) {
  Layout L;
  if (const int rc = layout_of(desc, &L)) return rc;
  const int img = L.c[0] * L.h[0] * L.w[0];
  if (!packed || !tactile || !h || !actions_out || !ws || (desc->proprio_dim > 0 && !proprio) || n <= 0 || n > INT32_MAX ||
      proprio_row_stride < desc->proprio_dim || tactile_row_stride < img || (uintptr_t)packed % 16 || (uintptr_t)h % 16 || (uintptr_t)ws % 16)
    return einval("lt_student_step: packed, tactile, h, actions_out, ws (and proprio) non-null; packed, h and ws 16-byte aligned; n in [1, 2^31); "
                  "row strides at least the row widths");
  const int D = desc->head_out, H = desc->rnn_hidden;
  float* emb = ws;
  float* hnew = ws + (size_t)n * D;  // D % 16 == 0: aligned
  EncArgs e;
  e.tactile = tactile; e.tstride = tactile_row_stride; e.n = n; e.emb = emb;
  lt_cnn::fill_enc_args(desc, L, &e);
  for (int l = 0; l < MAXC; ++l) {
    const bool on = l < desc->num_convs;
    e.cw[l] = on ? packed + L.conv_w[l] : nullptr; e.cb[l] = on ? packed + L.conv_b[l] : nullptr;
  }
  e.hw = packed + L.head_w; e.hb = packed + L.head_b;
  GruArgs g;
  g.emb = emb; g.h = h; g.done = done_mask; g.w = packed + L.gru_w; g.bi = packed + L.gru_bi; g.bh = packed + L.gru_bh; g.hnew = hnew; g.n = n;
  g.D = D; g.H = H;
  MlpArgs m;
  m.hnew = hnew; m.h = h; m.proprio = proprio; m.pstride = proprio_row_stride; m.n = n; m.actions = actions_out;
  m.H = H; m.P = desc->proprio_dim; m.S = L.S; m.cat_pad = L.cat_pad;
  const lt_mlp_desc* md[2] = {&desc->encoder, &desc->backbone};
  Mlp* mm[2] = {&m.enc, &m.bb};
  for (int t = 0; t < 2; ++t) {
    mm[t]->L = md[t]->num_layers;
    for (int l = 0; l < MAXL; ++l) {
      const bool on = l < md[t]->num_layers;
      mm[t]->kpad[l] = !on ? 0 : (t == 1 && l == 0) ? L.cat_pad : pad16(md[t]->dims[l]);
      mm[t]->n[l] = on ? md[t]->dims[l + 1] : 0;
      mm[t]->npad[l] = on ? pad16(md[t]->dims[l + 1]) : 0;
      mm[t]->w[l] = on ? packed + (t ? L.bb_w[l] : L.enc_w[l]) : nullptr;
      mm[t]->b[l] = on ? packed + (t ? L.bb_b[l] : L.enc_b[l]) : nullptr;
    }
  }
  const struct { const void* k; int bytes; } dyn[3] = {{(const void*)lt_student_encoder_kernel, L.enc_bytes},
                                                      {(const void*)lt_student_gru_kernel, L.gru_bytes},
                                                      {(const void*)lt_student_mlp_kernel, L.mlp_bytes}};
  for (const auto& k : dyn)
    if (k.bytes > 64 * 1024)
      if (const int err = lt_ensure_dynamic_lds(k.k, MAX_LDS)) { lt_set_error(lt_hip_error_string(err)); return LT_EHIP; }
  const unsigned tiles = (unsigned)((n + RT - 1) / RT);
  hipLaunchKernelGGL(lt_student_encoder_kernel, dim3((unsigned)((n + ET - 1) / ET)), dim3(TPB), (size_t)L.enc_bytes, (hipStream_t)stream, e);
  hipLaunchKernelGGL(lt_student_gru_kernel, dim3((unsigned)(H / UT), tiles), dim3(TPB), (size_t)L.gru_bytes, (hipStream_t)stream, g);
  hipLaunchKernelGGL(lt_student_mlp_kernel, dim3(tiles), dim3(MLP_TPB), (size_t)L.mlp_bytes, (hipStream_t)stream, m);
  return launch_status("lt_student_step");
}

}  // extern "C"
