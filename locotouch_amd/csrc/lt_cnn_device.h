// lt_cnn_device.h - the tactile conv stack (conv + bias + ReLU, optional 2 x 2 max-pool, Linear head) as device code shared by the
// student's inference step (lt_student.hip, launch 1) and the training form of the CNN head (lt_cnn_train.hip): ONE source for the
// forward arithmetic, so a row's embedding has the same bits from both, and one geometry check for both descriptors.
#pragma once

#include <hip/hip_runtime.h>

#include "lt_device_prims.h"
#include "lt_internal.h"

namespace lt_cnn {

constexpr int TPB = 256;
constexpr int ET = LT_STUDENT_ENV_TILE;  // images of one workgroup
constexpr int OCB = 6;                   // output channels a wave accumulates per (image, position)
constexpr int MAXC = LT_STUDENT_MAX_CONVS;
constexpr int MAX_LDS = 160 * 1024;

__host__ __device__ constexpr int pad4(int x) { return (x + 3) & ~3; }

struct EncArgs {
  const float* tactile;
  long long tstride, n;
  float* emb;                        // [n][D]
  const float *cw[MAXC], *cb[MAXC];  // packed: weight [Cin * K * K][Cout], bias [Cout]
  const float *hw, *hb;              // packed head: [flat][D], [D]
  int nconv, c[MAXC + 1], h[MAXC + 1], w[MAXC + 1], k[MAXC], cs[MAXC], pool[MAXC];
  int flat, D, buf_floats[2];        // per-image floats of the two LDS buffers (maps 0, 2 / maps 1, 3)
};

// out[e][oc][y][x] = max over the P x P pool window of relu(conv(in)[e][oc][..] + b[oc]) (P = 1: no pool) for a workgroup of NT threads.
// ARG: arg[e][oc][y][x] = the window's FIRST maximum in row-major window order (dy * P + dx), what the pool's backward pays.
template <int P, int NT = TPB, bool ARG = false>
__device__ void conv_layer(const float* in, float* out, const float* __restrict__ wt, const float* __restrict__ bias, int Cin, int H, int W,
                           int Cout, int K, int cs, int Ho, int Wo, unsigned char* arg = nullptr) {
  const int lane = threadIdx.x & 63, wave = lt::wave_uniform(threadIdx.x >> 6);
  const int npos = Ho * Wo, items = ET * npos, chunks = (items + 63) / 64, groups = (Cout + OCB - 1) / OCB;
  for (int t = wave; t < groups * chunks; t += NT / 64) {
    const int oc0 = (t % groups) * OCB, it_raw = (t / groups) * 64 + lane;
    const int it = it_raw < items ? it_raw : items - 1;  // a lane past the end repeats the last item and stores nothing: uniform control flow
    const int e = it / npos, p = it - e * npos, y = p / Wo, x = p - y * Wo;
    float acc[OCB][P * P];
#pragma unroll
    for (int o = 0; o < OCB; ++o)
#pragma unroll
      for (int d = 0; d < P * P; ++d) acc[o][d] = 0.f;
    const float* base = in + e * Cin * H * W + (y * P * cs) * W + x * P * cs;
    for (int ic = 0; ic < Cin; ++ic) {
      for (int ky = 0; ky < K; ++ky) {
        for (int kx = 0; kx < K; ++kx) {
          const float* wp = wt + ((ic * K + ky) * K + kx) * Cout + oc0;
          float wv[OCB];
#pragma unroll
          for (int o = 0; o < OCB; ++o) wv[o] = oc0 + o < Cout ? wp[o] : 0.f;
          const float* ip = base + (ic * H + ky) * W + kx;
#pragma unroll
          for (int dy = 0; dy < P; ++dy)
#pragma unroll
            for (int dx = 0; dx < P; ++dx) {
              const float v = ip[dy * cs * W + dx * cs];
#pragma unroll
              for (int o = 0; o < OCB; ++o) acc[o][dy * P + dx] = fmaf(wv[o], v, acc[o][dy * P + dx]);
            }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < OCB; ++o) {
      if (oc0 + o >= Cout || it_raw >= items) break;
      float m = acc[o][0];
      if constexpr (ARG) {
        int best = 0;
#pragma unroll
        for (int d = 1; d < P * P; ++d)
          if (acc[o][d] > m) { m = acc[o][d]; best = d; }
        arg[(e * Cout + oc0 + o) * npos + p] = (unsigned char)best;
      } else {
#pragma unroll
        for (int d = 1; d < P * P; ++d) m = fmaxf(m, acc[o][d]);
      }
      out[(e * Cout + oc0 + o) * npos + p] = fmaxf(m + bias[oc0 + o], 0.f);
    }
  }
}

// out[e][o] = head_b[o] + sum_k head_w[k][o] in[e][k] for the tile's ET images; rows < n go to a.emb
__device__ __forceinline__ void head_layer(const EncArgs& a, const float* in, long long row0) {
  const int flat = a.flat, D = a.D;
  for (int it = threadIdx.x; it < ET * D; it += TPB) {
    const int e = it / D, o = it - e * D;
    const float* x = in + e * flat;
    const float* wp = a.hw + o;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = 0;
    for (; k + 3 < flat; k += 4) {
      s0 = fmaf(wp[(k + 0) * D], x[k + 0], s0);
      s1 = fmaf(wp[(k + 1) * D], x[k + 1], s1);
      s2 = fmaf(wp[(k + 2) * D], x[k + 2], s2);
      s3 = fmaf(wp[(k + 3) * D], x[k + 3], s3);
    }
    for (; k < flat; ++k) s0 = fmaf(wp[k * D], x[k], s0);
    if (row0 + e < a.n) a.emb[(row0 + e) * D + o] = ((s0 + s1) + (s2 + s3)) + a.hb[o];
  }
}

// The whole encoder of the tile of ET images that starts at row blockIdx.x * ET (a workgroup of TPB threads, dynamic LDS `lds`).
__device__ __forceinline__ void encoder_tile(const EncArgs& a, float* lds) {
  const int boff[2] = {0, ET * a.buf_floats[0]};
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * ET;
  const int img = a.c[0] * a.h[0] * a.w[0];
  for (int i = tid; i < ET * img; i += TPB) {
    const int e = i / img, c = i - e * img;
    lds[i] = row0 + e < a.n ? a.tactile[(row0 + e) * a.tstride + c] : 0.f;  // a tail image computes on zeros and stores nothing
  }
  __syncthreads();
  for (int l = 0; l < a.nconv; ++l) {
    const float* in = lds + boff[l & 1];
    float* out = lds + boff[(l + 1) & 1];
    if (a.pool[l] == 2) conv_layer<2>(in, out, a.cw[l], a.cb[l], a.c[l], a.h[l], a.w[l], a.c[l + 1], a.k[l], a.cs[l], a.h[l + 1], a.w[l + 1]);
    else conv_layer<1>(in, out, a.cw[l], a.cb[l], a.c[l], a.h[l], a.w[l], a.c[l + 1], a.k[l], a.cs[l], a.h[l + 1], a.w[l + 1]);
    __syncthreads();
  }
  head_layer(a, lds + boff[a.nconv & 1], row0);
}

// ---- host: the geometry of a conv stack -----------------------------------------------------------------------------------------------
struct Geometry {
  int c[MAXC + 1], h[MAXC + 1], w[MAXC + 1], cs[MAXC], pool[MAXC], flat, buf_floats[2], enc_bytes;
};

// The conv-stack fields of a descriptor (lt_student_desc, lt_cnn_desc: the same names): nullptr if the kernels serve them, else the
// refusal, which names the field.
template <class Desc>
const char* geometry_of(const Desc* d, Geometry* L) {
  if (d->conv_norm != 0) return "conv_norm must be 0 (norm layers are not served)";
  if (d->num_convs < 1 || d->num_convs > MAXC) return "num_convs must be in [1, LT_STUDENT_MAX_CONVS]";
  if (d->conv_activation != LT_ACT_RELU) return "conv_activation must be LT_ACT_RELU";
  if (d->img_channels < 1 || d->img_height < 1 || d->img_width < 1 || d->img_channels > 64 || d->img_height > 256 || d->img_width > 256)
    return "img_channels / img_height / img_width must be positive (at most 64 x 256 x 256)";
  L->c[0] = d->img_channels; L->h[0] = d->img_height; L->w[0] = d->img_width;
  for (int l = 0; l < d->num_convs; ++l) {
    if (d->conv_padding[l] != 0) return "conv_padding must be 0";
    if (d->conv_channels[l] < 1 || d->conv_channels[l] > 256) return "conv_channels must be in [1, 256]";
    if (d->conv_kernel[l] < 1 || d->conv_kernel[l] > 16) return "conv_kernel must be in [1, 16]";
    if (d->conv_stride[l] < 1 || d->conv_stride[l] > 16) return "conv_stride must be in [1, 16]";
    if (d->use_maxpool && d->conv_stride[l] > 2) return "conv_stride above 2 with use_maxpool (a pool larger than 2 x 2 is not served)";
    L->cs[l] = d->use_maxpool ? 1 : d->conv_stride[l];
    L->pool[l] = d->use_maxpool ? d->conv_stride[l] : 1;
    const int hc = (L->h[l] - d->conv_kernel[l]) / L->cs[l] + 1, wc = (L->w[l] - d->conv_kernel[l]) / L->cs[l] + 1;
    if (L->h[l] < d->conv_kernel[l] || L->w[l] < d->conv_kernel[l] || hc / L->pool[l] < 1 || wc / L->pool[l] < 1)
      return "conv_kernel / conv_stride leave no output for the image (img_height, img_width)";
    L->c[l + 1] = d->conv_channels[l]; L->h[l + 1] = hc / L->pool[l]; L->w[l + 1] = wc / L->pool[l];
  }
  L->buf_floats[0] = L->buf_floats[1] = 0;
  for (int l = 0; l <= d->num_convs; ++l) {
    const int sz = pad4(L->c[l] * L->h[l] * L->w[l]);
    if (sz > L->buf_floats[l & 1]) L->buf_floats[l & 1] = sz;
  }
  L->flat = L->c[d->num_convs] * L->h[d->num_convs] * L->w[d->num_convs];
  L->enc_bytes = ET * (L->buf_floats[0] + L->buf_floats[1]) * (int)sizeof(float);
  if (L->enc_bytes > MAX_LDS) return "img_height / img_width / conv_channels: the maps of 8 envs do not fit in LDS";
  if (d->head_out < 16 || d->head_out > 256 || d->head_out % 16) return "head_out must be a multiple of 16 in [16, 256]";
  return nullptr;
}

// The encoder's arguments but for the pointers (tactile, tstride, n, emb, cw, cb, hw, hb)
template <class Desc>
void fill_enc_args(const Desc* desc, const Geometry& L, EncArgs* e) {
  e->nconv = desc->num_convs; e->flat = L.flat; e->D = desc->head_out; e->buf_floats[0] = L.buf_floats[0]; e->buf_floats[1] = L.buf_floats[1];
  for (int l = 0; l <= MAXC; ++l) { e->c[l] = L.c[l <= desc->num_convs ? l : 0]; e->h[l] = L.h[l <= desc->num_convs ? l : 0]; e->w[l] = L.w[l <= desc->num_convs ? l : 0]; }
  for (int l = 0; l < MAXC; ++l) {
    const bool on = l < desc->num_convs;
    e->k[l] = on ? desc->conv_kernel[l] : 1; e->cs[l] = on ? L.cs[l] : 1; e->pool[l] = on ? L.pool[l] : 1;
  }
}

}  // namespace lt_cnn
