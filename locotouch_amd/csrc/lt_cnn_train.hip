// lt_cnn_train.hip - the training form of the student's tactile CNN head (include/lt_cnn_train.h).
//
// The eager form (`Conv2dAsGemm`) applies each convolution as a dense GEMM against the layer's response to the identity basis: 14 x the
// FLOPs, and autograd keeps every map of every image (~0.95 GB at 50 000 images).  Here:
//   forward   pack (1 launch) + lt_cnn_forward_kernel: the encoder of lt_student_step (lt_cnn_device.h, the same source, hence the same
//             bits per row) over all n images, a workgroup per tile of 8.
//   backward  pack + lt_cnn_backward_kernel + lt_cnn_reduce_kernel.  A workgroup of 512 threads owns a SLAB of consecutive tiles (the
//             partition is a function of n alone: at most LT_CNN_MAX_SLABS = 256 workgroups, one per CU - the tile's maps take ~106 KB of
//             the 160 KB of LDS, so a CU holds one workgroup anyway, at two waves per SIMD).  Per tile it recomputes the maps in LDS
//             (every map stays: it is the next layer's input and its own ReLU mask; the 2 x 2 pool also leaves a 2-bit argmax per pooled
//             element), carries d_emb back through the head and the convolutions, and adds the tile's weight gradients to the
//             workgroup's PRIVATE partial in the scratch (plain read-modify-write by the one thread that owns the element: L2-resident,
//             ~0.5 % of the tile's instructions).  The second launch adds the partials in workgroup order.  No atomics; every sum has
//             one order.
//   weight gradient  dW[oc][j] = sum over (image, position) of dz[oc][p] * in[j at p] on the VALU: a thread owns a 6 x 4 block of
//             (oc, j) in registers and walks the tile's positions - 10 LDS reads per 24 fmaf - and, where a layer has fewer blocks than
//             threads, 2 / 4 / 8 neighbouring lanes split the tile's images and add up by a fixed shuffle tree.  Behind a pool only the
//             argmax position of each window carries gradient, so conv 1 sums over 35 pooled positions, not 140.  The Linear head is
//             the same routine (a 1 x 1 convolution on a flat x 1 x 1 map).  The f32 MFMA (v_mfma_f32_16x16x4_f32) has the VALU's peak
//             rate on this part; it would save LDS reads, but its operand tiles (im2col patches, and per-oc argmax gathers for conv 1)
//             would have to be built in LDS first - the judgement of lt_student.hip's encoder, which holds here too.
//   input gradient   a "full" convolution of dz with the flipped weights in the forward's form: a lane owns one (image, input position),
//             a wave six input channels, so the weights are wave-uniform (scalar loads; the pack writes an [oc][k][k][ic] copy for it).
#include <hip/hip_runtime.h>

#include "../../include/lt_cnn_train.h"
#include "lt_cnn_device.h"
#include "lt_host_check.h"

static_assert(LT_CNN_MAX_CONVS == LT_STUDENT_MAX_CONVS && LT_CNN_TILE == LT_STUDENT_ENV_TILE, "lt_cnn_train.h mirrors lt_student.h");

namespace {

using namespace lt_cnn;

constexpr int BT = 512;   // threads of the backward workgroup
constexpr int WR = 6;     // weight-gradient register block: output channels
constexpr int WS = 4;     //                                 x weight positions j = (ic, ky, kx)
constexpr int NL = MAXC + 1;  // "layers" of the backward: the convolutions and the head

// ---- forward -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void lt_cnn_forward_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  encoder_tile(a, lds);
}

// ---- pack ----------------------------------------------------------------------------------------------------------------------------
// fwd[j][oc] = src[oc][j] (j < J = Cin K K); bwd[oc][kk][ic] = src[oc][ic][kk] (bwd may be null)
struct PackSeg {
  const float* src;
  float *fwd, *bwd;
  int Cout, Cin, KK;
};
struct PackArgs {
  int nseg;
  PackSeg seg[NL];
};

__global__ __launch_bounds__(TPB) void lt_cnn_pack_kernel(const PackArgs a) {
  const PackSeg& s = a.seg[blockIdx.y];
  const int J = s.Cin * s.KK, total = s.Cout * J;
  for (int idx = blockIdx.x * TPB + threadIdx.x; idx < total; idx += gridDim.x * TPB) {
    const int oc = idx / J, j = idx - oc * J, ic = j / s.KK, kk = j - ic * s.KK;
    const float v = s.src[idx];
    s.fwd[j * s.Cout + oc] = v;
    if (s.bwd) s.bwd[(oc * s.KK + kk) * s.Cin + ic] = v;
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
  const float *x, *demb;
  long long n;
  int tiles, tiles_per_slab;
  EncArgs enc;                // geometry and the packed forward weights (tactile, tstride, n, emb unused)
  const float* wb[MAXC];      // [oc][k][k][ic] copies of conv 1 .. (null for conv 0: it has no input gradient)
  float* partial;             // [slabs][part_floats]
  int part_floats, pw[NL], pb[NL];  // offsets of a layer's weight / bias gradient inside a partial (layer nconv: the head)
  int map_off[NL], g_off[2], demb_off, arg_off[MAXC];  // LDS offsets in floats
  int split[NL];              // lanes that share a weight-gradient block (a power of two, <= ET)
};

// part_w[oc][j] (+)= sum_{e, p} dz[e][oc][p] * in[e][j at the conv position p stands for]; part_b[oc] (+)= sum dz[e][oc][p]
template <int P>
__device__ void wgrad_layer(const float* in, const float* dz, const unsigned char* arg, float* part_w, float* part_b, bool first, int Cin, int H,
                            int W, int Cout, int K, int cs, int Ho, int Wo, int IS) {
  const int J = Cin * K * K, njg = (J + WS - 1) / WS, nocg = (Cout + WR - 1) / WR, nitems = njg * nocg;
  const int npos = Ho * Wo, in_sz = Cin * H * W, out_sz = Cout * npos;
  const int ih = threadIdx.x & (IS - 1);
  for (int item = threadIdx.x / IS; item < nitems; item += BT / IS) {
    const int jg = item % njg, oc0 = (item / njg) * WR;
    int joff[WS], ocr[WR];
#pragma unroll
    for (int s = 0; s < WS; ++s) {
      const int j = min(jg * WS + s, J - 1), ic = j / (K * K), r = j - ic * K * K, ky = r / K;
      joff[s] = (ic * H + ky) * W + (r - ky * K);
    }
#pragma unroll
    for (int r = 0; r < WR; ++r) ocr[r] = min(oc0 + r, Cout - 1) * npos;
    float acc[WR][WS], bacc[WR];
#pragma unroll
    for (int r = 0; r < WR; ++r) {
      bacc[r] = 0.f;
#pragma unroll
      for (int s = 0; s < WS; ++s) acc[r][s] = 0.f;
    }
    for (int e = ih; e < ET; e += IS) {
      const float* dze = dz + e * out_sz;
      for (int y = 0; y < Ho; ++y) {
        for (int x = 0; x < Wo; ++x) {
          const int p = y * Wo + x;
          const float* base = in + e * in_sz + (y * P * cs) * W + x * P * cs;
          float dzv[WR];
#pragma unroll
          for (int r = 0; r < WR; ++r) dzv[r] = dze[ocr[r] + p];
          if constexpr (P == 1) {
            float iv[WS];
#pragma unroll
            for (int s = 0; s < WS; ++s) iv[s] = base[joff[s]];
#pragma unroll
            for (int r = 0; r < WR; ++r)
#pragma unroll
              for (int s = 0; s < WS; ++s) acc[r][s] = fmaf(dzv[r], iv[s], acc[r][s]);
          } else {
#pragma unroll
            for (int r = 0; r < WR; ++r) {
              const int c = arg[e * out_sz + ocr[r] + p];  // the window's first maximum: dy = c / P, dx = c % P
              const float* bp = base + ((c / P) * W + (c % P)) * cs;
#pragma unroll
              for (int s = 0; s < WS; ++s) acc[r][s] = fmaf(dzv[r], bp[joff[s]], acc[r][s]);
            }
          }
#pragma unroll
          for (int r = 0; r < WR; ++r) bacc[r] += dzv[r];
        }
      }
    }
    for (int m = 1; m < IS; m <<= 1) {  // the IS lanes of the block: one fixed tree
#pragma unroll
      for (int r = 0; r < WR; ++r) {
        bacc[r] += __shfl_xor(bacc[r], m);
#pragma unroll
        for (int s = 0; s < WS; ++s) acc[r][s] += __shfl_xor(acc[r][s], m);
      }
    }
    if (ih == 0) {
#pragma unroll
      for (int r = 0; r < WR; ++r) {
        if (oc0 + r >= Cout) break;
#pragma unroll
        for (int s = 0; s < WS; ++s) {
          const int j = jg * WS + s;
          if (j < J) {
            float* q = part_w + (oc0 + r) * J + j;
            *q = first ? acc[r][s] : *q + acc[r][s];
          }
        }
        if (jg == 0) part_b[oc0 + r] = first ? bacc[r] : part_b[oc0 + r] + bacc[r];
      }
    }
  }
}

// g_in[e][ic][iy][ix] = (a_in > 0) * sum_{oc, ky, kx} dz[e][oc][the output (iy - ky, ix - kx) feeds] * w[oc][ic][ky][kx]
template <int P, bool UNIT>  // UNIT: the convolution runs at stride 1
__device__ void dgrad_layer(const float* dz, const unsigned char* arg, const float* __restrict__ wb, const float* a_in, float* g_in, int Cin, int H,
                            int W, int Cout, int K, int cs, int Ho, int Wo) {
  const int lane = threadIdx.x & 63, wave = lt::wave_uniform(threadIdx.x >> 6);
  const int hw = H * W, items = ET * hw, chunks = (items + 63) / 64, groups = (Cin + OCB - 1) / OCB, npos = Ho * Wo;
  for (int t = wave; t < groups * chunks; t += BT / 64) {
    const int ic0 = (t % groups) * OCB, it_raw = (t / groups) * 64 + lane;
    const int it = it_raw < items ? it_raw : items - 1;
    const int e = it / hw, q = it - e * hw, iy = q / W, ix = q - iy * W;
    const float* dze = dz + e * Cout * npos;
    float acc[OCB];
#pragma unroll
    for (int o = 0; o < OCB; ++o) acc[o] = 0.f;
    for (int ky = 0; ky < K; ++ky) {
      for (int kx = 0; kx < K; ++kx) {
        int cy = iy - ky, cx = ix - kx;
        bool ok = cy >= 0 && cx >= 0;
        if constexpr (!UNIT) {
          ok = ok && cy % cs == 0 && cx % cs == 0;
          cy /= cs; cx /= cs;
        }
        const int code = (cy % P) * P + (cx % P), py = cy / P, px = cx / P;
        ok = ok && py < Ho && px < Wo;
        const int p = ok ? py * Wo + px : 0;
        for (int oc = 0; oc < Cout; ++oc) {
          float v = dze[oc * npos + p];
          if constexpr (P > 1) v = arg[(e * Cout + oc) * npos + p] == code ? v : 0.f;
          v = ok ? v : 0.f;
          const float* wp = wb + ((oc * K + ky) * K + kx) * Cin + ic0;
#pragma unroll
          for (int o = 0; o < OCB; ++o) acc[o] = fmaf(ic0 + o < Cin ? wp[o] : 0.f, v, acc[o]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < OCB; ++o) {
      if (ic0 + o >= Cin || it_raw >= items) break;
      const int at = (e * Cin + ic0 + o) * hw + q;
      g_in[at] = a_in[at] > 0.f ? acc[o] : 0.f;
    }
  }
}

__global__ __launch_bounds__(BT) void lt_cnn_backward_kernel(const BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const EncArgs& g = a.enc;
  const int tid = threadIdx.x, nc = g.nconv, D = g.D, flat = g.flat, img = g.c[0] * g.h[0] * g.w[0];
  float* part = a.partial + (long long)blockIdx.x * a.part_floats;
  float* demb = lds + a.demb_off;
  const int t0 = blockIdx.x * a.tiles_per_slab, t1 = min(t0 + a.tiles_per_slab, a.tiles);
  for (int tile = t0; tile < t1; ++tile) {
    const long long row0 = (long long)tile * ET;
    const bool first = tile == t0;
    __syncthreads();  // the previous tile's readers are done
    for (int i = tid; i < ET * img; i += BT) {
      const int e = i / img;
      lds[a.map_off[0] + i] = row0 + e < a.n ? a.x[row0 * img + i] : 0.f;  // a tail image: zeros, and a zero d_emb row
    }
    for (int i = tid; i < ET * D; i += BT) demb[i] = row0 + i / D < a.n ? a.demb[row0 * D + i] : 0.f;
    __syncthreads();
    for (int l = 0; l < nc; ++l) {
      const float* in = lds + a.map_off[l];
      float* out = lds + a.map_off[l + 1];
      if (g.pool[l] == 2)
        conv_layer<2, BT, true>(in, out, g.cw[l], g.cb[l], g.c[l], g.h[l], g.w[l], g.c[l + 1], g.k[l], g.cs[l], g.h[l + 1], g.w[l + 1],
                                (unsigned char*)(lds + a.arg_off[l]));
      else conv_layer<1, BT>(in, out, g.cw[l], g.cb[l], g.c[l], g.h[l], g.w[l], g.c[l + 1], g.k[l], g.cs[l], g.h[l + 1], g.w[l + 1]);
      __syncthreads();
    }
    // the head: a 1 x 1 convolution on the flat x 1 x 1 map, dz = d_emb
    const float* top = lds + a.map_off[nc];
    wgrad_layer<1>(top, demb, nullptr, part + a.pw[nc], part + a.pb[nc], first, flat, 1, 1, D, 1, 1, 1, 1, a.split[nc]);
    float* gtop = lds + a.g_off[nc & 1];
    for (int it = tid; it < ET * flat; it += BT) {
      const int e = it / flat, k = it - e * flat;
      const lt::f32x4* wp = (const lt::f32x4*)(g.hw + (long long)k * D);  // packed head [flat][D], D % 16 == 0
      const lt::f32x4* dp = (const lt::f32x4*)(demb + e * D);
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      for (int o = 0; o < D / 4; ++o) {
        const lt::f32x4 w = wp[o], d = dp[o];
        s0 = fmaf(w[0], d[0], s0); s1 = fmaf(w[1], d[1], s1); s2 = fmaf(w[2], d[2], s2); s3 = fmaf(w[3], d[3], s3);
      }
      gtop[it] = top[it] > 0.f ? (s0 + s1) + (s2 + s3) : 0.f;
    }
    __syncthreads();
    for (int l = nc - 1; l >= 0; --l) {
      const float* in = lds + a.map_off[l];
      const float* dz = lds + a.g_off[(l + 1) & 1];
      const unsigned char* arg = (const unsigned char*)(lds + a.arg_off[l]);
      const bool pooled = g.pool[l] == 2;
      if (pooled) wgrad_layer<2>(in, dz, arg, part + a.pw[l], part + a.pb[l], first, g.c[l], g.h[l], g.w[l], g.c[l + 1], g.k[l], g.cs[l], g.h[l + 1], g.w[l + 1], a.split[l]);
      else wgrad_layer<1>(in, dz, arg, part + a.pw[l], part + a.pb[l], first, g.c[l], g.h[l], g.w[l], g.c[l + 1], g.k[l], g.cs[l], g.h[l + 1], g.w[l + 1], a.split[l]);
      if (l > 0) {
        float* gin = lds + a.g_off[l & 1];
        if (pooled) dgrad_layer<2, true>(dz, arg, a.wb[l], in, gin, g.c[l], g.h[l], g.w[l], g.c[l + 1], g.k[l], g.cs[l], g.h[l + 1], g.w[l + 1]);
        else if (g.cs[l] == 1) dgrad_layer<1, true>(dz, arg, a.wb[l], in, gin, g.c[l], g.h[l], g.w[l], g.c[l + 1], g.k[l], g.cs[l], g.h[l + 1], g.w[l + 1]);
        else dgrad_layer<1, false>(dz, arg, a.wb[l], in, gin, g.c[l], g.h[l], g.w[l], g.c[l + 1], g.k[l], g.cs[l], g.h[l + 1], g.w[l + 1]);
        __syncthreads();
      }
    }
  }
}

// out[i] = partial[0][i] + partial[1][i] + ... in workgroup order, scattered to the gradient tensors
struct ReduceArgs {
  const float* partial;
  int slabs, part_floats, nseg, begin[2 * NL], count[2 * NL];
  float* dst[2 * NL];
};

__global__ __launch_bounds__(TPB) void lt_cnn_reduce_kernel(const ReduceArgs a) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= a.part_floats) return;
  int s = 0;
  while (s < a.nseg && !(i >= a.begin[s] && i < a.begin[s] + a.count[s])) ++s;
  if (s == a.nseg) return;  // padding between two segments
  float sum = a.partial[i];
  for (int b = 1; b < a.slabs; ++b) sum += a.partial[(long long)b * a.part_floats + i];
  a.dst[s][i - a.begin[s]] = sum;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct Plan : Geometry {
  size_t fw[NL], bw[MAXC], packed;  // ws offsets: forward copies (layer nconv: the head), [oc][kk][ic] copies, their total
  int pw[NL], pb[NL], part_floats;
  int map_off[NL], g_off[2], demb_off, arg_off[MAXC], bwd_bytes, split[NL];
};

int plan_of(const lt_cnn_desc* d, Plan* L) {
  if (!d) return refuse("lt_cnn_desc", "desc is NULL");
  if (const char* why = geometry_of(d, L)) return refuse("lt_cnn_desc", why);
  const int nc = d->num_convs, D = d->head_out;
  size_t off = 0;
  auto take = [&](size_t floats) { const size_t at = off; off += (floats + 3) & ~(size_t)3; return at; };
  int poff = 0;
  auto ptake = [&](int floats) { const int at = poff; poff += pad4(floats); return at; };
  for (int l = 0; l <= nc; ++l) {
    const int cin = l < nc ? L->c[l] : L->flat, cout = l < nc ? L->c[l + 1] : D, kk = l < nc ? d->conv_kernel[l] * d->conv_kernel[l] : 1;
    L->fw[l] = take((size_t)cin * kk * cout);
    L->pw[l] = ptake(cin * kk * cout);
    L->pb[l] = ptake(cout);
    int items = ((cin * kk + WS - 1) / WS) * ((cout + WR - 1) / WR), split = 1;
    while (split < ET && items * split * 2 <= BT) split *= 2;
    L->split[l] = split;
  }
  for (int l = 1; l < nc; ++l) L->bw[l] = take((size_t)L->c[l] * d->conv_kernel[l] * d->conv_kernel[l] * L->c[l + 1]);
  L->packed = off;
  L->part_floats = poff;
  // LDS of the backward: every map, two gradient buffers (maps of equal parity share one), d_emb, the argmax bytes of the pooled layers
  int lds = 0, gsz[2] = {0, 0};
  for (int l = 0; l <= nc; ++l) {
    const int sz = L->c[l] * L->h[l] * L->w[l];
    L->map_off[l] = lds;
    lds += pad4(ET * sz);
    if (l > 0 && ET * sz > gsz[l & 1]) gsz[l & 1] = ET * sz;
  }
  for (int b = 0; b < 2; ++b) { L->g_off[b] = lds; lds += pad4(gsz[b]); }
  L->demb_off = lds;
  lds += ET * D;
  for (int l = 0; l < nc; ++l) {
    L->arg_off[l] = lds;
    if (L->pool[l] == 2) lds += pad4(ET * L->c[l + 1] * L->h[l + 1] * L->w[l + 1]) / 4;
  }
  L->bwd_bytes = lds * (int)sizeof(float);
  if (L->bwd_bytes > MAX_LDS) return refuse("lt_cnn_desc", "img_height / img_width / conv_channels: the maps and gradient maps of 8 images do not fit in LDS");
  return LT_OK;
}

int slabs_of(int64_t n, int* tiles_per_slab, int* tiles) {
  const int64_t t = (n + ET - 1) / ET, per = (t + LT_CNN_MAX_SLABS - 1) / LT_CNN_MAX_SLABS;
  *tiles = (int)t;
  *tiles_per_slab = (int)per;
  return (int)((t + per - 1) / per);
}

bool complete(const lt_cnn_desc* d, const float* const* w, const float* const* b, const float* hw, const float* hb) {
  for (int l = 0; l < d->num_convs; ++l)
    if (!w[l] || !b[l]) return false;
  return hw && hb;
}

// the pack launch and the encoder's arguments over the packed copies; `backward`: also the [oc][k][k][ic] copies of the input gradient
int pack(const lt_cnn_desc* d, const Plan& L, const lt_cnn_params* p, float* ws, bool backward, hipStream_t stream, EncArgs* e) {
  const int nc = d->num_convs;
  PackArgs a;
  a.nseg = nc + 1;
  int most = 0;
  for (int l = 0; l <= nc; ++l) {
    const bool conv = l < nc;
    a.seg[l] = PackSeg{conv ? p->conv_w[l] : p->head_w, ws + L.fw[l], backward && conv && l > 0 ? ws + L.bw[l] : nullptr, conv ? L.c[l + 1] : d->head_out,
                       conv ? L.c[l] : L.flat, conv ? d->conv_kernel[l] * d->conv_kernel[l] : 1};
    const int total = a.seg[l].Cout * a.seg[l].Cin * a.seg[l].KK;
    if (total > most) most = total;
  }
  fill_enc_args(d, L, e);
  for (int l = 0; l < MAXC; ++l) {
    e->cw[l] = l < nc ? ws + L.fw[l] : nullptr;
    e->cb[l] = l < nc ? p->conv_b[l] : nullptr;
  }
  e->hw = ws + L.fw[nc]; e->hb = p->head_b;
  const int blocks = (most + TPB - 1) / TPB;
  hipLaunchKernelGGL(lt_cnn_pack_kernel, dim3((unsigned)(blocks < 64 ? blocks : 64), (unsigned)a.nseg), dim3(TPB), 0, stream, a);
  return launch_status("lt_cnn_pack");
}

}  // namespace

extern "C" {

int lt_cnn_validate(const lt_cnn_desc* desc) {
  Plan L;
  return plan_of(desc, &L);
}

int lt_cnn_ws_floats(const lt_cnn_desc* desc, int64_t n, size_t* floats) {
  Plan L;
  if (const int rc = plan_of(desc, &L)) return rc;
  if (!floats || n < 1 || n > INT32_MAX) return einval("lt_cnn_ws_floats: floats non-null and n in [1, 2^31)");
  int per, tiles;
  *floats = L.packed + (size_t)slabs_of(n, &per, &tiles) * (size_t)L.part_floats;
  return LT_OK;
}

int lt_cnn_launches(const lt_cnn_desc* desc, int64_t n, int backward) {
  Plan L;
  if (const int rc = plan_of(desc, &L)) return rc;
  if (n < 1 || n > INT32_MAX) return einval("lt_cnn_launches: n must be in [1, 2^31)");
  return backward ? 3 : 2;
}

int lt_cnn_forward(const lt_cnn_desc* desc, const lt_cnn_params* p, const float* x, int64_t n, float* emb_out, float* ws, void* stream) {
  Plan L;
  if (const int rc = plan_of(desc, &L)) return rc;
  if (!p || !x || !emb_out || !ws || (uintptr_t)ws % 16 || n < 1 || n > INT32_MAX || !complete(desc, p->conv_w, p->conv_b, p->head_w, p->head_b))
    return einval("lt_cnn_forward: params (every pointer the descriptor needs), x, emb_out and a 16-byte aligned ws non-null; n in [1, 2^31)");
  EncArgs e;
  if (const int rc = pack(desc, L, p, ws, false, (hipStream_t)stream, &e)) return rc;
  e.tactile = x; e.tstride = L.c[0] * L.h[0] * L.w[0]; e.n = n; e.emb = emb_out;
  if (L.enc_bytes > 64 * 1024)
    if (const int err = lt_ensure_dynamic_lds((const void*)lt_cnn_forward_kernel, MAX_LDS)) { lt_set_error(lt_hip_error_string(err)); return LT_EHIP; }
  hipLaunchKernelGGL(lt_cnn_forward_kernel, dim3((unsigned)((n + ET - 1) / ET)), dim3(TPB), (size_t)L.enc_bytes, (hipStream_t)stream, e);
  return launch_status("lt_cnn_forward");
}

int lt_cnn_backward(const lt_cnn_desc* desc, const lt_cnn_params* p, const float* x, const float* d_emb, int64_t n, const lt_cnn_grads* grads,
                    float* ws, void* stream) {
  Plan L;
  if (const int rc = plan_of(desc, &L)) return rc;
  if (!p || !x || !d_emb || !grads || !ws || (uintptr_t)ws % 16 || n < 1 || n > INT32_MAX ||
      !complete(desc, p->conv_w, p->conv_b, p->head_w, p->head_b) || !complete(desc, grads->conv_w, grads->conv_b, grads->head_w, grads->head_b))
    return einval("lt_cnn_backward: params and grads_out (every pointer the descriptor needs), x, d_emb and a 16-byte aligned ws non-null; "
                  "n in [1, 2^31)");
  const int nc = desc->num_convs;
  BwdArgs b;
  if (const int rc = pack(desc, L, p, ws, true, (hipStream_t)stream, &b.enc)) return rc;
  b.enc.tactile = nullptr; b.enc.tstride = 0; b.enc.n = n; b.enc.emb = nullptr;
  b.x = x; b.demb = d_emb; b.n = n;
  const int slabs = slabs_of(n, &b.tiles_per_slab, &b.tiles);
  b.partial = ws + L.packed; b.part_floats = L.part_floats;
  b.g_off[0] = L.g_off[0]; b.g_off[1] = L.g_off[1]; b.demb_off = L.demb_off;
  ReduceArgs r;
  r.partial = b.partial; r.slabs = slabs; r.part_floats = L.part_floats; r.nseg = 0;
  for (int l = 0; l < NL; ++l) {
    const bool on = l <= nc;
    b.pw[l] = on ? L.pw[l] : 0; b.pb[l] = on ? L.pb[l] : 0; b.map_off[l] = on ? L.map_off[l] : 0; b.split[l] = on ? L.split[l] : 1;
    if (l < MAXC) { b.wb[l] = l > 0 && l < nc ? ws + L.bw[l] : nullptr; b.arg_off[l] = l < nc ? L.arg_off[l] : 0; }
    if (!on) continue;
    const int cin = l < nc ? L.c[l] : L.flat, cout = l < nc ? L.c[l + 1] : desc->head_out, kk = l < nc ? desc->conv_kernel[l] * desc->conv_kernel[l] : 1;
    r.begin[r.nseg] = L.pw[l]; r.count[r.nseg] = cin * kk * cout; r.dst[r.nseg++] = l < nc ? grads->conv_w[l] : grads->head_w;
    r.begin[r.nseg] = L.pb[l]; r.count[r.nseg] = cout; r.dst[r.nseg++] = l < nc ? grads->conv_b[l] : grads->head_b;
  }
  for (int s = r.nseg; s < 2 * NL; ++s) { r.begin[s] = r.count[s] = 0; r.dst[s] = nullptr; }
  if (L.bwd_bytes > 64 * 1024)
    if (const int err = lt_ensure_dynamic_lds((const void*)lt_cnn_backward_kernel, MAX_LDS)) { lt_set_error(lt_hip_error_string(err)); return LT_EHIP; }
  hipLaunchKernelGGL(lt_cnn_backward_kernel, dim3((unsigned)slabs), dim3(BT), (size_t)L.bwd_bytes, (hipStream_t)stream, b);
  hipLaunchKernelGGL(lt_cnn_reduce_kernel, dim3((unsigned)((L.part_floats + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, r);
  return launch_status("lt_cnn_backward");
}

}  // extern "C"
