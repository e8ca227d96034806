// One rollout step of the two LSTM memories of a recurrent policy in one launch (include/lt_memory.h).
//
// Shape: B = num_envs rows (4096 and up), K = I + H (observation width + hidden size), 4H gate rows, two networks.  lt_lstm.hip's step
// kernel is laid out for the update (B ~ 47: a 16 x 16 tile per workgroup, weights streamed once per tile); at the rollout's shape that
// re-reads all of W_hh once per 16 rows and leaves the input GEMM to a library call.  Here a workgroup owns UT hidden units (4 UT gate
// rows of [W_ih | W_hh]) and a ROW BLOCK of RB rows:
//   1. the weight panel [4 UT][I + H] is staged into LDS ONCE (UT = 16: 64 gate rows, up to 160 KiB; UT = 8 when that does not fit);
//   2. the four waves walk the row block in 16-row sub-tiles (wave w takes sub-tiles w, w + 4, ...): the B operand (x_t | h rows) comes
//      straight from global memory, one 16-byte load per lane and 16-wide k block, double-buffered in groups of four blocks; the A
//      operand is one ds_read_b128 per M tile and k block; 4 UT / 16 MFMA tiles share each B load;
//   3. the gate arithmetic is the epilogue, in registers: the M index of a tile is 4 * g + gate, so lane (n, g) of the D layout holds the
//      four gates of ONE unit of row n - no LDS round trip, no second launch.
// grid (H / UT, ceil(N / RB), 2 networks), block 256.  RB is chosen on the host so that the grid covers the chip once.
//
// The reset mask (`PolicyMemory.reset(dones)`) is applied WHERE THE OPERAND IS LOADED: h and c of the previous step are read as
// where(done, 0, .) by every workgroup that needs them and the buffers themselves are never rewritten, so no workgroup reads what another
// writes in the same launch.  The new raw state goes to the other ping-pong buffer.  The workgroups of unit tile 0 also copy the masked
// pre-step state of their row block into the storage slot (`saved_hidden_states`).
//
// Arithmetic: v_mfma_f32_16x16x4_f32, exact f32 products, f32 accumulation, k blocks in index order (x side first, then h) dealt to four
// partial sums that are added pairwise: one fixed order, no atomics.  Operand trick as lt_lstm.hip: MFMA step s of a 16-wide k block consumes the k-set {kb + 4 q + s}, so lane (i, q)
// supplies component s of ONE 16-byte load.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "lt_env.h"
#include "lt_internal.h"
#include "lt_memory.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { const float e = __expf(-2.f * fabsf(x)); const float t = (1.f - e) / (1.f + e); return x < 0.f ? -t : t; }

struct NetArgs {
  const float* x; const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; const float* h_in; const float* c_in;
  float* h_out; float* c_out; float* saved_h; float* saved_c;
  int I, IP, KP;  // IP: I rounded up to 16 (the x side's k blocks; the panel holds zeros in [I, IP)); KP: LDS row stride in floats
};
struct StepArgs { NetArgs net[2]; const uint8_t* dones; int N, H, RB; };

constexpr int kLdsBytes = 160 * 1024;

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// LDS row stride: IP + H + 8 is an odd multiple of 8 floats (IP, H multiples of 16): the 16 lanes of a ds_read_b128 lane group (rows
// {0-3, 12-15} at one q, rows 4-11 at the next) then start at 16 distinct multiples of 4 banks
__host__ __device__ inline int panel_stride(int I, int H) { return round_up(I, 16) + H + 8; }

// The B operand of k block `blk` for lane (row, q): x[row][16 blk + 4 q .. + 3] (zeros past I; rows are only 4-byte aligned unless
// `xvec`), or behind the x side's blocks where(done, 0, h[row][...]).
__device__ __forceinline__ f32x4 load_b(const float* __restrict__ xrow, const float* __restrict__ hrow, int blk, int q, int I, int xblks, bool xvec,
                                        bool done) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (blk < xblks) {
    const int k = 16 * blk + 4 * q;
    if (xvec && k + 3 < I) {
      v = *(const f32x4*)(xrow + k);
    } else {
      if (k < I) v[0] = xrow[k];
      if (k + 1 < I) v[1] = xrow[k + 1];
      if (k + 2 < I) v[2] = xrow[k + 2];
      if (k + 3 < I) v[3] = xrow[k + 3];
    }
  } else if (!done) {
    v = *(const f32x4*)(hrow + 16 * (blk - xblks) + 4 * q);
  }
  return v;
}

// MT consecutive floats as ONE access (MT = 4: 16 bytes, MT = 2: 8 bytes; the offsets are multiples of MT floats from 16-byte aligned rows)
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int MT> __device__ __forceinline__ void load_units(const float* __restrict__ src, float* dst) {
  if constexpr (MT == 4) { const f32x4 v = *(const f32x4*)src; dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3]; }
  else { const f32x2 v = *(const f32x2*)src; dst[0] = v[0]; dst[1] = v[1]; }
}
template <int MT> __device__ __forceinline__ void store_units(float* __restrict__ dst, const float* src) {
  if constexpr (MT == 4) *(f32x4*)dst = (f32x4){src[0], src[1], src[2], src[3]};
  else *(f32x2*)dst = (f32x2){src[0], src[1]};
}

template <int UT>  // hidden units per workgroup: 16 or 8
__global__ __launch_bounds__(256) void lt_memory_step_kernel(const StepArgs a) {
  constexpr int MT = UT / 4;  // 16-row MFMA tiles of the panel; lane (n, g) of the D layout owns units g * MT .. + MT - 1 of its row
  extern __shared__ __attribute__((aligned(16))) float panel[];  // [4 UT][KP]
  const NetArgs& p = a.net[blockIdx.z];
  const int N = a.N, H = a.H, I = p.I, IP = p.IP, KP = p.KP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * UT;
  const int r0 = blockIdx.y * a.RB;
  const int r1 = min(N, r0 + a.RB);

  // ---- 1. the weight panel, once.  Panel row pr = 16 mt + 4 g + v holds gate v of unit j0 + g * MT + mt: [W_ih row | 0 | W_hh row]
  for (int idx = tid; idx < 4 * UT * IP; idx += 256) {
    const int pr = idx / IP, k = idx - pr * IP;
    const int unit = j0 + ((pr >> 2) & 3) * MT + (pr >> 4), wrow = (pr & 3) * H + unit;
    panel[pr * KP + k] = k < I ? p.w_ih[(long long)wrow * I + k] : 0.f;
  }
  const int h4 = H / 4;
  for (int idx = tid; idx < 4 * UT * h4; idx += 256) {
    const int pr = idx / h4, k4 = idx - pr * h4;
    const int unit = j0 + ((pr >> 2) & 3) * MT + (pr >> 4), wrow = (pr & 3) * H + unit;
    *(f32x4*)(panel + pr * KP + IP + 4 * k4) = *(const f32x4*)(p.w_hh + (long long)wrow * H + 4 * k4);
  }

  // ---- the masked pre-step state of this row block -> the storage slot (unit tile 0 alone; every element of the slot's rows)
  if (blockIdx.x == 0) {
    for (int idx = tid; idx < (r1 - r0) * h4; idx += 256) {
      const int r = r0 + idx / h4;
      const long long o = (long long)r * H + 4 * (idx % h4);
      const bool done = a.dones && a.dones[r] != 0;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(p.saved_h + o) = done ? z : *(const f32x4*)(p.h_in + o);
      *(f32x4*)(p.saved_c + o) = done ? z : *(const f32x4*)(p.c_in + o);
    }
  }

  // ---- the biases of this lane's units (lane (n, g): units j0 + g * MT + mt, gate v), b_ih + b_hh
  float bias[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int wrow = v * H + j0 + q * MT + mt;
      bias[mt][v] = p.b_ih[wrow] + p.b_hh[wrow];
    }
  __syncthreads();

  // ---- 2. the row block, 16 rows per wave and pass
  const int xblks = IP / 16, nblk = xblks + H / 16;
  const bool xvec = (I & 3) == 0 && ((uintptr_t)p.x & 15) == 0;
  const int nsub = (r1 - r0 + 15) / 16;
  for (int s = wave; s < nsub; s += 4) {
    const int row = r0 + 16 * s + i;  // the row this lane feeds as the B operand, and (n = i) the row it owns in the epilogue
    const bool row_ok = row < r1;
    const int rc = row_ok ? row : r0;  // (a clamped lane computes a column of D nobody stores)
    const bool done = a.dones && a.dones[rc] != 0;
    const float* xrow = p.x + (long long)rc * I;
    const float* hrow = p.h_in + (long long)rc * H;
    // the epilogue's operand, requested now: c of (row, units j0 + q * MT .. + MT - 1)
    float cp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) cp[mt] = 0.f;
    if (!done) load_units<MT>(p.c_in + (long long)rc * H + j0 + q * MT, cp);
    // four partial sums per gate (k block b goes to chain b % 4), added pairwise at the end: chains of K / 4 terms round less than one of
    // K terms - measured, one chain was twice as far from f64 as the eager composition, whose four waves split K - and four independent
    // MFMA chains per tile never wait for the 40-cycle dependent latency
    f32x4 acc[4][MT];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[u][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 cur[4], nxt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = load_b(xrow, hrow, u, q, I, xblks, xvec, done);  // (nblk >= 5: H >= 64 and I >= 1)
    for (int b0 = 0; b0 < nblk; b0 += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        nxt[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (b0 + 4 + u < nblk) nxt[u] = load_b(xrow, hrow, b0 + 4 + u, q, I, xblks, xvec, done);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (b0 + u < nblk) {
          const float* ap = panel + i * KP + 16 * (b0 + u) + 4 * q;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const f32x4 w = *(const f32x4*)(ap + 16 * mt * KP);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[e], cur[u][e], acc[u][mt], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
    }
    // ---- 3. epilogue: sum[v] of lane (n, g) is D[4 g + v][n] = gate v of unit j0 + g * MT + mt, row n
    if (!row_ok) continue;
    float hn[MT], cn[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 sum = (acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt]);
      const float gi = sigmoidf_(sum[0] + bias[mt][0]);
      const float gf = sigmoidf_(sum[1] + bias[mt][1]);
      const float gg = tanhf_(sum[2] + bias[mt][2]);
      const float go = sigmoidf_(sum[3] + bias[mt][3]);
      cn[mt] = gf * cp[mt] + gi * gg;
      hn[mt] = go * tanhf_(cn[mt]);
    }
    const long long o = (long long)row * H + j0 + q * MT;
    store_units<MT>(p.h_out + o, hn);
    store_units<MT>(p.c_out + o, cn);
  }
}

// out = where(dones, 0, raw) for the four state arrays; grid (ceil(N H / 4 / 256), 4 arrays)
struct FinishArgs { const float* in[4]; float* out[4]; const uint8_t* dones; int N, H; };

__global__ __launch_bounds__(256) void lt_memory_finish_kernel(const FinishArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // one float4
  const int h4 = a.H / 4;
  if (idx >= (long long)a.N * h4) return;
  const int r = (int)(idx / h4);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!(a.dones && a.dones[r] != 0)) v = *(const f32x4*)(a.in[blockIdx.y] + 4 * idx);
  *(f32x4*)(a.out[blockIdx.y] + 4 * idx) = v;
}

// ---- host side: validation before anything is launched --------------------------------------------------------------------------------
int refuse(const char* fn, const char* who, const char* field, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: invalid argument: %s%s must be %s", fn, who, field, what);
  lt_set_error(msg);
  return LT_EINVAL;
}

int check_sizes(const char* fn, int N, int H) {
  if (N < 1 || N > 16 * 65535) return refuse(fn, "", "N", "in [1, 16 * 65535]");
  if (H < 64 || H > 512 || (H % 64) != 0) return refuse(fn, "", "H", "a multiple of 64 in [64, 512]");
  return LT_OK;
}

int check_net(const char* fn, const char* who, const lt_memory_net* n, int H) {
  if (!n) return refuse(fn, who, "", "non-null");
  if (n->I < 1 || n->I + H > 1248) return refuse(fn, who, ".I", "at least 1 with I + H <= 1248");
  const struct { const char* name; const void* p; int align; } ptrs[] = {
      {".x", n->x, 4}, {".w_ih", n->w_ih, 4}, {".w_hh", n->w_hh, 16}, {".b_ih", n->b_ih, 16}, {".b_hh", n->b_hh, 16}, {".h_in", n->h_in, 16},
      {".c_in", n->c_in, 16}, {".h_out", n->h_out, 16}, {".c_out", n->c_out, 16}, {".saved_h", n->saved_h, 16}, {".saved_c", n->saved_c, 16}};
  for (const auto& e : ptrs)
    if (!e.p || (uintptr_t)e.p % e.align != 0) return refuse(fn, who, e.name, e.align == 16 ? "non-null and 16-byte aligned" : "non-null and 4-byte aligned");
  if (n->h_out == n->h_in || n->c_out == n->c_in) return refuse(fn, who, ".h_out / .c_out", "another buffer than .h_in / .c_in (ping-pong)");
  return LT_OK;
}

NetArgs net_args(const lt_memory_net* n, int H) {
  NetArgs r;
  r.x = n->x; r.w_ih = n->w_ih; r.w_hh = n->w_hh; r.b_ih = n->b_ih; r.b_hh = n->b_hh; r.h_in = n->h_in; r.c_in = n->c_in;
  r.h_out = n->h_out; r.c_out = n->c_out; r.saved_h = n->saved_h; r.saved_c = n->saved_c;
  r.I = n->I; r.IP = round_up(n->I, 16); r.KP = panel_stride(n->I, H);
  return r;
}

}  // namespace

extern "C" {

int lt_memory_step(const lt_memory_net* actor, const lt_memory_net* critic, const uint8_t* dones, int N, int H, void* stream) {
  const char* fn = "lt_memory_step";
  if (const int rc = check_sizes(fn, N, H)) return rc;
  if (const int rc = check_net(fn, "actor", actor, H)) return rc;
  if (const int rc = check_net(fn, "critic", critic, H)) return rc;
  StepArgs a;
  a.net[0] = net_args(actor, H);
  a.net[1] = net_args(critic, H);
  a.dones = dones; a.N = N; a.H = H;
  const int kp = a.net[0].KP > a.net[1].KP ? a.net[0].KP : a.net[1].KP;
  const int ut = 64 * kp * (int)sizeof(float) <= kLdsBytes ? 16 : 8;  // 32 x 1280 floats fill the LDS exactly: I + H <= 1248 always fits
  const int lds = 4 * ut * kp * (int)sizeof(float);
  // row block: the grid covers the chip about once (one workgroup per CU: the panel takes most of its LDS), whole 64-row passes
  static int cus = 0;  // (every device of a node is the same chip)
  if (cus == 0) {
    int dev = 0, v = 0;
    cus = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
  }
  const int tiles = 2 * (H / ut);
  const int blocks = cus / tiles > 0 ? cus / tiles : 1;
  a.RB = round_up((N + blocks - 1) / blocks, 64);
  const dim3 grid((unsigned)(H / ut), (unsigned)((N + a.RB - 1) / a.RB), 2);
  const void* kernel = ut == 16 ? (const void*)lt_memory_step_kernel<16> : (const void*)lt_memory_step_kernel<8>;
  if (const int e = lt_ensure_dynamic_lds(kernel, kLdsBytes)) { lt_set_error(hipGetErrorString((hipError_t)e)); return LT_EHIP; }
  if (ut == 16) hipLaunchKernelGGL(lt_memory_step_kernel<16>, grid, dim3(256), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(lt_memory_step_kernel<8>, grid, dim3(256), lds, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  return LT_OK;
}

int lt_memory_finish(const float* h_a, const float* c_a, const float* h_c, const float* c_c, const uint8_t* dones, int N, int H,
                     float* out_h_a, float* out_c_a, float* out_h_c, float* out_c_c, void* stream) {
  const char* fn = "lt_memory_finish";
  if (const int rc = check_sizes(fn, N, H)) return rc;
  const struct { const char* name; const void* p; } ptrs[] = {{"h_a", h_a}, {"c_a", c_a}, {"h_c", h_c}, {"c_c", c_c}, {"out_h_a", out_h_a},
                                                             {"out_c_a", out_c_a}, {"out_h_c", out_h_c}, {"out_c_c", out_c_c}};
  for (const auto& e : ptrs)
    if (!e.p || (uintptr_t)e.p % 16 != 0) return refuse(fn, "", e.name, "non-null and 16-byte aligned");
  FinishArgs a;
  a.in[0] = h_a; a.in[1] = c_a; a.in[2] = h_c; a.in[3] = c_c;
  a.out[0] = out_h_a; a.out[1] = out_c_a; a.out[2] = out_h_c; a.out[3] = out_c_c;
  a.dones = dones; a.N = N; a.H = H;
  const long long n4 = (long long)N * (H / 4);
  hipLaunchKernelGGL(lt_memory_finish_kernel, dim3((unsigned)((n4 + 255) / 256), 4), dim3(256), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  return LT_OK;
}

}  // extern "C"
