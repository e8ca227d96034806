// lt_policy.hip - one inference step of a trained recurrent policy (include/lt_policy.h): the memory step below, then lt_mlp_forward's
// launch on the new hidden state.
//
// The rollout kernel (lt_memory_tile.h) is laid out for 4096 rows and up: a workgroup stages a weight panel of up to 137 KiB and walks a
// row block under it.  At play's shape (50 envs) that is 16 workgroups, each pulling its whole panel for 50 rows, and it needs both
// networks and a storage slot.  Here the plan is lt_student_gru_kernel's, with the cells of the memory kernels (lt_memory_cells.h):
//   grid (H / 64, ceil(n / 16)), block 256.  A workgroup stages its 16 rows [x | h] in LDS - the observation normaliser and the done mask
//   are applied as a row is read, tail rows are zeros - and each wave owns 16 hidden units: four 16-row MFMA tiles whose M index is
//   4 g + v (unit u0 + 4 g + mt, row kind v), the rollout kernel's UT = 16 layout, so lane (n, g) of the D layout holds the four sums of
//   four CONSECUTIVE units of row n and the gate arithmetic is the in-register epilogue.  The weights [W_ih | W_hh] stream from global
//   memory / L2, four 16-wide k blocks per lane in flight; there is no panel in LDS and no tile shape depends on n.
//
// Summation order: lt_memory_step_kernel's.  k blocks in index order, the x side first (padded to a multiple of 16 with zeros on both
// operands), then h; block b goes to partial sum b % 4, MFMA step e of a block consumes the k-set {16 b + 4 q + e}; the four partial sums
// are added pairwise, then the cell adds the biases.  With the same Cell::gates this gives the rollout kernel's bits
// (tests/test_hip_policy_step.py).
#include "lt_policy.h"

#include "lt_memory_cells.h"
#include "lt_memory_tile.h"

namespace {

constexpr int RT = 16;  // rows of a workgroup
constexpr int UW = 64;  // hidden units of a workgroup: 16 per wave

struct PolicyArgs {
  const float* x; long long xstride;
  const uint8_t* done;
  const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh;
  const float* mean; const float* std; float eps;
  const float* s_in[2]; float* s_out[2];
  int n, I, IP, H, S;  // IP: I rounded up to 16; S: LDS row stride in floats, IP + H + 4
};

// the A operand of x-side k block `blk` for lane (panel row, q): W_ih[wrow][16 blk + 4 q .. + 3], zeros past I (rows of W_ih are only
// 4-byte aligned unless `wvec`)
__device__ __forceinline__ f32x4 load_w_ih(const float* __restrict__ wrow, int blk, int q, int I, bool wvec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const int k = 16 * blk + 4 * q;
  if (wvec && k + 3 < I) {
    v = *(const f32x4*)(wrow + k);
  } else {
    if (k < I) v[0] = wrow[k];
    if (k + 1 < I) v[1] = wrow[k + 1];
    if (k + 2 < I) v[2] = wrow[k + 2];
    if (k + 3 < I) v[3] = wrow[k + 3];
  }
  return v;
}

template <class Cell> __global__ __launch_bounds__(256) void lt_policy_memory_kernel(const PolicyArgs a) {
  constexpr int NS = Cell::NS, MT = 4;
  extern __shared__ __attribute__((aligned(16))) float rows[];  // [RT][S]: x (normalised) | zeros up to IP | where(done, 0, h)
  const int n = a.n, H = a.H, I = a.I, IP = a.IP, S = a.S;
  const int tid = threadIdx.x, lane = tid & 63, wave = lt::wave_uniform(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.y * RT;

  // ---- 1. the 16 rows, once
  for (int idx = tid; idx < RT * IP; idx += 256) {
    const int r = idx / IP, k = idx - r * IP;
    float v = 0.f;
    if (row0 + r < n && k < I) {
      v = a.x[(long long)(row0 + r) * a.xstride + k];
      // (the torch normaliser's statement bit for bit: the IEEE quotient.  `__fdiv_rn` is not: this toolchain defines it as `/`, which
      // -freciprocal-math makes v_rcp_f32 and a multiplication, one ulp off now and then)
      if (a.mean) v = ieee_div(v - a.mean[k], a.std[k] + a.eps);
    }
    rows[r * S + k] = v;
  }
  const int h4 = H / 4;
  for (int idx = tid; idx < RT * h4; idx += 256) {
    const int r = idx / h4, k4 = idx - r * h4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + r < n && !(a.done && a.done[row0 + r] != 0)) v = *(const f32x4*)(a.s_in[0] + (long long)(row0 + r) * H + 4 * k4);
    *(f32x4*)(rows + r * S + IP + 4 * k4) = v;
  }

  // ---- this lane's part of the epilogue, requested now: row row0 + i, units u0 + 4 q .. + 3
  const int u0 = blockIdx.x * UW + wave * 16;
  const int row = row0 + i;
  const bool row_ok = row < n;
  float bias[MT][4], prev[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    Cell::load_bias(a.b_ih, a.b_hh, H, u0, q * MT, mt, bias[mt]);
    prev[mt] = 0.f;
  }
  if (row_ok && !(a.done && a.done[row] != 0)) load_units<MT>(a.s_in[NS - 1] + (long long)row * H + u0 + q * MT, prev);

  // ---- this lane's rows of the A operand: panel row i of tile mt is row kind v = i % 4 of unit u0 + 4 (i / 4) + mt
  const int v = i & 3;
  const bool ih_on = Cell::ih_used(v), hh_on = Cell::hh_used(v);
  const float* wi[MT];
  const float* wh[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int unit = u0 + 4 * (i >> 2) + mt;
    wi[mt] = a.w_ih + (long long)(Cell::ih_gate(v) * H + unit) * I;
    wh[mt] = a.w_hh + (long long)(Cell::hh_gate(v) * H + unit) * H + 4 * q;
  }
  const bool wvec = (I & 3) == 0 && ((uintptr_t)a.w_ih & 15) == 0;
  __syncthreads();

  // ---- 2. the GEMM: 64 panel rows x 16 rows x (IP + H), four k blocks' operands in flight
  const int xblks = IP / 16, nblk = xblks + H / 16;
  const float* br = rows + i * S + 4 * q;  // (the LDS column of k block b is 16 b on both sides: IP = 16 xblks)
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4][MT];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[u][mt] = zero;
  for (int b0 = 0; b0 < nblk; b0 += 4) {
    f32x4 w[4][MT], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = b0 + u;
      xv[u] = zero;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) w[u][mt] = zero;
      if (b < nblk) {
        xv[u] = *(const f32x4*)(br + 16 * b);
        if (b < xblks) {
          if (ih_on) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) w[u][mt] = load_w_ih(wi[mt], b, q, I, wvec);
          }
        } else if (hh_on) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) w[u][mt] = *(const f32x4*)(wh[mt] + 16 * (b - xblks));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (b0 + u < nblk) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[u][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u][mt][e], xv[u][e], acc[u][mt], 0, 0, 0);
        }
      }
    }
  }

  // ---- 3. epilogue: sum[v] of lane (n, g), tile mt is D[4 g + v][n] = row kind v of unit u0 + 4 g + mt, row n
  if (!row_ok) return;
  float next[NS][MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const f32x4 sum = (acc[0][mt] + acc[1][mt]) + (acc[2][mt] + acc[3][mt]);
    float sn[NS], ga[4];
    Cell::gates(sum, bias[mt], prev[mt], sn, ga);
#pragma unroll
    for (int k = 0; k < NS; ++k) next[k][mt] = sn[k];
  }
  const long long o = (long long)row * H + u0 + q * MT;
  store_units<MT>(a.s_out[0] + o, next[0]);
  if constexpr (NS == 2) store_units<MT>(a.s_out[1] + o, next[1]);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
int check_desc(const char* fn, const lt_policy_desc* d) {
  if (!d) return refuse(fn, "", "desc", "non-null");
  if (d->rnn_type != LT_POLICY_RNN_LSTM && d->rnn_type != LT_POLICY_RNN_GRU) return refuse(fn, "", "rnn_type", "LT_POLICY_RNN_LSTM or LT_POLICY_RNN_GRU");
  if (d->rnn_layers != 1) return refuse(fn, "", "rnn_layers", "1 (a multi-layer memory is not served)");
  const int H = d->rnn_hidden;
  if (H < 64 || H > 512 || (H % 64) != 0) return refuse(fn, "", "rnn_hidden", "a multiple of 64 in [64, 512]");
  if (d->obs_dim < 1 || d->obs_dim + H > 1248) return refuse(fn, "", "obs_dim", "at least 1 with obs_dim + rnn_hidden <= 1248");
  if (d->actor.input_format != LT_ROWS_F32) return refuse(fn, "", "actor.input_format", "LT_ROWS_F32 (bf16 rows are not served)");
  if (d->actor.dims[0] != H) return refuse(fn, "", "actor.dims[0]", "rnn_hidden (the actor reads the hidden state)");
  size_t floats = 0;
  if (lt_mlp_packed_floats(&d->actor, &floats) != LT_OK) return refuse(fn, "", "actor", "a network lt_mlp_forward serves (1 .. LT_MLP_MAX_LAYERS layers, widths in [1, 512])");
  return LT_OK;
}

int check_rows(const char* fn, int64_t n) {
  if (n < 1 || n > 16 * 65535) return refuse(fn, "", "n", "in [1, 16 * 65535]");
  return LT_OK;
}

template <class Cell> int launch_memory(const PolicyArgs& a, void* stream) {
  const kernel_fn<PolicyArgs> kernel = lt_policy_memory_kernel<Cell>;
  const int lds = RT * a.S * (int)sizeof(float);  // at most 16 x 1252 floats
  if (lds > 64 * 1024)
    if (const int rc = allow_lds(kernel)) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(a.H / UW), (unsigned)((a.n + RT - 1) / RT)), dim3(256), lds, (hipStream_t)stream, a);
  return launch_status();
}

}  // namespace

// The memory launch alone, on operands its caller has validated (lt_internal.h): lt_policy_step below, and lt_policy_encoder_step
// (csrc/lt_policy_encoder.hip), which hands it the tail columns of its rows and the tail slices of the statistics.
int lt_policy_memory_launch(int rnn_type, const lt_policy_memory* mem, int I, int H, const float* x, long long x_stride, const uint8_t* done_mask,
                            const float* h_in, const float* c_in, float* h_out, float* c_out, int n, void* stream) {
  PolicyArgs a;
  a.x = x; a.xstride = x_stride; a.done = done_mask;
  a.w_ih = mem->w_ih; a.w_hh = mem->w_hh; a.b_ih = mem->b_ih; a.b_hh = mem->b_hh;
  a.mean = mem->norm_mean; a.std = mem->norm_std; a.eps = mem->norm_eps;
  a.s_in[0] = h_in; a.s_in[1] = c_in; a.s_out[0] = h_out; a.s_out[1] = c_out;
  a.n = n; a.I = I; a.IP = round_up(I, 16); a.H = H; a.S = a.IP + H + 4;
  return rnn_type == LT_POLICY_RNN_LSTM ? launch_memory<LstmCell>(a, stream) : launch_memory<GruCell>(a, stream);
}

extern "C" {

int lt_policy_validate(const lt_policy_desc* desc) { return check_desc("lt_policy_validate", desc); }

int lt_policy_step_launches(const lt_policy_desc* desc, int64_t n) {
  const char* fn = "lt_policy_step_launches";
  if (const int rc = check_desc(fn, desc)) return rc;
  if (const int rc = check_rows(fn, n)) return rc;
  return 2;
}

int lt_policy_step(const lt_policy_desc* desc, const lt_policy_memory* mem, const float* actor_packed, const float* obs,
                   int64_t obs_row_stride, const uint8_t* done_mask, const float* h_in, const float* c_in, float* h_out, float* c_out,
                   int64_t n, float* actions_out, void* stream) {
  const char* fn = "lt_policy_step";
  if (const int rc = check_desc(fn, desc)) return rc;
  if (const int rc = check_rows(fn, n)) return rc;
  const int H = desc->rnn_hidden, I = desc->obs_dim;
  const bool lstm = desc->rnn_type == LT_POLICY_RNN_LSTM;
  if (obs_row_stride < I) return refuse(fn, "", "obs_row_stride", "at least obs_dim");
  if (!mem) return refuse(fn, "", "mem", "non-null");
  if (const int rc = check_ptrs(fn, "", {{"mem.w_ih", mem->w_ih, 4}, {"mem.w_hh", mem->w_hh, 16}, {"mem.b_ih", mem->b_ih, 16}, {"mem.b_hh", mem->b_hh, 16}}))
    return rc;
  if (!mem->norm_mean != !mem->norm_std) return refuse(fn, "", "mem.norm_mean / mem.norm_std", "both NULL or both set");
  if (mem->norm_mean)
    if (const int rc = check_ptrs(fn, "", {{"mem.norm_mean", mem->norm_mean, 4}, {"mem.norm_std", mem->norm_std, 4}})) return rc;
  if (const int rc = check_ptrs(fn, "", {{"actor_packed", actor_packed, 16}, {"obs", obs, 4}, {"h_in", h_in, 16}, {"h_out", h_out, 16},
                                         {"actions_out", actions_out, 4}}))
    return rc;
  if (lstm) {
    if (const int rc = check_ptrs(fn, "", {{"c_in", c_in, 16}, {"c_out", c_out, 16}})) return rc;
  } else {
    if (c_in) return refuse(fn, "", "c_in", "NULL for a GRU");
    if (c_out) return refuse(fn, "", "c_out", "NULL for a GRU");
  }
  const long long nH = (long long)n * H;
  const struct { const char* name; const float* p; } outs[] = {{"h_out", h_out}, {"c_out", c_out}};
  for (const auto& e : outs)
    for (const float* in : {h_in, c_in})
      if (e.p && in && overlaps(e.p, nH, in, nH)) return refuse(fn, "", e.name, "a buffer that does not overlap h_in / c_in (ping-pong)");

  if (const int rc = lt_policy_memory_launch(desc->rnn_type, mem, I, H, obs, obs_row_stride, done_mask, h_in, c_in, h_out, c_out, (int)n, stream))
    return rc;
  return lt_mlp_forward(&desc->actor, actor_packed, h_out, n, actions_out, stream);
}

}  // extern "C"
