// lt_bc.hip - the two ends of the student's behaviour-cloning step (include/lt_bc.h): batch assembly, the masked loss, AdamW.
//
// Each of the three is a string of small torch launches on the default path (distill/replay_buffer.py `_prepare_padded_sequence`,
// distill/student.py `batch_loss`, torch.optim.AdamW over ~28 tensors).  None is compute; here each is one pass over its data:
//   lt_bc_gather_kernel        : a wave per (t, b) element of the padded batch.  The element's trajectory, first row and length are
//                                wave-uniform; the wave copies the policy row and the tactile row as 16-, 8- or 4-byte vectors (or
//                                writes zeros), lane 0 writes the mask byte.  Every output element is written exactly once.
//   lt_bc_loss_partial_kernel  : a lane per row.  The lane sums its row's squared / absolute differences in column order, a butterfly
//                                combines the 64 rows of a wave (every lane ends with the same bits), the four waves are added in
//                                order, and the workgroup writes one partial of four floats.
//   lt_bc_loss_finish_kernel   : four lanes, one per statistic, add the partials in index order and divide.
//   lt_bc_loss_backward_kernel : a lane per element (per four when the width allows).
//   lt_adamw_kernel            : a lane per element (per four when n and the alignment allow).
// No atomics; no sum whose order depends on the schedule of the waves.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lt_host_check.h"
#include "lt_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVE = 64;
constexpr int NW = TPB / WAVE;
static_assert(LT_BC_ROWS_PER_GROUP == TPB, "a lane per row");

template <int V> struct vec_of;
template <> struct vec_of<4> { using type = float4; };
template <> struct vec_of<2> { using type = float2; };
template <> struct vec_of<1> { using type = float; };

// ---- batch assembly ---------------------------------------------------------------------------------------------------------------
struct GatherArgs {
  const float* policy;
  const float* tactile;
  const long long* first;
  const long long* len;
  const long long* traj_idx;
  float* pol;
  float* tac;
  unsigned char* mask;
  long long rows_total, pe, td, num_trajs, nb, num_envs, R, B;
  int vec_pe, vec_td;  // floats per vector: 4, 2 or 1
};

// dst[0 .. width) = src[0 .. width), or zeros if src is null; `width` is a multiple of V and both rows are V * 4-byte aligned
template <int V>
__device__ __forceinline__ void move_row(float* dst, const float* src, long long width, int lane) {
  using T = typename vec_of<V>::type;
  const long long nv = width / V;
  T* d = reinterpret_cast<T*>(dst);
  if (src) {
    const T* s = reinterpret_cast<const T*>(src);
    for (long long i = lane; i < nv; i += WAVE) d[i] = s[i];
  } else {
    T z;
    __builtin_memset(&z, 0, sizeof z);
    for (long long i = lane; i < nv; i += WAVE) d[i] = z;
  }
}

__device__ __forceinline__ void move_row_by(int vec, float* dst, const float* src, long long width, int lane) {
  if (vec == 4) move_row<4>(dst, src, width, lane);
  else if (vec == 2) move_row<2>(dst, src, width, lane);
  else move_row<1>(dst, src, width, lane);
}

__global__ __launch_bounds__(TPB) void lt_bc_gather_kernel(const GatherArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long r = (long long)blockIdx.x * NW + (threadIdx.x >> 6);  // r = t * B + b (wave-uniform)
  if (r >= a.R) return;
  const long long t = r / a.B, b = r - t * a.B;
  long long src_row = -1;  // -1: an invalid element
  if (b < a.nb) {
    const long long k = a.traj_idx[b];
    if (k >= 0 && k < a.num_trajs && t < a.len[k]) {
      const long long row = a.first[k] + t * a.num_envs;
      if (row >= 0 && row < a.rows_total) src_row = row;
    }
  }
  const bool valid = src_row >= 0;
  move_row_by(a.vec_pe, a.pol + r * a.pe, valid ? a.policy + src_row * a.pe : nullptr, a.pe, lane);
  move_row_by(a.vec_td, a.tac + r * a.td, valid ? a.tactile + src_row * a.td : nullptr, a.td, lane);
  if (lane == 0) a.mask[r] = valid ? 1 : 0;
}

// ---- the masked loss ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {  // a butterfly: every lane ends with the same bits
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

struct LossArgs {
  const float* pred;
  const float* target;
  const float* sa;
  const float* ta;
  const unsigned char* mask;
  float* ws;
  long long R, W, A;
  float clip_range;
};

__device__ __forceinline__ float sq_row(const float* x, const float* y, long long n) {
  float s = 0.0f;
  for (long long i = 0; i < n; ++i) {
    const float d = x[i] - y[i];
    s += d * d;
  }
  return s / (float)n;
}

__global__ __launch_bounds__(TPB) void lt_bc_loss_partial_kernel(const LossArgs a) {
  __shared__ float s_part[4][NW];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const long long r = (long long)blockIdx.x * TPB + tid;
  float loss = 0.0f, mse = 0.0f, mae = 0.0f, cnt = 0.0f;
  if (r < a.R) {
    const float m = a.mask[r] ? 1.0f : 0.0f;
    loss = sq_row(a.pred + r * a.W, a.target + r * a.W, a.W) * m;
    const float* sa = a.sa + r * a.A;
    const float* ta = a.ta + r * a.A;
    mse = a.sa == a.pred && a.ta == a.target ? loss : sq_row(sa, ta, a.A) * m;
    const float c = a.clip_range;
    float s = 0.0f;
    for (long long i = 0; i < a.A; ++i) {
      float x = sa[i], y = ta[i];
      if (c > 0.0f) {
        x = fminf(fmaxf(x, -c), c);
        y = fminf(fmaxf(y, -c), c);
      }
      s += fabsf(x - y);
    }
    mae = s / (float)a.A * m;
    cnt = m;
  }
  loss = wave_sum(loss);
  mse = wave_sum(mse);
  mae = wave_sum(mae);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    s_part[0][wave] = loss;
    s_part[1][wave] = mse;
    s_part[2][wave] = mae;
    s_part[3][wave] = cnt;
  }
  __syncthreads();
  if (tid < 4) {
    float s = s_part[tid][0];
    for (int w = 1; w < NW; ++w) s += s_part[tid][w];
    a.ws[4 * (long long)blockIdx.x + tid] = s;
  }
}

// lanes 0..2: the three sums; every lane: the count (exact in int64; one conversion, as the eager code's int64 mask sum has)
__global__ __launch_bounds__(WAVE) void lt_bc_loss_finish_kernel(const float* ws, long long nblk, float action_scale, float* stats) {
  const int tid = threadIdx.x;
  if (tid >= 3) return;
  long long count = 0;
  float s = 0.0f;
  for (long long k = 0; k < nblk; ++k) {
    count += (long long)ws[4 * k + 3];
    s += ws[4 * k + tid];
  }
  const float denom = (float)count;
  s = s / denom;
  if (tid == LT_BC_ACTION_MAE) s *= action_scale;
  stats[tid] = s;
  if (tid == 0) stats[LT_BC_DENOM] = denom;
}

template <int V>
__global__ __launch_bounds__(TPB) void lt_bc_loss_backward_kernel(const float* pred, const float* target, const unsigned char* mask, const float* g,
                                                                  const float* stats, float* d_pred, long long R, long long W) {
  using T = typename vec_of<V>::type;
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;  // vector index
  const long long wv = W / V;
  if (i >= R * wv) return;
  const long long r = i / wv;
  const float coef = (g[0] / stats[LT_BC_DENOM]) * (mask[r] ? 1.0f : 0.0f) / (float)W;
  const T p = reinterpret_cast<const T*>(pred)[i], q = reinterpret_cast<const T*>(target)[i];
  T d;
  const float* pf = reinterpret_cast<const float*>(&p);
  const float* qf = reinterpret_cast<const float*>(&q);
  float* df = reinterpret_cast<float*>(&d);
#pragma unroll
  for (int j = 0; j < V; ++j) df[j] = coef * (2.0f * (pf[j] - qf[j]));
  reinterpret_cast<T*>(d_pred)[i] = d;
}

// ---- AdamW ---------------------------------------------------------------------------------------------------------------------------
struct AdamwArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
  float decay, one_minus_b1, b2, one_minus_b2, step_size, bc2_sqrt, eps;
};

template <int V>
__global__ __launch_bounds__(TPB) void lt_adamw_kernel(const AdamwArgs a) {
  using T = typename vec_of<V>::type;
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;  // vector index
  if (i >= a.n / V) return;
  T p = reinterpret_cast<T*>(a.p)[i], m = reinterpret_cast<T*>(a.m)[i], v = reinterpret_cast<T*>(a.v)[i];
  const T g = reinterpret_cast<const T*>(a.g)[i];
  float* pf = reinterpret_cast<float*>(&p);
  float* mf = reinterpret_cast<float*>(&m);
  float* vf = reinterpret_cast<float*>(&v);
  const float* gf = reinterpret_cast<const float*>(&g);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float gj = gf[j];
    const float mj = mf[j] + a.one_minus_b1 * (gj - mf[j]);
    const float vj = a.b2 * vf[j] + a.one_minus_b2 * (gj * gj);
    const float denom = sqrtf(vj) / a.bc2_sqrt + a.eps;
    pf[j] = pf[j] * a.decay - a.step_size * (mj / denom);
    mf[j] = mj;
    vf[j] = vj;
  }
  reinterpret_cast<T*>(a.p)[i] = p;
  reinterpret_cast<T*>(a.m)[i] = m;
  reinterpret_cast<T*>(a.v)[i] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
bool misaligned(const void* p, size_t bytes) { return (uintptr_t)p % bytes != 0; }

// floats per vector for rows of `width` floats that start at a and at b: the widest of 4, 2, 1 that divides the width and both alignments
int row_vec(int64_t width, const void* a, const void* b) {
  for (int v = 4; v > 1; v >>= 1)
    if (width % v == 0 && !misaligned(a, 4 * v) && !misaligned(b, 4 * v)) return v;
  return 1;
}

constexpr int64_t MAX_GRID = INT32_MAX;  // grid.x

int64_t loss_groups(int64_t R) { return (R + TPB - 1) / TPB; }

}  // namespace

extern "C" {

int lt_bc_gather(const float* policy, const float* tactile, int64_t rows_total, int64_t pe, int64_t td, const int64_t* first, const int64_t* len,
                 int64_t num_trajs, const int64_t* traj_idx, int64_t nb, int64_t num_envs, int64_t L, int64_t B, float* pol, float* tac,
                 uint8_t* mask, void* stream) {
  const char* fn = "lt_bc_gather";
  if (L < 1) return refuse(fn, "L must be at least 1");
  if (B < 1) return refuse(fn, "B must be at least 1");
  if (L > MAX_GRID / B) return refuse(fn, "L * B must be below 2^31");
  if (rows_total < 1) return refuse(fn, "rows_total must be at least 1");
  if (pe < 1 || pe > INT32_MAX) return refuse(fn, "pe must be in [1, 2^31)");
  if (td < 1 || td > INT32_MAX) return refuse(fn, "td must be in [1, 2^31)");
  if (num_trajs < 1) return refuse(fn, "num_trajs must be at least 1");
  if (nb < 0 || nb > B) return refuse(fn, "nb must be in [0, B]");
  if (num_envs < 1) return refuse(fn, "num_envs must be at least 1");
  if (!policy || misaligned(policy, 4)) return refuse(fn, "policy must be non-null and 4-byte aligned");
  if (!tactile || misaligned(tactile, 4)) return refuse(fn, "tactile must be non-null and 4-byte aligned");
  if (!first || misaligned(first, 8)) return refuse(fn, "first must be non-null and 8-byte aligned");
  if (!len || misaligned(len, 8)) return refuse(fn, "len must be non-null and 8-byte aligned");
  if ((nb > 0 && !traj_idx) || misaligned(traj_idx, 8)) return refuse(fn, "traj_idx must be 8-byte aligned, and non-null when nb is not 0");
  if (!pol || misaligned(pol, 4)) return refuse(fn, "pol must be non-null and 4-byte aligned");
  if (!tac || misaligned(tac, 4)) return refuse(fn, "tac must be non-null and 4-byte aligned");
  if (!mask) return refuse(fn, "mask must be non-null");
  GatherArgs a;
  a.policy = policy; a.tactile = tactile; a.first = (const long long*)first; a.len = (const long long*)len;
  a.traj_idx = (const long long*)traj_idx; a.pol = pol; a.tac = tac; a.mask = mask;
  a.rows_total = rows_total; a.pe = pe; a.td = td; a.num_trajs = num_trajs; a.nb = nb; a.num_envs = num_envs; a.R = L * B; a.B = B;
  a.vec_pe = row_vec(pe, policy, pol);
  a.vec_td = row_vec(td, tactile, tac);
  hipLaunchKernelGGL(lt_bc_gather_kernel, dim3((unsigned)((a.R + NW - 1) / NW)), dim3(TPB), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

int lt_bc_loss_ws_floats(int64_t R, size_t* floats) {
  const char* fn = "lt_bc_loss_ws_floats";
  if (R < 1 || R > MAX_GRID) return refuse(fn, "R must be in [1, 2^31)");
  if (!floats) return refuse(fn, "floats must be non-null");
  *floats = (size_t)4 * (size_t)loss_groups(R);
  return LT_OK;
}

int lt_bc_loss_forward(const float* pred, const float* target, int64_t W, const float* sa_or_null, const float* ta_or_null, int64_t A,
                       const uint8_t* mask, int64_t R, float clip_range, float action_scale, float* stats, float* ws, void* stream) {
  const char* fn = "lt_bc_loss_forward";
  if (R < 1 || R > MAX_GRID) return refuse(fn, "R must be in [1, 2^31)");
  if (W < 1 || W > LT_BC_MAX_WIDTH) return refuse(fn, "W must be in [1, LT_BC_MAX_WIDTH]");
  if (!pred || misaligned(pred, 4)) return refuse(fn, "pred must be non-null and 4-byte aligned");
  if (!target || misaligned(target, 4)) return refuse(fn, "target must be non-null and 4-byte aligned");
  if (!sa_or_null != !ta_or_null) return refuse(fn, "sa and ta must be given together");
  if (misaligned(sa_or_null, 4)) return refuse(fn, "sa must be 4-byte aligned");
  if (misaligned(ta_or_null, 4)) return refuse(fn, "ta must be 4-byte aligned");
  if (sa_or_null && (A < 1 || A > LT_BC_MAX_WIDTH)) return refuse(fn, "A must be in [1, LT_BC_MAX_WIDTH]");
  if (!mask) return refuse(fn, "mask must be non-null");
  if (!stats || misaligned(stats, 16)) return refuse(fn, "stats must be non-null and 16-byte aligned");
  if (!ws || misaligned(ws, 4)) return refuse(fn, "ws must be non-null and 4-byte aligned");
  LossArgs a;
  a.pred = pred; a.target = target; a.sa = sa_or_null ? sa_or_null : pred; a.ta = ta_or_null ? ta_or_null : target; a.mask = mask; a.ws = ws;
  a.R = R; a.W = W; a.A = sa_or_null ? A : W; a.clip_range = clip_range;
  const int64_t nblk = loss_groups(R);
  hipLaunchKernelGGL(lt_bc_loss_partial_kernel, dim3((unsigned)nblk), dim3(TPB), 0, (hipStream_t)stream, a);
  if (int rc = launch_status(fn)) return rc;
  hipLaunchKernelGGL(lt_bc_loss_finish_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, (const float*)ws, (long long)nblk, action_scale, stats);
  return launch_status(fn);
}

int lt_bc_loss_backward(const float* pred, const float* target, int64_t W, const uint8_t* mask, int64_t R, const float* g, const float* stats,
                        float* d_pred, void* stream) {
  const char* fn = "lt_bc_loss_backward";
  if (R < 1 || R > MAX_GRID) return refuse(fn, "R must be in [1, 2^31)");
  if (W < 1 || W > LT_BC_MAX_WIDTH) return refuse(fn, "W must be in [1, LT_BC_MAX_WIDTH]");
  if (!pred || misaligned(pred, 4)) return refuse(fn, "pred must be non-null and 4-byte aligned");
  if (!target || misaligned(target, 4)) return refuse(fn, "target must be non-null and 4-byte aligned");
  if (!mask) return refuse(fn, "mask must be non-null");
  if (!g || misaligned(g, 4)) return refuse(fn, "g must be non-null and 4-byte aligned");
  if (!stats || misaligned(stats, 16)) return refuse(fn, "stats must be non-null and 16-byte aligned");
  if (!d_pred || misaligned(d_pred, 4)) return refuse(fn, "d_pred must be non-null and 4-byte aligned");
  const bool wide = W % 4 == 0 && !misaligned(pred, 16) && !misaligned(target, 16) && !misaligned(d_pred, 16);
  const int64_t vecs = R * (wide ? W / 4 : W);  // < 2^31 * 2^12
  const int64_t blocks = (vecs + TPB - 1) / TPB;
  if (blocks > MAX_GRID) return refuse(fn, "R * W is too large for one launch");
  if (wide)
    hipLaunchKernelGGL(lt_bc_loss_backward_kernel<4>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, pred, target, mask, g, stats, d_pred,
                       (long long)R, (long long)W);
  else
    hipLaunchKernelGGL(lt_bc_loss_backward_kernel<1>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, pred, target, mask, g, stats, d_pred,
                       (long long)R, (long long)W);
  return launch_status(fn);
}

int lt_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int64_t step, void* stream) {
  const char* fn = "lt_adamw_step";
  if (n < 1) return refuse(fn, "n must be at least 1");
  if (step < 1) return refuse(fn, "step must be at least 1 (the 1-based count of this update)");
  if (!params || misaligned(params, 4)) return refuse(fn, "params must be non-null and 4-byte aligned");
  if (!grads || misaligned(grads, 4)) return refuse(fn, "grads must be non-null and 4-byte aligned");
  if (!exp_avg || misaligned(exp_avg, 4)) return refuse(fn, "exp_avg must be non-null and 4-byte aligned");
  if (!exp_avg_sq || misaligned(exp_avg_sq, 4)) return refuse(fn, "exp_avg_sq must be non-null and 4-byte aligned");
  if (lr < 0.0) return refuse(fn, "lr must not be negative");
  if (beta1 < 0.0 || beta1 >= 1.0) return refuse(fn, "beta1 must be in [0, 1)");
  if (beta2 < 0.0 || beta2 >= 1.0) return refuse(fn, "beta2 must be in [0, 1)");
  if (eps < 0.0) return refuse(fn, "eps must not be negative");
  if (weight_decay < 0.0) return refuse(fn, "weight_decay must not be negative");
  const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
  AdamwArgs a;
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
  a.decay = (float)(1.0 - lr * weight_decay); a.one_minus_b1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.one_minus_b2 = (float)(1.0 - beta2);
  a.step_size = (float)(lr / bc1); a.bc2_sqrt = (float)std::sqrt(bc2); a.eps = (float)eps;
  const bool wide = n % 4 == 0 && !misaligned(params, 16) && !misaligned(grads, 16) && !misaligned(exp_avg, 16) && !misaligned(exp_avg_sq, 16);
  const int64_t blocks = ((wide ? n / 4 : n) + TPB - 1) / TPB;
  if (blocks > MAX_GRID) return refuse(fn, "n is too large for one launch");
  if (wide)
    hipLaunchKernelGGL(lt_adamw_kernel<4>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(lt_adamw_kernel<1>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // extern "C"
