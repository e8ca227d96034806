// The mirror-symmetric PPO update (include/lt_ppo_sym.h): the packed table of a signed column permutation, the once-per-update gather of
// every minibatch's rows with their mirror images, and the minibatch loss with its gradients for the augmented batch [original; mirrored];
// and (include/lt_ppo_mirror.h) the loss of the update WITHOUT augmentation, where the actor alone runs on [original; mirrored].
//
// Reference: loco_rl/loco_rl/algorithms/ppo.py:216-246 (augmentation: observations and actions mirrored, old log-prob / advantages /
// returns / target values repeated) and :304-337 (mirror loss: MSE between the actor's mean on the mirrored observation and the mirror
// of its mean on the original one, the latter detached).  The per-row arithmetic is lt_ppo_loss_kernel's, from the one text of
// lt_ppo_device.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "lt_env.h"
#include "lt_host_check.h"
#include "lt_internal.h"
#include "lt_ppo_device.h"
#include "lt_ppo_mirror.h"
#include "lt_ppo_sym.h"

namespace {

constexpr unsigned SIGN_BIT = 0x80000000u;

// ---- the table ---------------------------------------------------------------------------------------------------------------------
// The host-checked table rides in the launch's arguments (16 bits a column: src in the low 15, the sign in the top one - 2 KiB at
// D = 1024), so no host buffer has to outlive the call and nothing is copied from pageable memory behind the caller's back.
struct PackedTable { unsigned short e[LT_SYM_MAX_D]; };

__global__ __launch_bounds__(256) void lt_sym_table_pack_kernel(const PackedTable T, int D, int* __restrict__ table) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < D) table[c] = (int)((unsigned)(T.e[c] & 0x7FFFu) | ((T.e[c] & 0x8000u) ? SIGN_BIT : 0u));
}

// ---- the gather --------------------------------------------------------------------------------------------------------------------
// A block keeps the table in LDS and walks GR_ROWS consecutive minibatch rows, a wave per row at a time: the wave loads the storage row
// coalesced (one element a lane and instruction: rows of 270 floats or 270 bf16 need no alignment beyond the element's), stores it as the
// original half and into the wave's LDS row, and reads the mirrored half back out of LDS through the table.
constexpr int GR_ROWS = 16;  // rows per block (4 per wave): 6144 blocks at 98 304 rows

template <bool BF16>
__global__ __launch_bounds__(256) void lt_sym_gather_rows_kernel(const void* __restrict__ rows, long long R, int D, const long long* __restrict__ idx,
                                                                 long long total, long long m, const int* __restrict__ table, float* __restrict__ out) {
  __shared__ int tab[LT_SYM_MAX_D];
  __shared__ unsigned row_lds[4][LT_SYM_MAX_D];
  for (int c = threadIdx.x; c < D; c += 256) tab[c] = table[c];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* const mine = row_lds[wave];
  for (int k = 0; k < GR_ROWS / 4; ++k) {  // (the same trip count in every wave: the barriers below are block-wide)
    const long long g = (long long)blockIdx.x * GR_ROWS + k * 4 + wave;  // minibatch row b * m + j
    const long long s = g < total ? idx[g] : -1;
    const bool ok = s >= 0 && s < R;
    const long long b = g / m, j = g - b * m;
    float* const o0 = out + ((b * 2) * m + j) * D;
    float* const o1 = out + ((b * 2 + 1) * m + j) * D;
    if (ok) {
      for (int c = lane; c < D; c += 64) {
        unsigned w;
        if constexpr (BF16) w = (unsigned)((const unsigned short*)rows)[s * D + c] << 16;  // bf16 -> f32: exact
        else w = ((const unsigned*)rows)[s * D + c];
        mine[c] = w;
        o0[c] = __uint_as_float(w);
      }
    }
    __syncthreads();  // the wave's row and (first trip) the table are in LDS
    if (ok) {
      for (int c = lane; c < D; c += 64) {
        const unsigned t = (unsigned)tab[c];
        o1[c] = __uint_as_float(mine[min((int)(t & 0x7FFFu), D - 1)] ^ (t & SIGN_BIT));  // (a packed table of D columns holds src < D)
      }
    }
    __syncthreads();  // before the next trip overwrites the row
  }
}

// ---- the loss ----------------------------------------------------------------------------------------------------------------------
// A thread owns the pair (r, M + r).  acc as lt_ppo_loss_kernel's, with [3] the sum of the squared mirror differences; the sums of
// the surrogate and the value loss run over both rows of the pair, the KL over row r alone.  MIRROR: the mirror loss is part of the
// loss (mirror_coeff != 0); without it the term is formed for the log alone and leaves dmu untouched.
template <bool LOG, bool NORM, bool MIRROR>
__global__ __launch_bounds__(256) void lt_ppo_loss_sym_kernel(const float* __restrict__ mu, const float* __restrict__ stdp, const float* __restrict__ value,
                                                              const float* __restrict__ actions, const float* __restrict__ old_logp,
                                                              const float* __restrict__ adv, const float* __restrict__ returns,
                                                              const float* __restrict__ old_values, const float* __restrict__ old_mu,
                                                              const float* __restrict__ old_sigma, const long long* __restrict__ idx, long long M, int A,
                                                              float clip, float vcoef, int clipped_value, const float* __restrict__ adv_stats,
                                                              const int* __restrict__ act_table, float mirror_scale, float* __restrict__ dmu,
                                                              float* __restrict__ dvalue, float* __restrict__ acc) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool ok = row < M;
  const long long src = (ok && idx) ? idx[row] : row;  // row of the rollout storage this pair was drawn from
  __shared__ float sigma_lds[MAX_A];  // (LOG alone; unreferenced otherwise)
  if constexpr (LOG) {
    if ((int)threadIdx.x < A) sigma_lds[threadIdx.x] = lt_sigma_of_log(stdp[threadIdx.x]);
    __syncthreads();
  }
  float part[4 + MAX_A];
  float amax_mu = 0.f, amax_v = 0.f;
#pragma unroll
  for (int i = 0; i < 4 + MAX_A; ++i) part[i] = 0.f;
  if (ok) {
    const float inv_2m = 1.f / (float)(2 * M);
    const long long row1 = M + row;
    float logp0 = 0.f, logp1 = 0.f, kl = 0.f, sq = 0.f;
    float z0[MAX_A], z1[MAX_A], isg[MAX_A], d[MAX_A];
#pragma unroll
    for (int a = 0; a < MAX_A; ++a) {
      if (a < A) {
        const unsigned t = (unsigned)act_table[a];
        const int sa = min((int)(t & 0x7FFFu), A - 1);  // (a packed table of A columns holds src < A; the clamp keeps any other in the row)
        const unsigned flip = t & SIGN_BIT;
        const float sg = LOG ? sigma_lds[a] : stdp[a], m0 = mu[row * A + a], m1 = mu[row1 * A + a], x0 = actions[src * A + a];
        const float x1 = __uint_as_float(__float_as_uint(actions[src * A + sa]) ^ flip);  // the mirrored action
        const float om = old_mu[src * A + a], os = old_sigma[src * A + a];
        isg[a] = 1.f / sg;
        z0[a] = (x0 - m0) * isg[a];
        z1[a] = (x1 - m1) * isg[a];
        logp0 += lt_ppo_logp_term<LOG>(z0[a], sg, stdp[a]);
        logp1 += lt_ppo_logp_term<LOG>(z1[a], sg, stdp[a]);
        kl += lt_ppo_kl_term(sg, os, om, m0);
        d[a] = m1 - __uint_as_float(__float_as_uint(mu[row * A + sa]) ^ flip);  // against the mirror of the original row's mean (detached)
        sq += d[a] * d[a];
      }
    }
    float advr = adv[src];
    if constexpr (NORM) advr = (advr - adv_stats[0]) * adv_stats[1];
    const float olp = old_logp[src];
    const float ratio0 = __expf(logp0 - olp), ratio1 = __expf(logp1 - olp);
    LT_PPO_SURROGATE(advr, ratio0, clip, s1a, s2a, dsurr0)
    LT_PPO_SURROGATE(advr, ratio1, clip, s1b, s2b, dsurr1)
    const float dlogp0 = dsurr0 * ratio0 * inv_2m, dlogp1 = dsurr1 * ratio1 * inv_2m;
#pragma unroll
    for (int a = 0; a < MAX_A; ++a) {
      if (a < A) {
        const float g0 = dlogp0 * z0[a] * isg[a];
        float g1 = dlogp1 * z1[a] * isg[a];
        if constexpr (MIRROR) g1 += mirror_scale * d[a];  // mirror_coeff * 2 d / (M A)
        dmu[row * A + a] = g0;
        dmu[row1 * A + a] = g1;
        amax_mu = fmaxf(amax_mu, fmaxf(fabsf(g0), fabsf(g1)));
        if constexpr (LOG) part[4 + a] = dlogp0 * (z0[a] * z0[a] - 1.f) + dlogp1 * (z1[a] * z1[a] - 1.f);
        else part[4 + a] = (dlogp0 * (z0[a] * z0[a] - 1.f) + dlogp1 * (z1[a] * z1[a] - 1.f)) * isg[a];
      }
    }
    const float v0 = value[row], v1 = value[row1], R = returns[src];
    float vl0, dv0, vl1, dv1;
    LT_PPO_VALUE_LOSS(v0, R, old_values, src, clip, clipped_value, vl0, dv0)
    LT_PPO_VALUE_LOSS(v1, R, old_values, src, clip, clipped_value, vl1, dv1)
    dvalue[row] = vcoef * dv0 * inv_2m;
    dvalue[row1] = vcoef * dv1 * inv_2m;
    amax_v = fmaxf(fabsf(vcoef * dv0 * inv_2m), fabsf(vcoef * dv1 * inv_2m));
    part[0] = fmaxf(s1a, s2a) + fmaxf(s1b, s2b);
    part[1] = vl0 + vl1;
    part[2] = kl;
    part[3] = sq;
  }
  LT_PPO_BLOCK_REDUCE(part, amax_mu, amax_v, A, acc, true)
}

// The one-wave finish: lt_ppo_finalize with the divisor 2 M, then lane 0 restates the KL over its M rows, forms the symmetry loss and
// adds it where asked.
__global__ __launch_bounds__(64) void lt_ppo_sym_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ stdp, int A, float inv_2m, float inv_m,
                                                                 float inv_ma, float vcoef, float ecoef, int std_is_log, float mirror_coeff,
                                                                 float* __restrict__ out, float* __restrict__ sym_sum) {
  lt_ppo_finalize(acc, stdp, A, inv_2m, vcoef, ecoef, std_is_log, out);
  if (threadIdx.x == 0) {
    const float sym = acc[3] * inv_ma;
    out[4] = acc[2] * inv_m;
    out[5] = sym;
    if (mirror_coeff != 0.f) out[0] += mirror_coeff * sym;
    if (sym_sum) *sym_sum += sym;
  }
}

// ---- the loss, mirror term alone (include/lt_ppo_mirror.h) -------------------------------------------------------------------------
// A thread owns row r: scored as lt_ppo_loss_kernel scores it (divisor M), and the mirror difference of the pair (r, M + r), whose
// gradient goes into row M + r alone.  MIRROR as above; without it row M + r of dmu is written as zeros (the backward chain may still
// read it).  acc as lt_ppo_loss_sym_kernel's.
template <bool LOG, bool NORM, bool MIRROR>
__global__ __launch_bounds__(256) void lt_ppo_loss_mirror_kernel(const float* __restrict__ mu, const float* __restrict__ stdp, const float* __restrict__ value,
                                                                 const float* __restrict__ actions, const float* __restrict__ old_logp,
                                                                 const float* __restrict__ adv, const float* __restrict__ returns,
                                                                 const float* __restrict__ old_values, const float* __restrict__ old_mu,
                                                                 const float* __restrict__ old_sigma, const long long* __restrict__ idx, long long M, int A,
                                                                 float clip, float vcoef, int clipped_value, const float* __restrict__ adv_stats,
                                                                 const int* __restrict__ act_table, float mirror_scale, float* __restrict__ dmu,
                                                                 float* __restrict__ dvalue, float* __restrict__ acc) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool ok = row < M;
  const long long src = (ok && idx) ? idx[row] : row;  // row of the rollout storage this minibatch row was drawn from
  __shared__ float sigma_lds[MAX_A];  // (LOG alone; unreferenced otherwise)
  if constexpr (LOG) {
    if ((int)threadIdx.x < A) sigma_lds[threadIdx.x] = lt_sigma_of_log(stdp[threadIdx.x]);
    __syncthreads();
  }
  float part[4 + MAX_A];
  float amax_mu = 0.f, amax_v = 0.f;
#pragma unroll
  for (int i = 0; i < 4 + MAX_A; ++i) part[i] = 0.f;
  if (ok) {
    const float inv_m = 1.f / (float)M;
    const long long row1 = M + row;
    float logp = 0.f, kl = 0.f, sq = 0.f;
    float z[MAX_A], isg[MAX_A], d[MAX_A];
#pragma unroll
    for (int a = 0; a < MAX_A; ++a) {
      if (a < A) {
        const unsigned t = (unsigned)act_table[a];
        const int sa = min((int)(t & 0x7FFFu), A - 1);  // (a packed table of A columns holds src < A; the clamp keeps any other in the row)
        const float sg = LOG ? sigma_lds[a] : stdp[a], m = mu[row * A + a], x = actions[src * A + a];
        const float om = old_mu[src * A + a], os = old_sigma[src * A + a];
        isg[a] = 1.f / sg;
        z[a] = (x - m) * isg[a];
        logp += lt_ppo_logp_term<LOG>(z[a], sg, stdp[a]);
        kl += lt_ppo_kl_term(sg, os, om, m);
        d[a] = mu[row1 * A + a] - __uint_as_float(__float_as_uint(mu[row * A + sa]) ^ (t & SIGN_BIT));  // against the mirror of row r's mean (detached)
        sq += d[a] * d[a];
      }
    }
    float advr = adv[src];
    if constexpr (NORM) advr = (advr - adv_stats[0]) * adv_stats[1];
    const float ratio = __expf(logp - old_logp[src]);
    LT_PPO_SURROGATE(advr, ratio, clip, s1, s2, dsurr_dratio)
    const float dlogp = dsurr_dratio * ratio * inv_m;
#pragma unroll
    for (int a = 0; a < MAX_A; ++a) {
      if (a < A) {
        const float g0 = dlogp * z[a] * isg[a];
        const float g1 = MIRROR ? mirror_scale * d[a] : 0.f;  // mirror_coeff * 2 d / (M A)
        dmu[row * A + a] = g0;
        dmu[row1 * A + a] = g1;
        amax_mu = fmaxf(amax_mu, fmaxf(fabsf(g0), fabsf(g1)));
        if constexpr (LOG) part[4 + a] = dlogp * (z[a] * z[a] - 1.f);
        else part[4 + a] = dlogp * (z[a] * z[a] - 1.f) * isg[a];
      }
    }
    const float v = value[row], R = returns[src];
    float vl, dv;
    LT_PPO_VALUE_LOSS(v, R, old_values, src, clip, clipped_value, vl, dv)
    dvalue[row] = vcoef * dv * inv_m;
    amax_v = fabsf(vcoef * dv * inv_m);
    part[0] = fmaxf(s1, s2);
    part[1] = vl;
    part[2] = kl;
    part[3] = sq;
  }
  LT_PPO_BLOCK_REDUCE(part, amax_mu, amax_v, A, acc, true)
}

// The one-wave finish: lt_ppo_finalize with the divisor M, then lane 0 forms the symmetry loss and adds it where asked.
__global__ __launch_bounds__(64) void lt_ppo_mirror_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ stdp, int A, float inv_m, float inv_ma,
                                                                    float vcoef, float ecoef, int std_is_log, float mirror_coeff, float* __restrict__ out,
                                                                    float* __restrict__ sym_sum) {
  lt_ppo_finalize(acc, stdp, A, inv_m, vcoef, ecoef, std_is_log, out);
  if (threadIdx.x == 0) {
    const float sym = acc[3] * inv_ma;
    out[5] = sym;
    if (mirror_coeff != 0.f) out[0] += mirror_coeff * sym;
    if (sym_sum) *sym_sum += sym;
  }
}

}  // namespace

extern "C" int lt_sym_table_pack(const int32_t* src_host, const float* sign_host, int D, int32_t* table, void* stream) {
  const char* fn = "lt_sym_table_pack";
  if (!src_host) return refuse(fn, "", "src_host", "non-null");
  if (!sign_host) return refuse(fn, "", "sign_host", "non-null");
  if (D < 1 || D > LT_SYM_MAX_D) return refuse(fn, "", "D", "in [1, 1024]");
  const ptr_check ptrs[] = {{"table", table, 4}};
  if (const int rc = check_ptrs(fn, "", ptrs)) return rc;
  PackedTable T = {};
  bool seen[LT_SYM_MAX_D] = {};
  for (int c = 0; c < D; ++c) {
    const int32_t s = src_host[c];
    if (s < 0 || s >= D || seen[s]) return refuse(fn, "", "src", "a permutation of 0 .. D - 1");
    seen[s] = true;
    uint32_t bits;  // (by bit pattern: the library is built with -ffinite-math-only, under which a comparison lets a NaN through)
    memcpy(&bits, sign_host + c, sizeof bits);
    if (bits != 0x3F800000u && bits != 0xBF800000u) return refuse(fn, "", "sign", "+1 or -1 in every column");
    T.e[c] = (unsigned short)(s | (bits >> 31 ? 0x8000 : 0));
  }
  hipLaunchKernelGGL(lt_sym_table_pack_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, D, (int*)table);
  return launch_status(fn);
}

extern "C" int lt_sym_gather_rows(const void* rows, int rows_bf16, int64_t R, int D, const int64_t* idx, int nmb, int64_t m, const int32_t* table,
                                  float* out, void* stream) {
  const char* fn = "lt_sym_gather_rows";
  if (!rows || (uintptr_t)rows % (rows_bf16 ? 2 : 4) != 0) return refuse(fn, "", "rows", rows_bf16 ? "non-null and 2-byte aligned" : "non-null and 4-byte aligned");
  if (!idx || (uintptr_t)idx % 8 != 0) return refuse(fn, "", "idx", "non-null and 8-byte aligned");
  const ptr_check ptrs[] = {{"table", table, 4}, {"out", out, 4}};
  if (const int rc = check_ptrs(fn, "", ptrs)) return rc;
  if (D < 1 || D > LT_SYM_MAX_D) return refuse(fn, "", "D", "in [1, 1024]");
  if (R < 1) return refuse(fn, "", "R", ">= 1");
  if (nmb < 1) return refuse(fn, "", "nmb", ">= 1");
  if (m < 1) return refuse(fn, "", "m", ">= 1");
  const long long total = (long long)nmb * m;
  if (total > (long long)0x7FFFFFFF * GR_ROWS) return refuse(fn, "", "nmb * m", "within one launch's 2^31 blocks of 16 rows");
  const dim3 grid((unsigned)((total + GR_ROWS - 1) / GR_ROWS));
  if (rows_bf16)
    hipLaunchKernelGGL((lt_sym_gather_rows_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, rows, (long long)R, D, (const long long*)idx, total,
                       (long long)m, (const int*)table, out);
  else
    hipLaunchKernelGGL((lt_sym_gather_rows_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, rows, (long long)R, D, (const long long*)idx, total,
                       (long long)m, (const int*)table, out);
  return launch_status(fn);
}

extern "C" int lt_ppo_loss_sym(const float* mu, const float* stdp, const float* value, const float* actions, const float* old_logp, const float* adv,
                               const float* returns, const float* old_values, const float* old_mu, const float* old_sigma, const int64_t* idx, int64_t M,
                               int A, float clip, float value_loss_coef, float entropy_coef, int use_clipped_value_loss, int std_is_log,
                               const float* adv_stats, const int32_t* act_table, float mirror_coeff, float* dmu, float* dvalue, float* acc, float* out,
                               float* sym_sum, void* stream) {
  const char* fn = "lt_ppo_loss_sym";
  const ptr_check ptrs[] = {{"mu", mu, 4}, {"std", stdp, 4}, {"value", value, 4}, {"actions", actions, 4}, {"old_logp", old_logp, 4}, {"adv", adv, 4},
                            {"returns", returns, 4}, {"old_values", old_values, 4}, {"old_mu", old_mu, 4}, {"old_sigma", old_sigma, 4},
                            {"act_table", act_table, 4}, {"dmu", dmu, 4}, {"dvalue", dvalue, 4}, {"acc", acc, 4}};
  if (const int rc = check_ptrs(fn, "", ptrs)) return rc;
  if ((uintptr_t)idx % 8 != 0) return refuse(fn, "", "idx", "NULL or 8-byte aligned");
  if ((uintptr_t)adv_stats % 4 != 0) return refuse(fn, "", "adv_stats", "NULL or 4-byte aligned");
  if ((uintptr_t)out % 4 != 0) return refuse(fn, "", "out", "NULL or 4-byte aligned");
  if ((uintptr_t)sym_sum % 4 != 0) return refuse(fn, "", "sym_sum", "NULL or 4-byte aligned");
  if (sym_sum && !out) return refuse(fn, "", "out", "non-null where sym_sum is given (the finish launch forms the symmetry loss)");
  if (M < 1 || M > 0x7FFFFFFF) return refuse(fn, "", "M", "in [1, 2^31)");
  if (A < 1 || A > MAX_A) return refuse(fn, "", "A", "in [1, 16]");
  // (the library is built with -ffinite-math-only, which lets the compiler take a float ARGUMENT for finite: the value is read back
  // through a volatile, and a NaN or an infinity is told by its exponent bits)
  volatile float coeff_held = mirror_coeff;
  const float coeff_seen = coeff_held;
  uint32_t coeff_bits;
  memcpy(&coeff_bits, &coeff_seen, sizeof coeff_bits);
  if ((coeff_bits & 0x7F800000u) == 0x7F800000u) return refuse(fn, "", "mirror_coeff", "finite");
  const hipError_t e = hipMemsetAsync(acc, 0, sizeof(float) * (4 + MAX_A + 4), (hipStream_t)stream);
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  const dim3 grid((unsigned)((M + 255) / 256));
  const float inv_ma = (float)(1.0 / ((double)M * (double)A));
  const float mirror_scale = (float)((double)mirror_coeff * 2.0 / ((double)M * (double)A));
#define LT_PPO_SYM_LAUNCH(LOG, NORM, MIRROR)                                                                                                     \
  hipLaunchKernelGGL((lt_ppo_loss_sym_kernel<LOG, NORM, MIRROR>), grid, dim3(256), 0, (hipStream_t)stream, mu, stdp, value, actions, old_logp, adv, \
                     returns, old_values, old_mu, old_sigma, (const long long*)idx, (long long)M, A, clip, value_loss_coef, use_clipped_value_loss, \
                     adv_stats, (const int*)act_table, mirror_scale, dmu, dvalue, acc)
#define LT_PPO_SYM_PICK(MIRROR)                                    \
  if (std_is_log && adv_stats) LT_PPO_SYM_LAUNCH(true, true, MIRROR); \
  else if (std_is_log) LT_PPO_SYM_LAUNCH(true, false, MIRROR);        \
  else if (adv_stats) LT_PPO_SYM_LAUNCH(false, true, MIRROR);         \
  else LT_PPO_SYM_LAUNCH(false, false, MIRROR)
  if (mirror_coeff != 0.f) { LT_PPO_SYM_PICK(true); }
  else { LT_PPO_SYM_PICK(false); }
#undef LT_PPO_SYM_PICK
#undef LT_PPO_SYM_LAUNCH
  if (out)
    hipLaunchKernelGGL(lt_ppo_sym_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, stdp, A, 1.f / (float)(2 * M), 1.f / (float)M, inv_ma,
                       value_loss_coef, entropy_coef, std_is_log ? 1 : 0, mirror_coeff, out, sym_sum);
  return launch_status(fn);
}

extern "C" int lt_ppo_loss_mirror(const float* mu, const float* stdp, const float* value, const float* actions, const float* old_logp, const float* adv,
                                  const float* returns, const float* old_values, const float* old_mu, const float* old_sigma, const int64_t* idx, int64_t M,
                                  int A, float clip, float value_loss_coef, float entropy_coef, int use_clipped_value_loss, int std_is_log,
                                  const float* adv_stats, const int32_t* act_table, float mirror_coeff, float* dmu, float* dvalue, float* acc, float* out,
                                  float* sym_sum, void* stream) {
  const char* fn = "lt_ppo_loss_mirror";
  const ptr_check ptrs[] = {{"mu", mu, 4}, {"std", stdp, 4}, {"value", value, 4}, {"actions", actions, 4}, {"old_logp", old_logp, 4}, {"adv", adv, 4},
                            {"returns", returns, 4}, {"old_values", old_values, 4}, {"old_mu", old_mu, 4}, {"old_sigma", old_sigma, 4},
                            {"act_table", act_table, 4}, {"dmu", dmu, 4}, {"dvalue", dvalue, 4}, {"acc", acc, 4}};
  if (const int rc = check_ptrs(fn, "", ptrs)) return rc;
  if ((uintptr_t)idx % 8 != 0) return refuse(fn, "", "idx", "NULL or 8-byte aligned");
  if ((uintptr_t)adv_stats % 4 != 0) return refuse(fn, "", "adv_stats", "NULL or 4-byte aligned");
  if ((uintptr_t)out % 4 != 0) return refuse(fn, "", "out", "NULL or 4-byte aligned");
  if ((uintptr_t)sym_sum % 4 != 0) return refuse(fn, "", "sym_sum", "NULL or 4-byte aligned");
  if (sym_sum && !out) return refuse(fn, "", "out", "non-null where sym_sum is given (the finish launch forms the symmetry loss)");
  if (M < 1 || M > 0x7FFFFFFF) return refuse(fn, "", "M", "in [1, 2^31)");
  if (A < 1 || A > MAX_A) return refuse(fn, "", "A", "in [1, 16]");
  // (the library is built with -ffinite-math-only, which lets the compiler take a float ARGUMENT for finite: the value is read back
  // through a volatile, and a NaN or an infinity is told by its exponent bits)
  volatile float coeff_held = mirror_coeff;
  const float coeff_seen = coeff_held;
  uint32_t coeff_bits;
  memcpy(&coeff_bits, &coeff_seen, sizeof coeff_bits);
  if ((coeff_bits & 0x7F800000u) == 0x7F800000u) return refuse(fn, "", "mirror_coeff", "finite");
  const hipError_t e = hipMemsetAsync(acc, 0, sizeof(float) * (4 + MAX_A + 4), (hipStream_t)stream);
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  const dim3 grid((unsigned)((M + 255) / 256));
  const float inv_ma = (float)(1.0 / ((double)M * (double)A));
  const float mirror_scale = (float)((double)mirror_coeff * 2.0 / ((double)M * (double)A));
#define LT_PPO_MIRROR_LAUNCH(LOG, NORM, MIRROR)                                                                                                        \
  hipLaunchKernelGGL((lt_ppo_loss_mirror_kernel<LOG, NORM, MIRROR>), grid, dim3(256), 0, (hipStream_t)stream, mu, stdp, value, actions, old_logp, adv, \
                     returns, old_values, old_mu, old_sigma, (const long long*)idx, (long long)M, A, clip, value_loss_coef, use_clipped_value_loss,    \
                     adv_stats, (const int*)act_table, mirror_scale, dmu, dvalue, acc)
#define LT_PPO_MIRROR_PICK(MIRROR)                                       \
  if (std_is_log && adv_stats) LT_PPO_MIRROR_LAUNCH(true, true, MIRROR); \
  else if (std_is_log) LT_PPO_MIRROR_LAUNCH(true, false, MIRROR);        \
  else if (adv_stats) LT_PPO_MIRROR_LAUNCH(false, true, MIRROR);         \
  else LT_PPO_MIRROR_LAUNCH(false, false, MIRROR)
  if (mirror_coeff != 0.f) { LT_PPO_MIRROR_PICK(true); }
  else { LT_PPO_MIRROR_PICK(false); }
#undef LT_PPO_MIRROR_PICK
#undef LT_PPO_MIRROR_LAUNCH
  if (out)
    hipLaunchKernelGGL(lt_ppo_mirror_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, stdp, A, 1.f / (float)M, inv_ma, value_loss_coef,
                       entropy_coef, std_is_log ? 1 : 0, mirror_coeff, out, sym_sum);
  return launch_status(fn);
}
