// lt_episode_stats.hip - statistics over the finished episodes of all envs (include/lt_episode_stats.h: metric arithmetic, state and
// result layouts, the one order of the f64 sums, refusals).
//
// STEP: a thread per env, 256 per workgroup, no LDS.  The plan is read through a uniform pointer (every lane the same words: scalar
// loads); the channel loads of an all-f32 metric go out four pairs at a time (term_of); a channel load is one strided 4-byte (f32, i32), 8-byte or 1-byte load per lane, neighbouring lanes neighbouring envs - for an
// arena quad field 16 bytes apart, for the state arrays (env index last) 4 bytes apart.  The f32 running values are read and written
// every step; the f64 accumulators are touched on the done path only.  A plan without the magic word, or one written for other counts
// than the launch's, ends the launch before it touches anything.
// REDUCE: one workgroup of 256 threads; per metric each thread walks its envs in index order, then a stride-halving tree over the 256
// partials in LDS - the header's order, which tests/episode_stats_ref.py restates.
// This file is built with -ffp-contract=off and without the relaxed-math switches of the other units (build.py: PRECISE_SOURCES): a
// product and the sum behind it are two roundings, 0.0f + x is an addition, NaN compares as NaN, and the f64 division and square root
// are the correctly rounded ones.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "lt_episode_stats.h"
#include "lt_host_check.h"
#include "lt_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_FILL_BLOCKS = 2048;
constexpr uint32_t PLAN_MAGIC = 0x4C544553u;  // "LTES"
constexpr int FLAG_SQRT = 1, FLAG_INCLUDE_DONE = 2, FLAG_ALL_F32 = 4;  // PlanMetric::flags (ALL_F32: every channel the term reads is f32)
constexpr int CAUSES = LT_EPISODE_STATS_CAUSES;
constexpr int FIELDS = LT_EPISODE_STATS_FIELDS;

struct PlanChannel {
  const void* base;
  long long env_stride, offset;
  int32_t dtype, reserved;
};
struct PlanHeader {
  uint32_t magic;
  int32_t nmetrics, nenvs, reserved;
  PlanChannel dones, time_out, term_bits;
};
struct PlanMetric {
  int32_t npairs, term, reduce, flags;  // FLAG_*
  PlanChannel ch[LT_EPISODE_STATS_MAX_PAIRS][2];
};
static_assert(sizeof(PlanChannel) == 32 && sizeof(PlanHeader) == LT_EPISODE_STATS_PLAN_HEADER_BYTES &&
                  sizeof(PlanMetric) == LT_EPISODE_STATS_PLAN_METRIC_BYTES,
              "the plan's layout");

constexpr size_t plan_bytes(int m) { return LT_EPISODE_STATS_PLAN_HEADER_BYTES + (size_t)LT_EPISODE_STATS_PLAN_METRIC_BYTES * m; }
constexpr size_t MAX_PLAN_BYTES = plan_bytes(LT_EPISODE_STATS_MAX_METRICS);
constexpr size_t state_bytes(int m, long long n) { return (size_t)n * (size_t)(8 * FIELDS * (m + 1) + 8 * m + 4 + 4 * CAUSES + 1); }
constexpr size_t result_bytes(int m) { return (size_t)8 * FIELDS * (m + 1) + 8 * CAUSES; }

// the state's arrays (the header's order)
struct State {
  double* fin;        // [M + 1][5][N]
  float* run;         // [M][N]
  int* count;         // [M][N]
  int* steps;         // [N]
  int* causes;        // [18][N]
  unsigned char* armed;  // [N]
};
__host__ __device__ __forceinline__ State state_of(void* p, int m, long long n) {
  State s;
  s.fin = (double*)p;
  s.run = (float*)(s.fin + (long long)(m + 1) * FIELDS * n);
  s.count = (int*)(s.run + (long long)m * n);
  s.steps = s.count + (long long)m * n;
  s.causes = s.steps + n;
  s.armed = (unsigned char*)(s.causes + (long long)CAUSES * n);
  return s;
}

__device__ __forceinline__ float load_as_float(const PlanChannel& c, long long env) {
  const long long i = env * c.env_stride + c.offset;
  switch (c.dtype) {
    case 0: return ((const float*)c.base)[i];
    case 1: return (float)((const long long*)c.base)[i];
    case 2: return (float)((const unsigned char*)c.base)[i];
    default: return (float)((const int*)c.base)[i];
  }
}

__device__ __forceinline__ float g_of(int term, float a, float b) {
  switch (term) {
    case LT_EPISODE_STATS_VALUE: return a;
    case LT_EPISODE_STATS_ABS: return fabsf(a);
    case LT_EPISODE_STATS_SQUARE: return a * a;
    case LT_EPISODE_STATS_DIFF_SQUARE: {
      const float d = a - b;
      return d * d;
    }
    default: return fabsf(a * b);
  }
}

// (a channel lies in device memory: the global address space, so the load is a global one that only the vector-memory counter waits for)
__device__ __forceinline__ float load_f32(const PlanChannel& c, long long env) {
  return ((const __attribute__((address_space(1))) float*)c.base)[env * c.env_stride + c.offset];
}

// the per-step term of metric pm for env e.  A metric whose channels are all f32 (FLAG_ALL_F32, set by the host) loads BATCH pairs at a
// time: the loads of a batch do not depend on each other and there is no branch between them, so they are in flight together (the
// generic loop below waits for every load before it issues the next: a dozen memory latencies in a row).  A batch's slots behind the
// last pair load that pair again (the address is valid, the value is not used); the sum runs over the pairs in order either way.
constexpr int BATCH = 4;
__device__ __forceinline__ float term_of(const PlanMetric* pm, long long e) {
  float s = 0.0f;
  const int term = pm->term, npairs = pm->npairs;
  const bool two = term == LT_EPISODE_STATS_DIFF_SQUARE || term == LT_EPISODE_STATS_ABS_PRODUCT;
  if (pm->flags & FLAG_ALL_F32) {
    for (int p0 = 0; p0 < npairs; p0 += BATCH) {
      float a[BATCH], b[BATCH];
      if (two) {
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
          const int p = p0 + k < npairs ? p0 + k : npairs - 1;
          a[k] = load_f32(pm->ch[p][0], e);
          b[k] = load_f32(pm->ch[p][1], e);
        }
      } else {
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
          const int p = p0 + k < npairs ? p0 + k : npairs - 1;
          a[k] = load_f32(pm->ch[p][0], e);
          b[k] = 0.0f;
        }
      }
#pragma unroll
      for (int k = 0; k < BATCH; ++k)
        if (p0 + k < npairs) s = s + g_of(term, a[k], b[k]);
    }
    return s;
  }
  for (int p = 0; p < npairs; ++p) {
    const float a = load_as_float(pm->ch[p][0], e);
    const float b = two ? load_as_float(pm->ch[p][1], e) : 0.0f;
    s = s + g_of(term, a, b);
  }
  return s;
}

__device__ __forceinline__ void fold(double* fin, long long n, long long e, int m, double v) {
  double* const f = fin + (long long)m * FIELDS * n + e;
  const double cnt = f[LT_EPISODE_STATS_F_N * n];
  const double lo = f[LT_EPISODE_STATS_F_MIN * n], hi = f[LT_EPISODE_STATS_F_MAX * n];
  f[LT_EPISODE_STATS_F_MIN * n] = cnt == 0.0 ? v : (v < lo ? v : lo);
  f[LT_EPISODE_STATS_F_MAX * n] = cnt == 0.0 ? v : (v > hi ? v : hi);
  f[LT_EPISODE_STATS_F_N * n] = cnt + 1.0;
  f[LT_EPISODE_STATS_F_SUM * n] = f[LT_EPISODE_STATS_F_SUM * n] + v;
  const double sq = v * v;
  f[LT_EPISODE_STATS_F_SUMSQ * n] = f[LT_EPISODE_STATS_F_SUMSQ * n] + sq;
}

__global__ __launch_bounds__(THREADS) void lt_episode_stats_step_kernel(const char* __restrict__ plan, void* state, int nmetrics, int nenvs) {
  const PlanHeader* const h = (const PlanHeader*)plan;
  if (h->magic != PLAN_MAGIC || h->nmetrics != nmetrics || h->nenvs != nenvs) return;  // (uniform)
  const long long n = nenvs;
  const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= n) return;
  const State st = state_of(state, nmetrics, n);
  const PlanMetric* const metrics = (const PlanMetric*)(plan + LT_EPISODE_STATS_PLAN_HEADER_BYTES);
  const bool done = load_as_float(h->dones, e) != 0.0f;
  const bool armed = st.armed[e] != 0;
  const int steps = st.steps[e] + 1;
  for (int m = 0; m < nmetrics; ++m) {
    const PlanMetric* const pm = metrics + m;
    const int reduce = pm->reduce, flags = pm->flags;
    const long long at = (long long)m * n + e;
    if (reduce == LT_EPISODE_STATS_LAST) {
      if (done && armed) {
        double v = (double)term_of(pm, e);
        if (flags & FLAG_SQRT) v = sqrt(v);
        fold(st.fin, n, e, m, v);
      }
      continue;
    }
    float run = st.run[at];
    int count = st.count[at];
    if (!done || (flags & FLAG_INCLUDE_DONE)) {
      const float s = term_of(pm, e);
      if (reduce == LT_EPISODE_STATS_MAX)
        run = count == 0 ? s : (s > run ? s : run);
      else
        run = run + s;
      count += 1;
    }
    if (done) {
      if (armed && count > 0) {
        double v = (double)run;
        if (reduce == LT_EPISODE_STATS_MEAN) v = v / (double)count;
        if (flags & FLAG_SQRT) v = sqrt(v);
        fold(st.fin, n, e, m, v);
      }
      run = 0.0f;
      count = 0;
    }
    st.run[at] = run;
    st.count[at] = count;
  }
  if (!done) {
    st.steps[e] = steps;
    return;
  }
  st.steps[e] = 0;
  if (!armed) {
    st.armed[e] = 1;
    return;
  }
  fold(st.fin, n, e, nmetrics, (double)steps);
  const int bits = (int)load_as_float(h->term_bits, e) & 0xFFFF;
  for (int b = 0; b < 16; ++b)
    if ((bits >> b) & 1) st.causes[(long long)b * n + e] += 1;
  if (load_as_float(h->time_out, e) != 0.0f) st.causes[16 * n + e] += 1;
  st.causes[17 * n + e] += 1;
}

// dwords [0, ndwords) of p become 0, bytes [0, nbytes) of tail become `value`
__global__ __launch_bounds__(THREADS) void lt_episode_stats_fill_kernel(uint32_t* p, long long ndwords, uint32_t* p2, long long ndwords2,
                                                                      unsigned char* tail, long long nbytes, unsigned char value) {
  const long long stride = (long long)gridDim.x * THREADS;
  const long long first = (long long)blockIdx.x * THREADS + threadIdx.x;
  for (long long i = first; i < ndwords; i += stride) p[i] = 0u;
  for (long long i = first; i < ndwords2; i += stride) p2[i] = 0u;
  for (long long i = first; i < nbytes; i += stride) tail[i] = value;
}

__global__ __launch_bounds__(THREADS) void lt_episode_stats_reduce_kernel(const void* state, int nmetrics, int nenvs, void* result) {
  __shared__ double s_val[FIELDS][THREADS];
  __shared__ long long s_int[THREADS];
  const long long n = nenvs;
  const int t = threadIdx.x;
  const State st = state_of(const_cast<void*>(state), nmetrics, n);
  double* const totals = (double*)result;
  long long* const causes = (long long*)(totals + (nmetrics + 1) * FIELDS);
  for (int m = 0; m <= nmetrics; ++m) {
    const double* const f = st.fin + (long long)m * FIELDS * n;
    double cnt = 0.0, sum = 0.0, sumsq = 0.0, lo = 0.0, hi = 0.0;
    for (long long e = t; e < n; e += THREADS) {
      const double c = f[LT_EPISODE_STATS_F_N * n + e];
      if (c != 0.0) {
        const double b_lo = f[LT_EPISODE_STATS_F_MIN * n + e], b_hi = f[LT_EPISODE_STATS_F_MAX * n + e];
        lo = cnt == 0.0 ? b_lo : (b_lo < lo ? b_lo : lo);
        hi = cnt == 0.0 ? b_hi : (b_hi > hi ? b_hi : hi);
      }
      cnt = cnt + c;
      sum = sum + f[LT_EPISODE_STATS_F_SUM * n + e];
      sumsq = sumsq + f[LT_EPISODE_STATS_F_SUMSQ * n + e];
    }
    s_val[0][t] = cnt; s_val[1][t] = sum; s_val[2][t] = sumsq; s_val[3][t] = lo; s_val[4][t] = hi;
    __syncthreads();
    for (int stride = THREADS / 2; stride >= 1; stride >>= 1) {
      if (t < stride) {
        const double a_n = s_val[0][t], b_n = s_val[0][t + stride];
        if (b_n != 0.0) {
          const double b_lo = s_val[3][t + stride], b_hi = s_val[4][t + stride];
          s_val[3][t] = a_n == 0.0 ? b_lo : (b_lo < s_val[3][t] ? b_lo : s_val[3][t]);
          s_val[4][t] = a_n == 0.0 ? b_hi : (b_hi > s_val[4][t] ? b_hi : s_val[4][t]);
        }
        s_val[0][t] = a_n + b_n;
        s_val[1][t] = s_val[1][t] + s_val[1][t + stride];
        s_val[2][t] = s_val[2][t] + s_val[2][t + stride];
      }
      __syncthreads();
    }
    if (t < FIELDS) totals[m * FIELDS + t] = s_val[t][0];
    __syncthreads();  // before the next metric's partials overwrite these
  }
  for (int c = 0; c < CAUSES; ++c) {
    long long acc = 0;
    for (long long e = t; e < n; e += THREADS) acc += st.causes[(long long)c * n + e];
    s_int[t] = acc;
    __syncthreads();
    for (int stride = THREADS / 2; stride >= 1; stride >>= 1) {
      if (t < stride) s_int[t] += s_int[t + stride];
      __syncthreads();
    }
    if (t == 0) causes[c] = s_int[0];
    __syncthreads();
  }
}

int check_range(const char* fn, const char* who, const char* field, long long v, long long lo, long long hi) {
  if (v >= lo && v <= hi) return LT_OK;
  char what[96];
  snprintf(what, sizeof what, "in %lld ... %lld", lo, hi);
  return refuse(fn, who, field, what);
}

int check_counts(const char* fn, int nmetrics, long long nenvs) {
  if (const int rc = check_range(fn, "", "nmetrics", nmetrics, 1, LT_EPISODE_STATS_MAX_METRICS)) return rc;
  return check_range(fn, "", "nenvs", nenvs, 1, LT_EPISODE_STATS_MAX_ENVS);
}

int check_channel(const char* fn, const char* who, const lt_telemetry_channel& ch) {
  static const int elem[4] = {4, 8, 1, 4};
  if (ch.dtype < 0 || ch.dtype > 3) return refuse(fn, who, "dtype", "in 0 ... 3 (f32, i64, u8, i32)");
  if (!ch.base || (uintptr_t)ch.base % elem[ch.dtype] != 0) return refuse(fn, who, "base", "non-null and aligned to its element");
  if (ch.env_stride < 0) return refuse(fn, who, "env_stride", "non-negative");
  if (ch.offset < 0) return refuse(fn, who, "offset", "non-negative");
  return LT_OK;
}

int check_ptr8(const char* fn, const char* name, const void* p) {
  if (!p || (uintptr_t)p % 8 != 0) return refuse(fn, "", name, "non-null and 8-byte aligned");
  return LT_OK;
}

int check_step(const char* fn, const void* device_plan, const void* state, int nmetrics, int nenvs) {
  if (const int rc = check_counts(fn, nmetrics, nenvs)) return rc;
  if (const int rc = check_ptr(fn, "", {"device_plan", device_plan, 16})) return rc;
  return check_ptr(fn, "", {"state", state, 16});
}

int check_reduce(const char* fn, const void* state, int nmetrics, int nenvs, const void* result) {
  if (const int rc = check_counts(fn, nmetrics, nenvs)) return rc;
  if (const int rc = check_ptr(fn, "", {"state", state, 16})) return rc;
  return check_ptr8(fn, "result", result);
}

PlanChannel plan_channel(const lt_telemetry_channel& c) { return {c.base, c.env_stride, c.offset, c.dtype, 0}; }

unsigned fill_blocks(long long items) {
  const long long blocks = (items + THREADS - 1) / THREADS;
  return (unsigned)(blocks < 1 ? 1 : blocks > MAX_FILL_BLOCKS ? MAX_FILL_BLOCKS : blocks);
}

}  // namespace

extern "C" {

int lt_episode_stats_plan_bytes(int nmetrics, size_t* bytes) {
  const char* fn = "lt_episode_stats_plan_bytes";
  if (const int rc = check_range(fn, "", "nmetrics", nmetrics, 1, LT_EPISODE_STATS_MAX_METRICS)) return rc;
  if (!bytes) return refuse(fn, "", "bytes", "non-null");
  *bytes = plan_bytes(nmetrics);
  return LT_OK;
}

int lt_episode_stats_state_bytes(int nmetrics, int nenvs, size_t* bytes) {
  const char* fn = "lt_episode_stats_state_bytes";
  if (const int rc = check_counts(fn, nmetrics, nenvs)) return rc;
  if (!bytes) return refuse(fn, "", "bytes", "non-null");
  *bytes = state_bytes(nmetrics, nenvs);
  return LT_OK;
}

int lt_episode_stats_result_bytes(int nmetrics, size_t* bytes) {
  const char* fn = "lt_episode_stats_result_bytes";
  if (const int rc = check_range(fn, "", "nmetrics", nmetrics, 1, LT_EPISODE_STATS_MAX_METRICS)) return rc;
  if (!bytes) return refuse(fn, "", "bytes", "non-null");
  *bytes = result_bytes(nmetrics);
  return LT_OK;
}

int lt_episode_stats_plan_write(const lt_episode_stats_metric* metrics, int nmetrics, const lt_telemetry_channel* dones,
                                const lt_telemetry_channel* time_out, const lt_telemetry_channel* term_bits, int nenvs, void* device_plan,
                                size_t bytes, void* stream) {
  const char* fn = "lt_episode_stats_plan_write";
  if (!metrics) return refuse(fn, "", "metrics", "non-null");
  if (!dones) return refuse(fn, "", "dones", "non-null");
  if (!time_out) return refuse(fn, "", "time_out", "non-null");
  if (!term_bits) return refuse(fn, "", "term_bits", "non-null");
  if (const int rc = check_counts(fn, nmetrics, nenvs)) return rc;
  char who[48];
  for (int m = 0; m < nmetrics; ++m) {
    const lt_episode_stats_metric& mt = metrics[m];
    snprintf(who, sizeof who, "metrics[%d].", m);
    if (const int rc = check_range(fn, who, "npairs", mt.npairs, 1, LT_EPISODE_STATS_MAX_PAIRS)) return rc;
    if (mt.term < 0 || mt.term > LT_EPISODE_STATS_ABS_PRODUCT)
      return refuse(fn, who, "term", "in 0 ... 4 (VALUE, ABS, SQUARE, DIFF_SQUARE, ABS_PRODUCT)");
    if (mt.reduce < 0 || mt.reduce > LT_EPISODE_STATS_LAST) return refuse(fn, who, "reduce", "in 0 ... 3 (MEAN, SUM, MAX, LAST)");
    if (const int rc = check_range(fn, who, "take_sqrt", mt.take_sqrt, 0, 1)) return rc;
    if (const int rc = check_range(fn, who, "include_done_step", mt.include_done_step, 0, 1)) return rc;
    const bool two = mt.term == LT_EPISODE_STATS_DIFF_SQUARE || mt.term == LT_EPISODE_STATS_ABS_PRODUCT;
    for (int p = 0; p < mt.npairs; ++p) {
      snprintf(who, sizeof who, "metrics[%d].pairs[%d].a.", m, p);
      if (const int rc = check_channel(fn, who, mt.pairs[p].a)) return rc;
      if (!two) continue;
      snprintf(who, sizeof who, "metrics[%d].pairs[%d].b.", m, p);
      if (const int rc = check_channel(fn, who, mt.pairs[p].b)) return rc;  // (DIFF_SQUARE and ABS_PRODUCT read b: it may not be absent)
    }
  }
  if (const int rc = check_channel(fn, "dones.", *dones)) return rc;
  if (const int rc = check_channel(fn, "time_out.", *time_out)) return rc;
  if (const int rc = check_channel(fn, "term_bits.", *term_bits)) return rc;
  if (const int rc = check_ptr(fn, "", {"device_plan", device_plan, 16})) return rc;
  const size_t need = plan_bytes(nmetrics);
  if (bytes < need) return refuse(fn, "", "bytes", "at least lt_episode_stats_plan_bytes(nmetrics)");
  // the staging copy: the runtime has read a pageable source when hipMemcpyAsync returns; one per thread
  alignas(16) static thread_local char staging[MAX_PLAN_BYTES];
  memset(staging, 0, need);
  const PlanHeader h = {PLAN_MAGIC, nmetrics, nenvs, 0, plan_channel(*dones), plan_channel(*time_out), plan_channel(*term_bits)};
  memcpy(staging, &h, sizeof h);
  PlanMetric* const pm = (PlanMetric*)(staging + LT_EPISODE_STATS_PLAN_HEADER_BYTES);
  for (int m = 0; m < nmetrics; ++m) {
    const lt_episode_stats_metric& mt = metrics[m];
    const bool two = mt.term == LT_EPISODE_STATS_DIFF_SQUARE || mt.term == LT_EPISODE_STATS_ABS_PRODUCT;
    pm[m].npairs = mt.npairs; pm[m].term = mt.term; pm[m].reduce = mt.reduce;
    bool all_f32 = true;
    for (int p = 0; p < mt.npairs; ++p) {
      pm[m].ch[p][0] = plan_channel(mt.pairs[p].a);
      if (two) pm[m].ch[p][1] = plan_channel(mt.pairs[p].b);
      all_f32 = all_f32 && mt.pairs[p].a.dtype == 0 && (!two || mt.pairs[p].b.dtype == 0);
    }
    pm[m].flags = (mt.take_sqrt ? FLAG_SQRT : 0) | (mt.include_done_step ? FLAG_INCLUDE_DONE : 0) | (all_f32 ? FLAG_ALL_F32 : 0);
  }
  const hipError_t e = hipMemcpyAsync(device_plan, staging, need, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", fn, hipGetErrorString(e));
    lt_set_error(msg);
    return LT_EHIP;
  }
  return LT_OK;
}

int lt_episode_stats_begin(void* state, int nmetrics, int nenvs, int skip_running, void* stream) {
  const char* fn = "lt_episode_stats_begin";
  if (const int rc = check_counts(fn, nmetrics, nenvs)) return rc;
  if (const int rc = check_ptr(fn, "", {"state", state, 16})) return rc;
  if (const int rc = check_range(fn, "", "skip_running", skip_running, 0, 1)) return rc;
  const State st = state_of(state, nmetrics, nenvs);
  const long long ndwords = ((char*)st.armed - (char*)state) / 4;  // everything in front of `armed` is whole dwords
  hipLaunchKernelGGL(lt_episode_stats_fill_kernel, dim3(fill_blocks(ndwords)), dim3(THREADS), 0, (hipStream_t)stream, (uint32_t*)state, ndwords,
                     (uint32_t*)nullptr, 0ll, st.armed, (long long)nenvs, (unsigned char)(skip_running ? 0 : 1));
  return launch_status(fn);
}

int lt_episode_stats_restart_running(void* state, int nmetrics, int nenvs, int skip_running, void* stream) {
  const char* fn = "lt_episode_stats_restart_running";
  if (const int rc = check_counts(fn, nmetrics, nenvs)) return rc;
  if (const int rc = check_ptr(fn, "", {"state", state, 16})) return rc;
  if (const int rc = check_range(fn, "", "skip_running", skip_running, 0, 1)) return rc;
  const State st = state_of(state, nmetrics, nenvs);
  const long long ndwords = (long long)(2 * nmetrics + 1) * nenvs;  // run, count and steps lie one behind the other
  hipLaunchKernelGGL(lt_episode_stats_fill_kernel, dim3(fill_blocks(ndwords)), dim3(THREADS), 0, (hipStream_t)stream, (uint32_t*)st.run, ndwords,
                     (uint32_t*)nullptr, 0ll, st.armed, (long long)nenvs, (unsigned char)(skip_running ? 0 : 1));
  return launch_status(fn);
}

int lt_episode_stats_step_launches(const void* device_plan, const void* state, int nmetrics, int nenvs) {
  if (const int rc = check_step("lt_episode_stats_step_launches", device_plan, state, nmetrics, nenvs)) return rc;
  return 1;
}

int lt_episode_stats_step(const void* device_plan, void* state, int nmetrics, int nenvs, void* stream) {
  const char* fn = "lt_episode_stats_step";
  if (const int rc = check_step(fn, device_plan, state, nmetrics, nenvs)) return rc;
  const unsigned blocks = (unsigned)((nenvs + THREADS - 1) / THREADS);  // <= 65535 for nenvs <= LT_EPISODE_STATS_MAX_ENVS
  hipLaunchKernelGGL(lt_episode_stats_step_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, (const char*)device_plan, state, nmetrics,
                     nenvs);
  return launch_status(fn);
}

int lt_episode_stats_clear_finished(void* state, int nmetrics, int nenvs, void* stream) {
  const char* fn = "lt_episode_stats_clear_finished";
  if (const int rc = check_counts(fn, nmetrics, nenvs)) return rc;
  if (const int rc = check_ptr(fn, "", {"state", state, 16})) return rc;
  const State st = state_of(state, nmetrics, nenvs);
  const long long fin_dwords = (long long)(nmetrics + 1) * FIELDS * nenvs * 2, cause_dwords = (long long)CAUSES * nenvs;
  hipLaunchKernelGGL(lt_episode_stats_fill_kernel, dim3(fill_blocks(fin_dwords)), dim3(THREADS), 0, (hipStream_t)stream, (uint32_t*)st.fin, fin_dwords,
                     (uint32_t*)st.causes, cause_dwords, (unsigned char*)nullptr, 0ll, (unsigned char)0);
  return launch_status(fn);
}

int lt_episode_stats_reduce_launches(const void* state, int nmetrics, int nenvs, const void* result) {
  if (const int rc = check_reduce("lt_episode_stats_reduce_launches", state, nmetrics, nenvs, result)) return rc;
  return 1;
}

int lt_episode_stats_reduce(const void* state, int nmetrics, int nenvs, void* result, void* stream) {
  const char* fn = "lt_episode_stats_reduce";
  if (const int rc = check_reduce(fn, state, nmetrics, nenvs, result)) return rc;
  hipLaunchKernelGGL(lt_episode_stats_reduce_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, state, nmetrics, nenvs, result);
  return launch_status(fn);
}

}  // extern "C"
