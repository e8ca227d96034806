// lt_telemetry.hip - the telemetry ring and its strip charts (include/lt_telemetry.h: channel, plan, ring, chart arithmetic, refusals).
//
// RECORD: one workgroup of 256 threads.  Every thread reads the plan's header and head[0], thread i moves the scalars i, i + 256, ...
// of the record's nenvs * nchannels (<= 2048) - neighbouring threads write neighbouring floats of the slot -, and behind the
// workgroup barrier thread 0 advances the head.  A plan without the magic word (memory lt_telemetry_plan never wrote) ends the launch
// before it touches anything; the slot index is formed unsigned, so whatever head[0] holds the slot lies inside the ring.
// CHART: one thread per panel pixel, a workgroup is a 64 x 4 pixel tile of the panel rectangle (a wave is 64 neighbouring pixels of one
// image row: one coalesced dword load of the frame and one coalesced dword store), blockIdx.z is the view.  A thread of a plot reads,
// per series, the sample of its column and of the column left of it (neighbouring lanes read records one slot apart), so at most 8
// floats.  The value -> row step is the chart's ONE float operation, k * v; whether a sample is drawn is decided on the product's
// bits, which the build's -ffinite-math-only cannot fold away.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "lt_host_check.h"
#include "lt_internal.h"
#include "lt_telemetry.h"

namespace {

constexpr int RECORD_THREADS = 256;
constexpr int TILE_W = 64, TILE_H = 4;
constexpr uint32_t PLAN_MAGIC = 0x4C54544Du;  // "LTTM"
constexpr uint32_t SKIP_FROM = 0x4E800000u;   // the bits of 2^30f: |p| from here on, +-inf and every NaN are not drawn
static_assert(LT_CHART_VIEWS_PER_LAUNCH == LT_RENDER_VIEWS_PER_LAUNCH, "the renderer's per-launch limit");

struct PlanHeader {
  uint32_t magic;
  int32_t nchannels, nenvs, capacity;
};
struct PlanChannel {
  const void* base;
  long long env_stride, offset;
  int32_t dtype, reserved;
};
static_assert(sizeof(PlanHeader) == LT_TELEMETRY_PLAN_HEADER_BYTES && sizeof(PlanChannel) == LT_TELEMETRY_PLAN_CHANNEL_BYTES, "the plan's layout");

constexpr size_t env_bytes(int nenvs) { return (size_t)((nenvs + 3) / 4) * 16; }
constexpr size_t plan_bytes(int nchannels, int nenvs) {
  return LT_TELEMETRY_PLAN_HEADER_BYTES + env_bytes(nenvs) + (size_t)LT_TELEMETRY_PLAN_CHANNEL_BYTES * nchannels;
}
constexpr size_t MAX_PLAN_BYTES = plan_bytes(LT_TELEMETRY_MAX_CHANNELS, LT_TELEMETRY_MAX_ENVS);

__device__ __forceinline__ float load_as_float(const void* base, long long i, int dtype) {
  switch (dtype) {
    case 0: return ((const float*)base)[i];
    case 1: return (float)((const long long*)base)[i];
    case 2: return (float)((const unsigned char*)base)[i];
    default: return (float)((const int*)base)[i];
  }
}

__global__ __launch_bounds__(RECORD_THREADS) void lt_telemetry_record_kernel(const char* __restrict__ plan, float* __restrict__ ring,
                                                                            long long* __restrict__ head) {
  const PlanHeader h = *(const PlanHeader*)plan;
  if (h.magic != PLAN_MAGIC || h.nchannels < 1 || h.nchannels > LT_TELEMETRY_MAX_CHANNELS || h.nenvs < 1 || h.nenvs > LT_TELEMETRY_MAX_ENVS ||
      h.capacity < 1 || h.capacity > LT_TELEMETRY_MAX_CAPACITY)
    return;  // (uniform: every thread reads the same header)
  const int32_t* const env_ids = (const int32_t*)(plan + LT_TELEMETRY_PLAN_HEADER_BYTES);
  const PlanChannel* const ch = (const PlanChannel*)(plan + LT_TELEMETRY_PLAN_HEADER_BYTES + env_bytes(h.nenvs));
  const long long count = head[0];
  const long long slot = (long long)((unsigned long long)count % (unsigned long long)h.capacity);
  const int per_record = h.nenvs * h.nchannels;
  float* const dst = ring + slot * per_record;
  for (int i = threadIdx.x; i < per_record; i += RECORD_THREADS) {
    const int e = i / h.nchannels, c = i - e * h.nchannels;
    const PlanChannel s = ch[c];
    dst[i] = load_as_float(s.base, (long long)env_ids[e] * s.env_stride + s.offset, s.dtype);
  }
  __syncthreads();  // every thread has read head[0] and written its part of the slot
  if (threadIdx.x == 0) {
    head[0] = count + 1;
    head[1] = (long long)((unsigned long long)(count + 1) % (unsigned long long)h.capacity);
  }
}

struct ChartArgs {
  const float* ring;
  const long long* head;
  uint32_t* rgba;
  int nenvs, nchannels, capacity;
  int nplots, pw, ph, gap, x0, y0, opacity;
  int cw, chh;  // the panel's size
  int width, height;
  int nseries[LT_CHART_MAX_PLOTS];
  int channels[LT_CHART_MAX_PLOTS][LT_CHART_MAX_SERIES];
  float k[LT_CHART_MAX_PLOTS];
  int y_zero[LT_CHART_MAX_PLOTS];
  int slot[LT_CHART_VIEWS_PER_LAUNCH];
};

__device__ __forceinline__ uint32_t series_colour(int s) {
  return s == 0 ? (uint32_t)LT_CHART_COLOR_SERIES_0 : s == 1 ? (uint32_t)LT_CHART_COLOR_SERIES_1 : s == 2 ? (uint32_t)LT_CHART_COLOR_SERIES_2
                                                                                                         : (uint32_t)LT_CHART_COLOR_SERIES_3;
}

// the row of value v; false for a sample that is not drawn
__device__ __forceinline__ bool value_row(float v, float k, int y_zero, int ph, int* row) {
  const float p = k * v;  // the one float operation
  if ((__float_as_uint(p) & 0x7fffffffu) >= SKIP_FROM) return false;
  const int r = y_zero - (int)rintf(p);  // |y_zero| <= 2^30 and |rintf(p)| < 2^30: no overflow
  *row = r < 0 ? 0 : r > ph - 1 ? ph - 1 : r;
  return true;
}

__global__ __launch_bounds__(TILE_W* TILE_H) void lt_telemetry_chart_kernel(const ChartArgs a) {
  const int px = blockIdx.x * TILE_W + (threadIdx.x & (TILE_W - 1)), py = blockIdx.y * TILE_H + (threadIdx.x >> 6);
  if (px >= a.cw || py >= a.chh) return;
  const int view = blockIdx.z;
  uint32_t p;
  if (px == 0 || py == 0 || px == a.cw - 1 || py == a.chh - 1) {
    p = LT_CHART_COLOR_FRAME;
  } else {
    p = LT_CHART_COLOR_GAP;
    const int x = px - 1, iy = py - 1;
    const int plot = iy / (a.ph + a.gap), y = iy - plot * (a.ph + a.gap);  // plot < nplots: iy < chh - 2
    if (y < a.ph) {
      p = y == a.y_zero[plot] ? (uint32_t)LT_CHART_COLOR_ZERO : (uint32_t)LT_CHART_COLOR_BG;
      const long long rec = a.head[0] - a.pw + x;
      if (rec >= 0) {
        const long long per_record = (long long)a.nenvs * a.nchannels;
        const float* const cur = a.ring + (long long)((unsigned long long)rec % (unsigned long long)a.capacity) * per_record + (long long)a.slot[view] * a.nchannels;
        const bool has_left = x > 0 && rec > 0;
        const float* const left = a.ring + (long long)((unsigned long long)(has_left ? rec - 1 : rec) % (unsigned long long)a.capacity) * per_record +
                                  (long long)a.slot[view] * a.nchannels;
        const float k = a.k[plot];
        const int y_zero = a.y_zero[plot];
        for (int s = 0; s < a.nseries[plot]; ++s) {
          const int c = a.channels[plot][s];
          int r1, r0;
          if (!value_row(cur[c], k, y_zero, a.ph, &r1)) continue;
          if (!has_left || !value_row(left[c], k, y_zero, a.ph, &r0)) r0 = r1;
          const int lo = r0 < r1 ? r0 : r1, hi = r0 < r1 ? r1 : r0;
          if (y >= lo && y <= hi) p = series_colour(s);
        }
      }
    }
  }
  uint32_t* const dst = a.rgba + ((long long)view * a.height + (a.y0 + py)) * a.width + (a.x0 + px);
  const uint32_t f = *dst, op = (uint32_t)a.opacity;
  uint32_t out = 255u << 24;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t pb = (p >> (8 * k)) & 255u, fb = (f >> (8 * k)) & 255u;
    out |= ((pb * op + fb * (255u - op) + 127u) / 255u) << (8 * k);
  }
  *dst = out;
}

int check_range(const char* fn, const char* who, const char* field, long long v, long long lo, long long hi) {
  if (v >= lo && v <= hi) return LT_OK;
  char what[96];
  snprintf(what, sizeof what, "in %lld ... %lld", lo, hi);
  return refuse(fn, who, field, what);
}

int check_ptr8(const char* fn, const char* name, const void* p) {
  if (!p || (uintptr_t)p % 8 != 0) return refuse(fn, "", name, "non-null and 8-byte aligned");
  return LT_OK;
}

int check_counts(const char* fn, int nchannels, int nenvs) {
  if (const int rc = check_range(fn, "", "nchannels", nchannels, 1, LT_TELEMETRY_MAX_CHANNELS)) return rc;
  return check_range(fn, "", "nenvs", nenvs, 1, LT_TELEMETRY_MAX_ENVS);
}

int check_record(const char* fn, const void* device_plan, const float* ring, const int64_t* head) {
  if (const int rc = check_ptr(fn, "", {"device_plan", device_plan, 16})) return rc;
  if (const int rc = check_ptr(fn, "", {"ring", ring, 4})) return rc;
  return check_ptr8(fn, "head", head);
}

// the refusals that decide the panel's size; *cw, *chh on LT_OK
int chart_shape(const char* fn, const lt_chart_desc* d, int* cw, int* chh) {
  if (!d) return refuse(fn, "", "desc", "non-null");
  if (const int rc = check_range(fn, "desc.", "nplots", d->nplots, 1, LT_CHART_MAX_PLOTS)) return rc;
  if (const int rc = check_range(fn, "desc.", "pw", d->pw, LT_CHART_MIN_PLOT, LT_CHART_MAX_PLOT_WIDTH)) return rc;
  if (const int rc = check_range(fn, "desc.", "ph", d->ph, LT_CHART_MIN_PLOT, LT_CHART_MAX_PLOT_HEIGHT)) return rc;
  if (const int rc = check_range(fn, "desc.", "gap", d->gap, 0, LT_CHART_MAX_GAP)) return rc;
  *cw = 2 + d->pw;
  *chh = 2 + d->nplots * d->ph + (d->nplots - 1) * d->gap;  // <= 2 + 4 * 256 + 3 * 16
  return LT_OK;
}

// every refusal of a draw but those of the pointers, the frame and the slots
int chart_check(const char* fn, const lt_chart_desc* d, int nenvs, int nchannels, int64_t capacity, int nviews, int* cw, int* chh) {
  if (const int rc = chart_shape(fn, d, cw, chh)) return rc;
  if (const int rc = check_range(fn, "desc.", "opacity", d->opacity, 0, 255)) return rc;
  if (const int rc = check_counts(fn, nchannels, nenvs)) return rc;
  if (const int rc = check_range(fn, "", "capacity", capacity, 1, LT_TELEMETRY_MAX_CAPACITY)) return rc;
  if (d->pw > capacity) return refuse(fn, "desc.", "pw", "at most capacity (a plot shows the newest pw records, and the ring holds capacity)");
  for (int p = 0; p < d->nplots; ++p) {
    char who[32];
    snprintf(who, sizeof who, "desc.plots[%d].", p);
    const lt_chart_plot& plot = d->plots[p];
    if (const int rc = check_range(fn, who, "nseries", plot.nseries, 1, LT_CHART_MAX_SERIES)) return rc;
    for (int s = 0; s < plot.nseries; ++s)
      if (plot.channels[s] < 0 || plot.channels[s] >= nchannels) return refuse(fn, who, "channels", "in 0 ... nchannels - 1 for every series");
    uint32_t kbits;
    memcpy(&kbits, &plot.k, sizeof kbits);  // (on the bits: the build's -ffinite-math-only)
    if ((kbits & 0x7f800000u) == 0x7f800000u) return refuse(fn, who, "k", "finite");
    if (const int rc = check_range(fn, who, "y_zero", plot.y_zero, -(long long)LT_CHART_MAX_ZERO, LT_CHART_MAX_ZERO)) return rc;
  }
  return check_range(fn, "", "nviews", nviews, 1, LT_CHART_VIEWS_PER_LAUNCH);
}

}  // namespace

extern "C" {

int lt_telemetry_plan_bytes(int nchannels, int nenvs, size_t* bytes) {
  const char* fn = "lt_telemetry_plan_bytes";
  if (const int rc = check_counts(fn, nchannels, nenvs)) return rc;
  if (!bytes) return refuse(fn, "", "bytes", "non-null");
  *bytes = plan_bytes(nchannels, nenvs);
  return LT_OK;
}

int lt_telemetry_plan(const lt_telemetry_channel* channels, int nchannels, const int32_t* env_ids, int nenvs, int64_t capacity,
                      void* device_plan, size_t bytes, void* stream) {
  const char* fn = "lt_telemetry_plan";
  if (!channels) return refuse(fn, "", "channels", "non-null");
  if (!env_ids) return refuse(fn, "", "env_ids", "non-null");
  if (const int rc = check_counts(fn, nchannels, nenvs)) return rc;
  if (const int rc = check_range(fn, "", "capacity", capacity, 1, LT_TELEMETRY_MAX_CAPACITY)) return rc;
  static const int elem[4] = {4, 8, 1, 4};
  for (int c = 0; c < nchannels; ++c) {
    char who[32];
    snprintf(who, sizeof who, "channels[%d].", c);
    const lt_telemetry_channel& ch = channels[c];
    if (ch.dtype < 0 || ch.dtype > 3) return refuse(fn, who, "dtype", "in 0 ... 3 (f32, i64, u8, i32)");
    if (!ch.base || (uintptr_t)ch.base % elem[ch.dtype] != 0) return refuse(fn, who, "base", "non-null and aligned to its element");
    if (ch.env_stride < 0) return refuse(fn, who, "env_stride", "non-negative");
    if (ch.offset < 0) return refuse(fn, who, "offset", "non-negative");
  }
  for (int e = 0; e < nenvs; ++e)
    if (env_ids[e] < 0) {
      char who[32];
      snprintf(who, sizeof who, "env_ids[%d]", e);
      return refuse(fn, "", who, "non-negative");
    }
  if (const int rc = check_ptr(fn, "", {"device_plan", device_plan, 16})) return rc;
  const size_t need = plan_bytes(nchannels, nenvs);
  if (bytes < need) return refuse(fn, "", "bytes", "at least lt_telemetry_plan_bytes(nchannels, nenvs)");
  // the staging copy: the runtime has read a pageable source when hipMemcpyAsync returns; one per thread, so that two planning threads
  // never share it
  alignas(16) static thread_local char staging[MAX_PLAN_BYTES];
  memset(staging, 0, need);
  const PlanHeader h = {PLAN_MAGIC, nchannels, nenvs, (int32_t)capacity};
  memcpy(staging, &h, sizeof h);
  memcpy(staging + LT_TELEMETRY_PLAN_HEADER_BYTES, env_ids, sizeof(int32_t) * (size_t)nenvs);
  PlanChannel* const pc = (PlanChannel*)(staging + LT_TELEMETRY_PLAN_HEADER_BYTES + env_bytes(nenvs));
  for (int c = 0; c < nchannels; ++c) pc[c] = {channels[c].base, channels[c].env_stride, channels[c].offset, channels[c].dtype, 0};
  const hipError_t e = hipMemcpyAsync(device_plan, staging, need, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", fn, hipGetErrorString(e));
    lt_set_error(msg);
    return LT_EHIP;
  }
  return LT_OK;
}

int lt_telemetry_record_launches(const void* device_plan, const float* ring, const int64_t* head) {
  if (const int rc = check_record("lt_telemetry_record_launches", device_plan, ring, head)) return rc;
  return 1;
}

int lt_telemetry_record(const void* device_plan, float* ring, int64_t* head, void* stream) {
  const char* fn = "lt_telemetry_record";
  if (const int rc = check_record(fn, device_plan, ring, head)) return rc;
  hipLaunchKernelGGL(lt_telemetry_record_kernel, dim3(1), dim3(RECORD_THREADS), 0, (hipStream_t)stream, (const char*)device_plan, ring,
                     (long long*)head);
  return launch_status(fn);
}

int lt_telemetry_chart_size(const lt_chart_desc* desc, int* width, int* height) {
  const char* fn = "lt_telemetry_chart_size";
  int cw, chh;
  if (const int rc = chart_shape(fn, desc, &cw, &chh)) return rc;
  if (!width) return refuse(fn, "", "width", "non-null");
  if (!height) return refuse(fn, "", "height", "non-null");
  *width = cw;
  *height = chh;
  return LT_OK;
}

int lt_telemetry_chart_launches(const lt_chart_desc* desc, int nenvs, int nchannels, int64_t capacity, int nviews) {
  int cw, chh;
  if (const int rc = chart_check("lt_telemetry_chart_launches", desc, nenvs, nchannels, capacity, nviews, &cw, &chh)) return rc;
  return 1;
}

int lt_telemetry_chart_draw(const lt_chart_desc* desc, const float* ring, const int64_t* head, int nenvs, int nchannels, int64_t capacity,
                            const int32_t* slots, int nviews, uint32_t* rgba, int width, int height, void* stream) {
  static_assert(sizeof(ChartArgs) <= 4096, "kernel arguments too large");
  const char* fn = "lt_telemetry_chart_draw";
  ChartArgs a = {};
  if (const int rc = chart_check(fn, desc, nenvs, nchannels, capacity, nviews, &a.cw, &a.chh)) return rc;
  if (!slots) return refuse(fn, "", "slots", "non-null");
  if (const int rc = check_ptr(fn, "", {"ring", ring, 4})) return rc;
  if (const int rc = check_ptr8(fn, "head", head)) return rc;
  if (const int rc = check_ptr(fn, "", {"rgba", rgba, 4})) return rc;
  if (const int rc = check_range(fn, "", "width", width, 1, LT_RENDER_MAX_SIZE)) return rc;
  if (const int rc = check_range(fn, "", "height", height, 1, LT_RENDER_MAX_SIZE)) return rc;
  char what[96];
  if (desc->x0 < 0 || desc->x0 > width - a.cw) {
    snprintf(what, sizeof what, "in 0 ... width - %d (the panel must lie inside the frame)", a.cw);
    return refuse(fn, "desc.", "x0", what);
  }
  if (desc->y0 < 0 || desc->y0 > height - a.chh) {
    snprintf(what, sizeof what, "in 0 ... height - %d (the panel must lie inside the frame)", a.chh);
    return refuse(fn, "desc.", "y0", what);
  }
  for (int v = 0; v < nviews; ++v) {
    if (slots[v] < 0 || slots[v] >= nenvs) {
      char who[32];
      snprintf(who, sizeof who, "slots[%d]", v);
      return refuse(fn, "", who, "in 0 ... nenvs - 1");
    }
    a.slot[v] = slots[v];
  }
  for (int p = 0; p < desc->nplots; ++p) {
    a.nseries[p] = desc->plots[p].nseries;
    for (int s = 0; s < desc->plots[p].nseries; ++s) a.channels[p][s] = desc->plots[p].channels[s];
    a.k[p] = desc->plots[p].k;
    a.y_zero[p] = desc->plots[p].y_zero;
  }
  a.ring = ring; a.head = (const long long*)head; a.rgba = rgba;
  a.nenvs = nenvs; a.nchannels = nchannels; a.capacity = (int)capacity;
  a.nplots = desc->nplots; a.pw = desc->pw; a.ph = desc->ph; a.gap = desc->gap; a.x0 = desc->x0; a.y0 = desc->y0; a.opacity = desc->opacity;
  a.width = width; a.height = height;
  const dim3 grid((unsigned)((a.cw + TILE_W - 1) / TILE_W), (unsigned)((a.chh + TILE_H - 1) / TILE_H), (unsigned)nviews);
  hipLaunchKernelGGL(lt_telemetry_chart_kernel, grid, dim3(TILE_W * TILE_H), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // extern "C"
