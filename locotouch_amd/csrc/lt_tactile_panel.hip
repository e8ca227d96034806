// lt_tactile_panel.hip - the taxel panel drawn over rendered frames (include/lt_tactile_panel.h: layout, colour arithmetic, refusals).
//
// One launch, one thread per panel pixel: a workgroup is a 64 x 4 pixel tile of the panel rectangle (a wave is 64 neighbouring pixels
// of one image row: one coalesced dword load of the frame and one coalesced dword store), blockIdx.z is the view.  A thread finds its
// signal, channel and taxel by integer division, loads that one float (neighbouring lanes share it or read its neighbours), and blends
// the colour over the frame's pixel.  Pixels outside the panel rectangle are neither read nor written.  No LDS, no atomics.
// The value -> intensity step works on the float's bits, so that the build's -ffinite-math-only cannot fold the NaN rule away: a set
// sign bit (negative values, -0.0, negative NaNs) gives 0, bits above +inf's (NaNs) give 0, bits from 1.0f's on (v >= 1, +inf) give
// 255, and what is left - 0 <= v < 1 - is the one float operation of the panel: rintf(255.0f * v).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "lt_host_check.h"
#include "lt_internal.h"
#include "lt_tactile_panel.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 4;
constexpr int GRID_COLS = 13, GRID_ROWS = 17;
static_assert(GRID_COLS * GRID_ROWS == LT_PANEL_TAXELS && GRID_ROWS == LT_TACTILE_ROWS && GRID_COLS == LT_TACTILE_COLS, "the taxel grid");
static_assert(LT_PANEL_VIEWS_PER_LAUNCH == LT_RENDER_VIEWS_PER_LAUNCH, "the renderer's per-launch limit");

struct PanelArgs {
  const float* rows[LT_PANEL_MAX_SIGNALS];
  long long stride[LT_PANEL_MAX_SIGNALS];
  int channels[LT_PANEL_MAX_SIGNALS];
  int ramp_bits[LT_PANEL_MAX_SIGNALS];  // bit c: channel c uses LT_PANEL_MAP_RAMP
  int nsignals, cell, gap, x0, y0, opacity;
  int pw, ph;  // the panel's size
  int width, height;
  uint32_t* rgba;
  int env[LT_PANEL_VIEWS_PER_LAUNCH];
};

__device__ __forceinline__ int intensity(float v) {
  const uint32_t b = __float_as_uint(v);
  if (b >> 31) return 0;
  if (b > 0x7f800000u) return 0;
  if (b >= 0x3f800000u) return 255;
  return (int)rintf(255.0f * v);
}

__device__ __forceinline__ uint32_t ramp(int q) {
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t lo = ((uint32_t)LT_PANEL_COLOR_RAMP_LO >> (8 * k)) & 255u, hi = ((uint32_t)LT_PANEL_COLOR_RAMP_HI >> (8 * k)) & 255u;
    c |= ((lo * (uint32_t)(255 - q) + hi * (uint32_t)q + 127u) / 255u) << (8 * k);
  }
  return c;
}

__global__ __launch_bounds__(TILE_W* TILE_H) void lt_tactile_panel_kernel(const PanelArgs a) {
  const int px = blockIdx.x * TILE_W + (threadIdx.x & (TILE_W - 1)), py = blockIdx.y * TILE_H + (threadIdx.x >> 6);
  if (px >= a.pw || py >= a.ph) return;
  const int view = blockIdx.z;
  uint32_t p;
  if (px == 0 || py == 0 || px == a.pw - 1 || py == a.ph - 1) {
    p = LT_PANEL_COLOR_FRAME;
  } else {
    p = LT_PANEL_COLOR_GAP;
    const int gw = GRID_COLS * a.cell, gh = GRID_ROWS * a.cell;
    const int ix = px - 1, iy = py - 1;
    const int s = iy / (gh + a.gap), ry = iy - s * (gh + a.gap);  // s < nsignals: iy < ph - 2
    const int c = ix / (gw + a.gap), rx = ix - c * (gw + a.gap);
    if (ry < gh && rx < gw && c < a.channels[s]) {
      const int row = ry / a.cell, col = rx / a.cell;
      const float v = a.rows[s][(long long)a.env[view] * a.stride[s] + c * LT_PANEL_TAXELS + row * GRID_COLS + col];
      const int q = intensity(v);
      p = (a.ramp_bits[s] >> c) & 1 ? ramp(q) : (q >= 128 ? (uint32_t)LT_PANEL_COLOR_ON : (uint32_t)LT_PANEL_COLOR_OFF);
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

// the refusals that decide the panel's size; *pw, *ph on LT_OK
int panel_shape(const char* fn, const lt_panel_desc* d, const lt_panel_signal* sig, int* pw, int* ph) {
  if (!d) return refuse(fn, "", "desc", "non-null");
  if (!sig) return refuse(fn, "", "signals", "non-null");
  char what[96];
  if (d->nsignals < 1 || d->nsignals > LT_PANEL_MAX_SIGNALS) {
    snprintf(what, sizeof what, "in 1 ... %d", LT_PANEL_MAX_SIGNALS);
    return refuse(fn, "desc.", "nsignals", what);
  }
  if (d->cell < 1 || d->cell > LT_PANEL_MAX_CELL) {
    snprintf(what, sizeof what, "in 1 ... %d", LT_PANEL_MAX_CELL);
    return refuse(fn, "desc.", "cell", what);
  }
  if (d->gap < 0 || d->gap > LT_PANEL_MAX_GAP) {
    snprintf(what, sizeof what, "in 0 ... %d", LT_PANEL_MAX_GAP);
    return refuse(fn, "desc.", "gap", what);
  }
  int cmax = 0;
  for (int s = 0; s < d->nsignals; ++s) {
    if (sig[s].channels < 1 || sig[s].channels > LT_PANEL_MAX_CHANNELS) {
      char who[32];
      snprintf(who, sizeof who, "signals[%d].", s);
      snprintf(what, sizeof what, "in 1 ... %d", LT_PANEL_MAX_CHANNELS);
      return refuse(fn, who, "channels", what);
    }
    cmax = sig[s].channels > cmax ? sig[s].channels : cmax;
  }
  *pw = 2 + cmax * GRID_COLS * d->cell + (cmax - 1) * d->gap;  // <= 2 + 4 * 13 * 32 + 3 * 16
  *ph = 2 + d->nsignals * GRID_ROWS * d->cell + (d->nsignals - 1) * d->gap;
  return LT_OK;
}

// every refusal of a draw but those of the frame and the env ids
int panel_check(const char* fn, const lt_panel_desc* d, const lt_panel_signal* sig, int nviews, int* pw, int* ph) {
  if (const int rc = panel_shape(fn, d, sig, pw, ph)) return rc;
  char what[96];
  if (d->opacity < 0 || d->opacity > 255) return refuse(fn, "desc.", "opacity", "in 0 ... 255");
  for (int s = 0; s < d->nsignals; ++s) {
    char who[32];
    snprintf(who, sizeof who, "signals[%d].", s);
    if (const int rc = check_ptr(fn, who, {"rows", sig[s].rows, 4})) return rc;
    if (sig[s].row_stride < (int64_t)sig[s].channels * LT_PANEL_TAXELS) return refuse(fn, who, "row_stride", "at least channels * 221");
    if (sig[s].n_envs < 1) return refuse(fn, who, "n_envs", "at least 1");
    for (int c = 0; c < sig[s].channels; ++c)
      if (sig[s].maps[c] != LT_PANEL_MAP_BINARY && sig[s].maps[c] != LT_PANEL_MAP_RAMP)
        return refuse(fn, who, "maps", "LT_PANEL_MAP_BINARY or LT_PANEL_MAP_RAMP for every channel");
  }
  if (nviews < 1 || nviews > LT_PANEL_VIEWS_PER_LAUNCH) {
    snprintf(what, sizeof what, "in 1 ... %d", LT_PANEL_VIEWS_PER_LAUNCH);
    return refuse(fn, "", "nviews", what);
  }
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_tactile_panel_size(const lt_panel_desc* desc, const lt_panel_signal* signals, int* width, int* height) {
  const char* fn = "lt_tactile_panel_size";
  int pw, ph;
  if (const int rc = panel_shape(fn, desc, signals, &pw, &ph)) return rc;
  if (!width) return refuse(fn, "", "width", "non-null");
  if (!height) return refuse(fn, "", "height", "non-null");
  *width = pw;
  *height = ph;
  return LT_OK;
}

int lt_tactile_panel_launches(const lt_panel_desc* desc, const lt_panel_signal* signals, int nviews) {
  int pw, ph;
  if (const int rc = panel_check("lt_tactile_panel_launches", desc, signals, nviews, &pw, &ph)) return rc;
  return 1;
}

int lt_tactile_panel_draw(const lt_panel_desc* desc, const lt_panel_signal* signals, const int32_t* env_ids, int nviews, uint32_t* rgba,
                          int width, int height, void* stream) {
  static_assert(sizeof(PanelArgs) <= 4096, "kernel arguments too large");
  const char* fn = "lt_tactile_panel_draw";
  PanelArgs a = {};
  if (const int rc = panel_check(fn, desc, signals, nviews, &a.pw, &a.ph)) return rc;
  if (!env_ids) return refuse(fn, "", "env_ids", "non-null");
  if (const int rc = check_ptr(fn, "", {"rgba", rgba, 4})) return rc;
  char what[96];
  snprintf(what, sizeof what, "in 1 ... %d", LT_RENDER_MAX_SIZE);
  if (width < 1 || width > LT_RENDER_MAX_SIZE) return refuse(fn, "", "width", what);
  if (height < 1 || height > LT_RENDER_MAX_SIZE) return refuse(fn, "", "height", what);
  if (desc->x0 < 0 || desc->x0 > width - a.pw) {
    snprintf(what, sizeof what, "in 0 ... width - %d (the panel must lie inside the frame)", a.pw);
    return refuse(fn, "desc.", "x0", what);
  }
  if (desc->y0 < 0 || desc->y0 > height - a.ph) {
    snprintf(what, sizeof what, "in 0 ... height - %d (the panel must lie inside the frame)", a.ph);
    return refuse(fn, "desc.", "y0", what);
  }
  for (int v = 0; v < nviews; ++v) {
    char who[32];
    snprintf(who, sizeof who, "env_ids[%d]", v);
    if (env_ids[v] < 0) return refuse(fn, "", who, "non-negative");
    for (int s = 0; s < desc->nsignals; ++s)
      if (env_ids[v] >= signals[s].n_envs) {
        snprintf(what, sizeof what, "below signals[%d].n_envs = %d", s, signals[s].n_envs);
        return refuse(fn, "", who, what);
      }
    a.env[v] = env_ids[v];
  }
  for (int s = 0; s < desc->nsignals; ++s) {
    a.rows[s] = signals[s].rows;
    a.stride[s] = signals[s].row_stride;
    a.channels[s] = signals[s].channels;
    for (int c = 0; c < signals[s].channels; ++c)
      if (signals[s].maps[c] == LT_PANEL_MAP_RAMP) a.ramp_bits[s] |= 1 << c;
  }
  a.nsignals = desc->nsignals; a.cell = desc->cell; a.gap = desc->gap; a.x0 = desc->x0; a.y0 = desc->y0; a.opacity = desc->opacity;
  a.width = width; a.height = height; a.rgba = rgba;
  const dim3 grid((unsigned)((a.pw + TILE_W - 1) / TILE_W), (unsigned)((a.ph + TILE_H - 1) / TILE_H), (unsigned)nviews);
  hipLaunchKernelGGL(lt_tactile_panel_kernel, grid, dim3(TILE_W * TILE_H), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // extern "C"
