/* lt_telemetry.h - per-step telemetry of chosen envs, kept on the device, and strip charts of it drawn over rendered frames (part of the
 * lt_env.h ABI; LT_ABI_VERSION 21).  The reference's play loop prints env 0's observation terms behind a `print_obs` switch
 * (locotouch/scripts/play.py:132-178); here chosen scalars of chosen envs go into a device ring behind every env step, are read out
 * once at the end, and their newest samples can be charted into the recorded video.  Implemented in csrc/lt_telemetry.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a caller that records no telemetry never calls
 * them); locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h (`_abi.TELEMETRY_SIGNATURES`).
 * Everything is stream-ordered: no allocation, no host read, no atomics; the record and the chart are graph-capturable and
 * bit-deterministic.
 *
 * A CHANNEL is one stored scalar per env: the value of env e is base[e * env_stride + offset], both counted in elements of `dtype`
 * (lt_view's codes: 0 f32, 1 i64, 2 u8, 3 i32), converted to f32 by value (integers round to nearest, ties to even).  This one form
 * covers every arena view (lt_env_get_view gives the pointer and the strides; component c of a quad field is element
 * (c / 4) * stride[1] + (c % 4) * stride[2]), a column of observation rows or of a storage slot, the contact-force buffer, and any
 * tensor of the caller.  A channel is a stored value, never a derived one.
 *
 * The PLAN is the channel table and the env list in caller-owned device memory (64 channels do not fit into kernel arguments):
 *     lt_telemetry_plan_bytes = LT_TELEMETRY_PLAN_HEADER_BYTES + 16 * ceil(nenvs / 4) + LT_TELEMETRY_PLAN_CHANNEL_BYTES * nchannels
 * The RING is f32 [capacity][nenvs][nchannels]; the HEAD is int64 [2], zeroed by the caller before the first record:
 *     head[0]   records written so far
 *     head[1]   head[0] % capacity: the slot the next record goes to
 * One record writes slot head[0] % capacity - element [slot][i][c] is channel c of env env_ids[i] - and then increments head[0] once,
 * behind a workgroup barrier (one launch of ONE workgroup: there is no second one to race with).  The counter lives on the device, so
 * a record captured into a graph advances with every replay.
 *
 * The CHART, in pixels: P plots of pw x ph pixels one below the other, `gap` pixels between them, inside a 1-pixel frame line:
 *     width  = 2 + pw
 *     height = 2 + P * ph + (P - 1) * gap
 * Plot p occupies panel rows 1 + p * (ph + gap) ... + ph - 1 and panel columns 1 ... pw.  The panel's top-left pixel lies at (x0, y0)
 * of the frame; a pixel outside the panel rectangle is neither read nor written.
 * Column x (0 = left) of every plot shows record head[0] - pw + x of env slot slots[view]: the newest record at the right.  A column
 * whose record does not exist yet (a negative index) shows background only.  pw <= capacity, so every shown record is still held.
 * ROW of a value v in a plot with scale k (pixels per unit, f32) and y_zero (the row of value 0, counted from the plot's top, possibly
 * outside the plot) - ONE float operation, integers after it:
 *     p = k * v                                  one multiplication, rounded to f32
 *     a sample whose p has an exponent-and-mantissa bit pattern >= 0x4E800000 (|p| >= 2^30, +-inf, every NaN) is SKIPPED: it draws
 *     nothing and breaks the line - decided on the bits of p, not by a float comparison
 *     r = y_zero - (int)rintf(p)                 to nearest, ties to even; then clamped to 0 ... ph - 1
 * LINE: in column x the series s of a plot colours the rows min(r(x - 1), r(x)) ... max(r(x - 1), r(x)), and row r(x) alone where the
 * left neighbour is missing (x = 0, or no such record) or skipped; a skipped r(x) colours nothing.  Series are drawn in order: a later
 * one over an earlier one.  Series s of a plot has LT_CHART_COLOR_SERIES_s.
 * BACKGROUND: row y_zero of a plot, where it lies inside it, has LT_CHART_COLOR_ZERO, the rest of the plot LT_CHART_COLOR_BG, the gaps
 * LT_CHART_COLOR_GAP, the outermost line LT_CHART_COLOR_FRAME.
 * BLEND of every panel pixel, per colour byte p over the frame's byte f, exactly the taxel panel's (lt_tactile_panel.h):
 *     (p * opacity + f * (255 - opacity) + 127) / 255                                   (integer division; the alpha byte becomes 255)
 * Colours are 0xBBGGRR: byte k of the packed pixel (R, G, B as lt_env_render packs them).
 * There are no labels (there is no font) and no autoscale (a frame would depend on the future): the ranges are the caller's. */
#ifndef LT_TELEMETRY_H
#define LT_TELEMETRY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_TELEMETRY_MAX_CHANNELS 64
#define LT_TELEMETRY_MAX_ENVS 32
#define LT_TELEMETRY_MAX_CAPACITY 1048576   /* 2^20 records */
#define LT_TELEMETRY_PLAN_HEADER_BYTES 16
#define LT_TELEMETRY_PLAN_CHANNEL_BYTES 32
#define LT_CHART_MAX_PLOTS 4
#define LT_CHART_MAX_SERIES 4               /* channels per plot */
#define LT_CHART_MIN_PLOT 8                 /* pw and ph from 8 on */
#define LT_CHART_MAX_PLOT_WIDTH 1024
#define LT_CHART_MAX_PLOT_HEIGHT 256
#define LT_CHART_MAX_GAP 16                 /* gap in 0 ... 16 */
#define LT_CHART_MAX_ZERO 1073741824        /* |y_zero| <= 2^30 */
#define LT_CHART_VIEWS_PER_LAUNCH 32        /* == LT_RENDER_VIEWS_PER_LAUNCH: the slots travel in the kernel arguments */

enum lt_chart_color {
  LT_CHART_COLOR_SERIES_0 = 0x3C4CE7, /* red */
  LT_CHART_COLOR_SERIES_1 = 0x71CC2E, /* green */
  LT_CHART_COLOR_SERIES_2 = 0xDB9834, /* blue */
  LT_CHART_COLOR_SERIES_3 = 0x0FC4F1, /* yellow */
  LT_CHART_COLOR_BG = 0x181818,
  LT_CHART_COLOR_ZERO = 0x707070,
  LT_CHART_COLOR_GAP = 0x1E1E1E,
  LT_CHART_COLOR_FRAME = 0xF0F0F0
};

typedef struct lt_telemetry_channel {
  const void* base;     /* device, aligned to its element: the element of env 0 at offset 0 */
  int32_t dtype;        /* lt_view's codes: 0 f32, 1 i64, 2 u8, 3 i32 */
  int64_t env_stride;   /* elements between two envs, >= 0 */
  int64_t offset;       /* elements, >= 0 */
} lt_telemetry_channel;

typedef struct lt_chart_plot {
  int32_t nseries;                        /* 1 ... LT_CHART_MAX_SERIES */
  int32_t channels[LT_CHART_MAX_SERIES];  /* indices into the plan's channels (entries from `nseries` on are ignored) */
  float k;                                /* pixels per unit, finite */
  int32_t y_zero;                         /* the row of value 0, |y_zero| <= LT_CHART_MAX_ZERO */
} lt_chart_plot;

typedef struct lt_chart_desc {
  int32_t nplots;       /* 1 ... LT_CHART_MAX_PLOTS */
  int32_t pw, ph;       /* a plot's size: LT_CHART_MIN_PLOT ... LT_CHART_MAX_PLOT_WIDTH / _HEIGHT */
  int32_t gap;          /* pixels between plots */
  int32_t x0, y0;       /* the panel's top-left pixel in the frame */
  int32_t opacity;      /* 0 (the frame shows through unchanged) ... 255 (the panel replaces the frame) */
  lt_chart_plot plots[LT_CHART_MAX_PLOTS];
} lt_chart_desc;

/* Host-only: the bytes of a plan by the formula above.  LT_EINVAL for a channel or env count outside its range. */
int lt_telemetry_plan_bytes(int nchannels, int nenvs, size_t* bytes);

/* Writes the plan of `channels` (HOST array) for the envs `env_ids` (HOST array; element [slot][i][...] of the ring is env env_ids[i])
 * and a ring of `capacity` records into `device_plan` (device, 16-byte aligned, `bytes` >= lt_telemetry_plan_bytes): ONE async copy on
 * `stream` from a staging copy of its own (the caller's arrays are free on return).
 * LT_EINVAL with "<function>: invalid argument: <field> must be ...", before anything is copied, for: a null channels or env_ids,
 * nchannels outside 1 ... LT_TELEMETRY_MAX_CHANNELS, nenvs outside 1 ... LT_TELEMETRY_MAX_ENVS, capacity outside
 * 1 ... LT_TELEMETRY_MAX_CAPACITY, a dtype outside 0 ... 3, a base that is null or not aligned to its element, a negative env_stride,
 * offset or env id, a null or misaligned device_plan, too few bytes.  (Whether env_ids[i] * env_stride + offset lies inside the
 * channel's array only the caller knows.) */
int lt_telemetry_plan(const lt_telemetry_channel* channels, int nchannels, const int32_t* env_ids, int nenvs, int64_t capacity,
                      void* device_plan, size_t bytes, void* stream);

/* One record (see above): ONE launch of ONE workgroup on `stream`.  `ring`: device f32 [capacity][nenvs][nchannels] of the plan,
 * 4-byte aligned; `head`: device int64 [2], 8-byte aligned.  LT_EINVAL, before the launch, for a null or misaligned pointer.  A plan
 * that lt_telemetry_plan did not write makes the launch do nothing. */
int lt_telemetry_record(const void* device_plan, float* ring, int64_t* head, void* stream);

/* VALUE query: the number of kernel launches one lt_telemetry_record issues (1), or a negative LT_* code for arguments it refuses.
 * Host-only. */
int lt_telemetry_record_launches(const void* device_plan, const float* ring, const int64_t* head);

/* Host-only: the panel's width and height by the formula above.  LT_EINVAL for a null pointer or nplots, pw, ph or gap outside its
 * range (nothing else of desc is looked at). */
int lt_telemetry_chart_size(const lt_chart_desc* desc, int* width, int* height);

/* Draws the chart of env slot slots[v] (an index into the plan's env list) into frame v of rgba, uint32 [nviews][height][width] (the
 * buffer lt_env_render writes: one packed dword per pixel, device, 4-byte aligned), for v < nviews <= LT_CHART_VIEWS_PER_LAUNCH, from
 * the newest records of `ring` f32 [capacity][nenvs][nchannels] and `head` as lt_telemetry_record keeps them.  `slots` is a HOST
 * array: it is copied into the kernel arguments.  ONE launch on `stream`: one thread per panel pixel, at most 8 ring reads each.
 * LT_EINVAL with "<function>: invalid argument: <field> must be ...", before anything is launched, for: a null desc or slots; nplots,
 * pw, ph, gap or opacity outside its range; a plot's nseries outside 1 ... LT_CHART_MAX_SERIES, a channel index outside
 * 0 ... nchannels - 1, a k that is not finite, a y_zero beyond +-LT_CHART_MAX_ZERO; nenvs, nchannels or capacity outside the plan's
 * ranges; pw > capacity; a null or misaligned ring, head or rgba; nviews outside 1 ... LT_CHART_VIEWS_PER_LAUNCH; a slot outside
 * 0 ... nenvs - 1; a width or height outside 1 ... LT_RENDER_MAX_SIZE; a panel that does not lie wholly inside width x height at
 * (x0, y0). */
int lt_telemetry_chart_draw(const lt_chart_desc* desc, const float* ring, const int64_t* head, int nenvs, int nchannels, int64_t capacity,
                            const int32_t* slots, int nviews, uint32_t* rgba, int width, int height, void* stream);

/* VALUE query: the number of kernel launches one lt_telemetry_chart_draw of this chart issues (1), or a negative LT_* code for a
 * descriptor, ring shape or view count it refuses.  Host-only. */
int lt_telemetry_chart_launches(const lt_chart_desc* desc, int nenvs, int nchannels, int64_t capacity, int nviews);

#ifdef __cplusplus
}
#endif

#endif /* LT_TELEMETRY_H */
