/* lt_tactile_panel.h - a panel of taxel grids drawn over rendered frames: what the tactile observation groups hold, shown in the corner
 * of the image lt_env_render wrote (part of the lt_env.h ABI; LT_ABI_VERSION 21).  The reference publishes the same signals on three
 * ROS topics for a viewer (locotouch/distill/distillation.py:132-143, 202-211); here they go into the recorded video.  Implemented in
 * csrc/lt_tactile_panel.hip.
 *
 * The entry points live in a header of their own because they are one optional unit (a caller that records no tactile panel never
 * calls them); locotouch_amd/_abi.py derives their binding from this file by the same rule as from lt_env.h
 * (`_abi.TACTILE_PANEL_SIGNATURES`).  Everything is stream-ordered: one launch, no host synchronisation, no allocation, no host read,
 * no atomics; graph-capturable; bit-deterministic.
 *
 * A SIGNAL is rows [n_envs][channels * 221] of f32 on the device (4-byte aligned, unit column stride, its own row stride in floats - a
 * column slice of wider rows is read in place), 1 to LT_PANEL_MAX_CHANNELS channels, channel-major: taxel (row, col) of channel c is
 * element c * 221 + row * 13 + col, the layout of every tactile observation group (LT_F_OBS_TACTILE, ...).
 *
 * LAYOUT, in pixels, for S signals with C_s channels, a cell of `cell` x `cell` pixels per taxel and `gap` pixels between grids:
 *     grid      13 * cell wide, 17 * cell high.  Taxel row * 13 + col is drawn at grid row `row` from the TOP and grid column `col` from
 *               the LEFT.  Taxel rows run front -> back and columns left -> right (x = X0 - DX * row, y = Y0 - DY * col in the trunk
 *               frame: the mapping of the plate tint in csrc/lt_render.hip), so the robot's front is at the top of a grid and its left
 *               at the left: the plate seen from above, robot facing up.
 *     signal    its channels left to right, channel c at x = 1 + c * (13 * cell + gap)
 *     panel     the signals one below the other, signal s at y = 1 + s * (17 * cell + gap), inside a 1-pixel frame line:
 *               width  = 2 + max_s (C_s * 13 * cell + (C_s - 1) * gap)
 *               height = 2 + S * 17 * cell + (S - 1) * gap
 *     A panel pixel on the outermost line has LT_PANEL_COLOR_FRAME, one in no grid (the gaps, and the space right of a signal with
 *     fewer channels than the widest) LT_PANEL_COLOR_GAP, one in a grid the colour of its taxel.
 * The panel's top-left pixel lies at (x0, y0) of the frame; a pixel outside the panel rectangle is not written (nor read).
 *
 * COLOUR of a taxel value v - one float operation, integers after it:
 *     q = (int)rintf(255.0f * min(max(v, 0), 1))       one multiplication, rounded to nearest even; NaN, -0.0 and v < 0 give 0, v > 1 255
 *     LT_PANEL_MAP_BINARY : q >= 128 ? LT_PANEL_COLOR_ON : LT_PANEL_COLOR_OFF
 *     LT_PANEL_MAP_RAMP   : per colour byte (lo * (255 - q) + hi * q + 127) / 255 with lo, hi the bytes of LT_PANEL_COLOR_RAMP_LO, _HI
 * and of every panel pixel, per colour byte over the frame's byte f:
 *     (p * opacity + f * (255 - opacity) + 127) / 255                                   (integer division; the alpha byte becomes 255)
 * Colours are 0xBBGGRR: byte k of the packed pixel (R, G, B as lt_env_render packs them). */
#ifndef LT_TACTILE_PANEL_H
#define LT_TACTILE_PANEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_PANEL_MAX_SIGNALS 4
#define LT_PANEL_MAX_CHANNELS 4
#define LT_PANEL_MAX_CELL 32        /* cell in 1 ... 32 */
#define LT_PANEL_MAX_GAP 16         /* gap in 0 ... 16 */
#define LT_PANEL_TAXELS 221         /* LT_TACTILE_ROWS * LT_TACTILE_COLS: floats per channel */
#define LT_PANEL_VIEWS_PER_LAUNCH 32 /* == LT_RENDER_VIEWS_PER_LAUNCH: the env ids travel in the kernel arguments */

enum lt_panel_map { LT_PANEL_MAP_BINARY = 0, LT_PANEL_MAP_RAMP = 1 };

enum lt_panel_color {
  LT_PANEL_COLOR_ON = 0x8C33F2,      /* the plate tint's pink (0.95, 0.20, 0.55) as lt_env_render packs it */
  LT_PANEL_COLOR_OFF = 0xA8A39E,     /* the plate tint's grey (0.62, 0.64, 0.66) */
  LT_PANEL_COLOR_RAMP_LO = 0x3C2814, /* q = 0: dark blue */
  LT_PANEL_COLOR_RAMP_HI = 0x3CDCFF, /* q = 255: yellow */
  LT_PANEL_COLOR_FRAME = 0xF0F0F0,
  LT_PANEL_COLOR_GAP = 0x1E1E1E
};

typedef struct lt_panel_signal {
  const float* rows;    /* device, 4-byte aligned: [n_envs][channels * LT_PANEL_TAXELS], row e at rows + e * row_stride */
  int64_t row_stride;   /* floats, >= channels * LT_PANEL_TAXELS */
  int32_t n_envs;       /* rows the signal holds: every env id must be below it */
  int32_t channels;     /* 1 ... LT_PANEL_MAX_CHANNELS */
  int32_t maps[LT_PANEL_MAX_CHANNELS]; /* lt_panel_map per channel (entries from `channels` on are ignored) */
} lt_panel_signal;

typedef struct lt_panel_desc {
  int32_t nsignals;     /* 1 ... LT_PANEL_MAX_SIGNALS */
  int32_t cell, gap;    /* pixels per taxel edge; pixels between grids and between signals */
  int32_t x0, y0;       /* the panel's top-left pixel in the frame */
  int32_t opacity;      /* 0 (the frame shows through unchanged) ... 255 (the panel replaces the frame) */
} lt_panel_desc;

/* Host-only: the panel's width and height by the formula above.  LT_EINVAL for a cell, gap, channel or signal count outside its range
 * (x0, y0, opacity and the signals' pointers, strides and row counts are not looked at). */
int lt_tactile_panel_size(const lt_panel_desc* desc, const lt_panel_signal* signals, int* width, int* height);

/* Draws the panel of env env_ids[v] into frame v of rgba, uint32 [nviews][height][width] (the buffer lt_env_render writes: one packed
 * dword per pixel, device, 4-byte aligned), for v < nviews <= LT_PANEL_VIEWS_PER_LAUNCH.  env_ids is a HOST array: it is copied into
 * the kernel arguments.  One launch on `stream`.
 * LT_EINVAL with "<function>: invalid argument: <field> must be ...", before anything is launched, for: a null desc, signals or env_ids,
 * nsignals, cell, gap, opacity or a signal's channels or a map outside its range, a row stride below channels * LT_PANEL_TAXELS, a
 * null or misaligned rgba or signal pointer, nviews outside 1 ... LT_PANEL_VIEWS_PER_LAUNCH, a width or height outside
 * 1 ... LT_RENDER_MAX_SIZE, a panel that does not lie wholly inside width x height at (x0, y0), an env id that is negative or not
 * below every signal's n_envs. */
int lt_tactile_panel_draw(const lt_panel_desc* desc, const lt_panel_signal* signals, const int32_t* env_ids, int nviews, uint32_t* rgba,
                          int width, int height, void* stream);

/* VALUE query: the number of kernel launches one lt_tactile_panel_draw of this panel and view count issues (1), or a negative LT_*
 * code for a descriptor or view count it refuses.  Host-only. */
int lt_tactile_panel_launches(const lt_panel_desc* desc, const lt_panel_signal* signals, int nviews);

#ifdef __cplusplus
}
#endif

#endif /* LT_TACTILE_PANEL_H */
