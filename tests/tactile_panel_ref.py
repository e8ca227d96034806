"""An independent numpy twin of the taxel panel (include/lt_tactile_panel.h): colours and limits from `_abi.TACTILE_PANEL_CONSTS`, the
arithmetic from the header's text.  All of it is integer behind one correctly rounded float32 product, so the twin and the kernel agree
bit for bit and no test that uses it has a tolerance.

    panel_size(cell, gap, channels)                      -> (width, height)
    intensity(v)                                         -> q, int32, the shape of v
    draw(frames, env_ids, signals, maps, cell, gap, x0, y0, opacity) -> a new uint32 [V, H, W] array

`signals` is a list of float32 [N, C * 221] arrays, `maps` one list of colour maps per signal, `frames` uint32 [V, H, W] packed RGBA
(byte 0 = R)."""
from __future__ import annotations

import numpy as np

from locotouch_amd import _abi

P = _abi.TACTILE_PANEL_CONSTS
ROWS, COLS = _abi.CONSTS["LT_TACTILE_ROWS"], _abi.CONSTS["LT_TACTILE_COLS"]
TAXELS = P["LT_PANEL_TAXELS"]
assert TAXELS == ROWS * COLS == 221
MAP_BINARY, MAP_RAMP = P["LT_PANEL_MAP_BINARY"], P["LT_PANEL_MAP_RAMP"]


def _bytes(colour: int) -> np.ndarray:
    """0xBBGGRR -> int64 [3] (R, G, B)."""
    return np.array([(colour >> (8 * k)) & 255 for k in range(3)], dtype=np.int64)


ON, OFF = _bytes(P["LT_PANEL_COLOR_ON"]), _bytes(P["LT_PANEL_COLOR_OFF"])
LO, HI = _bytes(P["LT_PANEL_COLOR_RAMP_LO"]), _bytes(P["LT_PANEL_COLOR_RAMP_HI"])
FRAME, GAP = _bytes(P["LT_PANEL_COLOR_FRAME"]), _bytes(P["LT_PANEL_COLOR_GAP"])


def panel_size(cell: int, gap: int, channels) -> tuple[int, int]:
    channels = list(channels)
    s, cmax = len(channels), max(channels)
    return 2 + cmax * COLS * cell + (cmax - 1) * gap, 2 + s * ROWS * cell + (s - 1) * gap


def intensity(v) -> np.ndarray:
    """q = (int)rintf(255.0f * min(max(v, 0), 1)); NaN draws as 0."""
    v = np.asarray(v, dtype=np.float32)
    clamped = np.where(v >= np.float32(1.0), np.float32(1.0), np.where(v > np.float32(0.0), v, np.float32(0.0))).astype(np.float32)  # NaN: neither
    prod = (np.float32(255.0) * clamped).astype(np.float32)  # the one float operation, rounded to float32
    return np.rint(prod).astype(np.int32)  # to nearest, ties to even


def taxel_colours(q: np.ndarray, cmap: int) -> np.ndarray:
    """int64 [..., 3] colour bytes of intensities q under one colour map."""
    q = q.astype(np.int64)[..., None]
    if cmap == MAP_BINARY:
        return np.where(q >= 128, ON, OFF)
    if cmap == MAP_RAMP:
        return (LO * (255 - q) + HI * q + 127) // 255
    raise ValueError(f"unknown colour map {cmap}")


def panel_image(rows, maps, cell: int, gap: int) -> np.ndarray:
    """int64 [h, w, 3]: the panel of one env. `rows`: one float32 [C * 221] row per signal."""
    w, h = panel_size(cell, gap, [len(r) // TAXELS for r in rows])
    img = np.empty((h, w, 3), dtype=np.int64)
    img[:] = GAP
    img[0, :], img[-1, :], img[:, 0], img[:, -1] = FRAME, FRAME, FRAME, FRAME
    gw, gh = COLS * cell, ROWS * cell
    for s, (row, smaps) in enumerate(zip(rows, maps)):
        grids = np.asarray(row, dtype=np.float32).reshape(-1, ROWS, COLS)  # channel-major; taxel row * 13 + col
        for c, grid in enumerate(grids):
            col = taxel_colours(intensity(grid), smaps[c])  # [17, 13, 3]: grid row from the top, grid column from the left
            y, x = 1 + s * (gh + gap), 1 + c * (gw + gap)
            img[y:y + gh, x:x + gw] = np.repeat(np.repeat(col, cell, axis=0), cell, axis=1)
    return img


def draw(frames, env_ids, signals, maps, cell: int, gap: int, x0: int, y0: int, opacity: int) -> np.ndarray:
    frames = np.array(frames, dtype=np.uint32, copy=True)
    assert frames.ndim == 3 and len(env_ids) == frames.shape[0]
    for v, e in enumerate(env_ids):
        img = panel_image([np.asarray(s)[e] for s in signals], maps, cell, gap)
        h, w, _ = img.shape
        assert 0 <= x0 and x0 + w <= frames.shape[2] and 0 <= y0 and y0 + h <= frames.shape[1], "the panel must lie inside the frame"
        under = frames[v, y0:y0 + h, x0:x0 + w].astype(np.int64)
        out = np.full((h, w), 255 << 24, dtype=np.int64)  # the alpha byte
        for k in range(3):
            f = (under >> (8 * k)) & 255
            out |= ((img[..., k] * opacity + f * (255 - opacity) + 127) // 255) << (8 * k)
        frames[v, y0:y0 + h, x0:x0 + w] = out.astype(np.uint32)
    return frames
