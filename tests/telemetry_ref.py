"""An independent numpy twin of the telemetry ring and its strip charts (include/lt_telemetry.h): colours and limits from
`_abi.TELEMETRY_CONSTS`, the arithmetic from the header's text.  A record is a copy with a conversion by value; the chart is integer
behind one correctly rounded float32 product.  So the twin and the kernels agree bit for bit and no test that uses it has a tolerance.

    plan_bytes(nchannels, nenvs), chart_size(nplots, pw, ph, gap)
    Ring(nchannels, nenvs, capacity).record(values)      values: [nenvs, nchannels], any of the four dtypes per element
    value_rows(v, k, y_zero, ph)                         -> (row int64, drawn bool)
    chart(frames, ring, head0, slots, plots, pw, ph, gap, x0, y0, opacity) -> a new uint32 [V, H, W] array

`plots` is a list of (channel indices, k, y_zero); `ring` float32 [capacity, nenvs, nchannels]; `frames` uint32 [V, H, W] packed RGBA
(byte 0 = R)."""
from __future__ import annotations

import numpy as np

from locotouch_amd import _abi

T = _abi.TELEMETRY_CONSTS
SERIES = [T[f"LT_CHART_COLOR_SERIES_{s}"] for s in range(T["LT_CHART_MAX_SERIES"])]
SKIP_FROM = 0x4E800000  # the bits of float32(2 ** 30)
assert np.array([2.0 ** 30], dtype=np.float32).view(np.uint32)[0] == SKIP_FROM


def _bytes(colour: int) -> np.ndarray:
    """0xBBGGRR -> int64 [3] (R, G, B)."""
    return np.array([(colour >> (8 * k)) & 255 for k in range(3)], dtype=np.int64)


def plan_bytes(nchannels: int, nenvs: int) -> int:
    return T["LT_TELEMETRY_PLAN_HEADER_BYTES"] + 16 * ((nenvs + 3) // 4) + T["LT_TELEMETRY_PLAN_CHANNEL_BYTES"] * nchannels


def chart_size(nplots: int, pw: int, ph: int, gap: int) -> tuple[int, int]:
    return 2 + pw, 2 + nplots * ph + (nplots - 1) * gap


def to_f32(x) -> np.float32:
    """One stored scalar (f32, i64, u8 or i32) as the record keeps it: by value, integers to nearest (ties to even)."""
    return np.float32(x)


class Ring:
    def __init__(self, nchannels: int, nenvs: int, capacity: int):
        self.ring = np.zeros((capacity, nenvs, nchannels), dtype=np.float32)
        self.head = np.zeros(2, dtype=np.int64)

    def record(self, values) -> None:
        """values[i][c]: channel c of the i-th env of the plan, as stored."""
        capacity = self.ring.shape[0]
        slot = int(self.head[0]) % capacity
        for i, row in enumerate(values):
            for c, x in enumerate(row):
                self.ring[slot, i, c] = to_f32(x)
        self.head[0] += 1
        self.head[1] = int(self.head[0]) % capacity

    def read(self) -> np.ndarray:
        """Chronological [T, nenvs, nchannels], T = min(count, capacity)."""
        count, capacity = int(self.head[0]), self.ring.shape[0]
        if count <= capacity:
            return self.ring[:count].copy()
        return np.roll(self.ring, -(count % capacity), axis=0)


def value_rows(v, k, y_zero: int, ph: int):
    """(row, drawn): p = k * v in float32; |p| >= 2 ** 30, inf and NaN (by the product's bits) are not drawn; row = clamp(y_zero -
    rint(p), 0, ph - 1)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = (np.float32(k) * v.reshape(-1)).astype(np.float32)  # the one float operation, rounded to float32
    drawn = (p.view(np.uint32) & 0x7FFFFFFF) < SKIP_FROM
    r = int(y_zero) - np.rint(np.where(drawn, p, np.float32(0))).astype(np.int64)  # to nearest, ties to even
    return np.clip(r, 0, ph - 1).reshape(v.shape), drawn.reshape(v.shape)


def chart_image(ring, head0: int, slot: int, plots, pw: int, ph: int, gap: int) -> np.ndarray:
    """int64 [h, w]: the packed 0xBBGGRR colours of the panel of one env slot."""
    w, h = chart_size(len(plots), pw, ph, gap)
    capacity = ring.shape[0]
    img = np.full((h, w), T["LT_CHART_COLOR_GAP"], dtype=np.int64)
    img[0, :] = img[-1, :] = img[:, 0] = img[:, -1] = T["LT_CHART_COLOR_FRAME"]
    for n, (channels, k, y_zero) in enumerate(plots):
        top = 1 + n * (ph + gap)
        plot = np.full((ph, pw), T["LT_CHART_COLOR_BG"], dtype=np.int64)
        if 0 <= y_zero < ph:
            plot[y_zero, :] = T["LT_CHART_COLOR_ZERO"]
        for s, c in enumerate(channels):
            prev = None  # the row of the column to the left, if it was drawn
            for x in range(pw):
                rec = head0 - pw + x
                if rec < 0:
                    prev = None
                    continue
                row, drawn = value_rows(ring[rec % capacity, slot, c], k, y_zero, ph)
                if not drawn:
                    prev = None
                    continue
                row = int(row)
                lo, hi = (row, row) if prev is None else (min(prev, row), max(prev, row))
                plot[lo:hi + 1, x] = SERIES[s]
                prev = row
        img[top:top + ph, 1:1 + pw] = plot
    return img


def chart(frames, ring, head0: int, slots, plots, pw: int, ph: int, gap: int, x0: int, y0: int, opacity: int) -> np.ndarray:
    frames = np.array(frames, dtype=np.uint32, copy=True)
    assert frames.ndim == 3 and len(slots) == frames.shape[0] and pw <= ring.shape[0]
    for v, slot in enumerate(slots):
        img = chart_image(np.asarray(ring, dtype=np.float32), int(head0), int(slot), plots, pw, ph, gap)
        h, w = img.shape
        assert 0 <= x0 and x0 + w <= frames.shape[2] and 0 <= y0 and y0 + h <= frames.shape[1], "the panel must lie inside the frame"
        under = frames[v, y0:y0 + h, x0:x0 + w].astype(np.int64)
        out = np.full((h, w), 255 << 24, dtype=np.int64)  # the alpha byte
        for k in range(3):
            p, f = (img >> (8 * k)) & 255, (under >> (8 * k)) & 255
            out |= ((p * opacity + f * (255 - opacity) + 127) // 255) << (8 * k)
        frames[v, y0:y0 + h, x0:x0 + w] = out.astype(np.uint32)
    return frames
