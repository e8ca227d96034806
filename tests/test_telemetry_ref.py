"""The numpy twin of the telemetry ring and its strip charts (tests/telemetry_ref.py) against cases worked by hand from the text of
include/lt_telemetry.h.  No device is needed."""
import numpy as np

from tests import telemetry_ref as T

C = T.T
CHARS = {".": C["LT_CHART_COLOR_BG"], "z": C["LT_CHART_COLOR_ZERO"], "g": C["LT_CHART_COLOR_GAP"], "#": C["LT_CHART_COLOR_FRAME"],
         "0": C["LT_CHART_COLOR_SERIES_0"], "1": C["LT_CHART_COLOR_SERIES_1"], "2": C["LT_CHART_COLOR_SERIES_2"], "3": C["LT_CHART_COLOR_SERIES_3"]}
OPAQUE = 255 << 24


def _picture(rows):
    """uint32 [h, w]: the packed pixels (alpha 255) of a panel written as one character per pixel."""
    return np.array([[CHARS[ch] | OPAQUE for ch in row] for row in rows], dtype=np.uint32)


def _ring(samples, capacity=8, channels=1):
    """A twin ring of one env with `samples` (one value, or one per channel, per record) recorded in order."""
    ring = T.Ring(channels, 1, capacity)
    for s in samples:
        ring.record([list(s) if isinstance(s, (list, tuple)) else [s]])
    return ring


def _one_plot(samples, k=1.0, y_zero=7, frame=None, opacity=255, capacity=8):
    ring = _ring(samples, capacity)
    frames = np.zeros((1, 10, 10), dtype=np.uint32) if frame is None else frame
    return T.chart(frames, ring.ring, int(ring.head[0]), [0], [([0], k, y_zero)], 8, 8, 0, 0, 0, opacity)[0]


def test_a_three_sample_ramp_pixel_by_pixel():
    # k = 1, the row of value 0 is 7: the values 0, 2, 6 lie on rows 7, 5, 1.  Three records in an 8-column plot: the columns 0 ... 4
    # have no record yet; column 5 has no left neighbour and colours its own row; columns 6 and 7 colour from the left row to their own.
    got = _one_plot([0.0, 2.0, 6.0])
    want = _picture(["##########",
                     "#........#",
                     "#.......0#",
                     "#.......0#",
                     "#.......0#",
                     "#.......0#",
                     "#......00#",
                     "#......0.#",
                     "#zzzzz00z#",
                     "##########"])
    assert np.array_equal(got, want)


def test_sizes_and_plan_bytes():
    assert T.chart_size(1, 8, 8, 0) == (10, 10) and T.chart_size(3, 240, 48, 2) == (242, 2 + 144 + 4) and T.chart_size(4, 1024, 256, 16) == (1026, 1074)
    assert T.plan_bytes(1, 1) == 16 + 16 + 32 and T.plan_bytes(64, 32) == 16 + 128 + 2048 and T.plan_bytes(5, 5) == 16 + 32 + 160


def test_a_tie_goes_to_the_even_row():
    rows, drawn = T.value_rows(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5], dtype=np.float32), 1.0, 8, 16)
    assert drawn.all() and rows.tolist() == [8, 6, 6, 8, 10, 10]  # rint: 0, 2, 2, -0, -2, -2
    # the product is rounded to float32 BEFORE the tie is decided: 0.1f * 5 = 0.5000000074505806 in exact arithmetic, 0.5f as a float
    rows, _ = T.value_rows(np.array([5.0], dtype=np.float32), np.float32(0.1), 8, 16)
    assert rows.tolist() == [8]


def test_a_nan_breaks_the_line():
    got = _one_plot([0.0, np.nan, 6.0])
    want = _picture(["##########",
                     "#........#",
                     "#.......0#",  # the sample right of the NaN has no drawn left neighbour: its own row alone
                     "#........#",
                     "#........#",
                     "#........#",
                     "#........#",
                     "#........#",
                     "#zzzzz0zz#",  # the NaN's column shows the background (here: the zero line)
                     "##########"])
    assert np.array_equal(got, want)


def test_far_values_clamp_to_the_edge_rows_and_huge_ones_are_skipped():
    just_below = np.float32(2.0 ** 30) - np.float32(64.0)  # the largest float32 below 2 ** 30
    assert float(just_below) == 2.0 ** 30 - 64
    v = np.array([1e6, -1e6, just_below, -just_below, 2.0 ** 30, -(2.0 ** 30), 1e30, np.inf, -np.inf, np.nan], dtype=np.float32)
    rows, drawn = T.value_rows(v, 1.0, 7, 8)
    assert drawn.tolist() == [True] * 4 + [False] * 6
    assert rows[:4].tolist() == [0, 7, 0, 7]
    # the decision is on the PRODUCT: 1e30 * 1e-30 is drawn, 3e5 * 4e3 is not
    rows, drawn = T.value_rows(np.array([1e30, 3e5], dtype=np.float32), np.float32(1e-30), 7, 8)
    assert drawn.tolist() == [True, True] and rows.tolist() == [6, 7]
    assert T.value_rows(np.array([3e5], dtype=np.float32), np.float32(4e3), 7, 8)[1].tolist() == [False]
    got = _one_plot([1e6, 0.0, -1e6])
    want = _picture(["##########",
                     "#.....00.#",
                     "#......0.#",
                     "#......0.#",
                     "#......0.#",
                     "#......0.#",
                     "#......0.#",
                     "#......0.#",
                     "#zzzzzz00#",
                     "##########"])
    assert np.array_equal(got, want)


def test_y_zero_outside_the_plot():
    # the row of value 0 is 20, below the plot: no zero line; 15 lies on row 5, 30 above the top (row 0), 0 on the bottom row
    got = _one_plot([15.0, 30.0, 0.0], y_zero=20)
    want = _picture(["##########",
                     "#......00#",
                     "#......00#",
                     "#......00#",
                     "#......00#",
                     "#......00#",
                     "#.....000#",
                     "#.......0#",
                     "#.......0#",
                     "##########"])
    assert np.array_equal(got, want)
    rows, drawn = T.value_rows(np.array([-5.0, 0.0], dtype=np.float32), 1.0, -3, 8)  # above the plot: -3 - (-5) = 2
    assert drawn.all() and rows.tolist() == [2, 0]


def test_opacity_0_leaves_the_frame_and_255_replaces_it():
    rng = np.random.default_rng(3)
    frame = (rng.integers(0, 1 << 24, size=(1, 10, 10)).astype(np.uint32) | np.uint32(OPAQUE))
    assert np.array_equal(_one_plot([0.0, 2.0, 6.0], frame=frame, opacity=0), frame[0])
    assert np.array_equal(_one_plot([0.0, 2.0, 6.0], frame=frame, opacity=255), _one_plot([0.0, 2.0, 6.0]))
    # in between: (p * o + f * (255 - o) + 127) // 255 per colour byte; the frame line (0xF0) over a byte of 0x10 at 128
    frame[:] = 0x101010 | OPAQUE
    assert _one_plot([0.0], frame=frame, opacity=128)[0, 0] == (OPAQUE | 0x010101 * ((0xF0 * 128 + 0x10 * 127 + 127) // 255))


def test_later_series_draw_over_earlier_ones_and_plots_stack_with_gaps():
    ring = _ring([(1.0, 1.0, 9.0)] * 2, capacity=8, channels=3)
    frames = np.zeros((1, 21, 12), dtype=np.uint32)
    got = T.chart(frames, ring.ring, 2, [0], [([0, 1], 1.0, 7), ([2], 0.5, 7)], 8, 8, 1, 1, 1, 255)[0]
    assert (got[0] == 0).all() and (got[:, 0] == 0).all() and (got[:, 11] == 0).all() and (got[20] == 0).all()  # outside the panel
    want = _picture(["##########",
                     "#........#", "#........#", "#........#", "#........#", "#........#", "#........#",
                     "#......11#",  # both series lie on row 6: the later one shows
                     "#zzzzzzzz#",
                     "#gggggggg#",
                     "#........#", "#........#", "#........#",
                     "#......00#",  # 9 * 0.5 = 4.5 -> 4 (even): row 3 of the second plot, whose first series it is
                     "#........#", "#........#", "#........#",
                     "#zzzzzzzz#",
                     "##########"])
    assert np.array_equal(got[1:20, 1:11], want)


def test_ring_wraps_and_converts_by_value():
    ring = T.Ring(4, 2, 3)
    for t in range(5):
        ring.record([[np.float32(t + 0.25), np.int64(2 ** 24 + 1 + 2 * t), np.uint8(250 + t), np.int32(-7 - t)],
                     [np.float32(-t), np.int64(-t), np.uint8(t), np.int32(2 ** 31 - 1)]])
        assert ring.head.tolist() == [t + 1, (t + 1) % 3]
    # slot t % 3 holds record t: 3 and 4 overwrote 0 and 1
    assert ring.ring[:, 0, 0].tolist() == [3.25, 4.25, 2.25]
    # 2 ** 24 + 1 is a tie between 2 ** 24 and 2 ** 24 + 2: to even; 2 ** 24 + 3 between + 2 and + 4: to + 4
    assert ring.ring[:, 0, 1].tolist() == [2.0 ** 24 + 8, 2.0 ** 24 + 8, 2.0 ** 24 + 4]
    assert ring.ring[:, 0, 2].tolist() == [253.0, 254.0, 252.0] and ring.ring[:, 0, 3].tolist() == [-10.0, -11.0, -9.0]
    assert ring.ring[0, 1].tolist() == [-3.0, -3.0, 3.0, 2.0 ** 31]
    assert ring.read()[:, 0, 0].tolist() == [2.25, 3.25, 4.25]  # chronological
    short = T.Ring(1, 1, 4)
    short.record([[1.0]])
    assert short.read().tolist() == [[[1.0]]]
