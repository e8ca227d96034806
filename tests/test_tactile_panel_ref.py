"""The numpy twin of the taxel panel (tests/tactile_panel_ref.py) held to the text of include/lt_tactile_panel.h: the size formula, the
two ends of the opacity, where one planted taxel lands, and the special values.  No device, no library call."""
import numpy as np
import pytest

from tests import tactile_panel_ref as T


def _frames(v, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 24, size=(v, h, w), dtype=np.uint32) | np.uint32(255 << 24)).astype(np.uint32)


def _rgb(frames):
    return np.ascontiguousarray(frames).view(np.uint8).reshape(*frames.shape, 4)


@pytest.mark.parametrize("cell,gap,channels,size", [
    (1, 0, [1], (2 + 13, 2 + 17)),
    (4, 2, [2], (2 + 2 * 52 + 2, 2 + 68)),
    (4, 2, [2, 2, 4, 4], (2 + 4 * 52 + 3 * 2, 2 + 4 * 68 + 3 * 2)),  # the default panel of the -Play- env under distill.py
    (3, 5, [4, 1, 2], (2 + 4 * 39 + 3 * 5, 2 + 3 * 51 + 2 * 5)),
    (32, 16, [4, 4, 4, 4], (2 + 4 * 416 + 48, 2 + 4 * 544 + 48)),
])
def test_size_formula(cell, gap, channels, size):
    assert T.panel_size(cell, gap, channels) == size
    rows = [np.zeros(c * 221, np.float32) for c in channels]
    assert T.panel_image(rows, [[T.MAP_BINARY] * c for c in channels], cell, gap).shape == (size[1], size[0], 3)


def test_opacity_0_returns_the_frame_and_255_the_panel():
    rng = np.random.default_rng(1)
    sig = [rng.random((3, 442)).astype(np.float32), rng.random((3, 884)).astype(np.float32)]
    maps = [[T.MAP_BINARY, T.MAP_RAMP], [T.MAP_RAMP] * 4]
    frames = _frames(2, 67, 101)
    w, h = T.panel_size(1, 1, [2, 4])
    assert np.array_equal(T.draw(frames, [2, 0], sig, maps, 1, 1, 7, 5, 0), frames)
    out = T.draw(frames, [2, 0], sig, maps, 1, 1, 7, 5, 255)
    for v, e in enumerate([2, 0]):
        img = T.panel_image([s[e] for s in sig], maps, 1, 1)
        assert np.array_equal(_rgb(out)[v, 5:5 + h, 7:7 + w, :3], img)
        assert (_rgb(out)[v, ..., 3] == 255).all()
    outside = np.ones(frames.shape, bool)
    outside[:, 5:5 + h, 7:7 + w] = False
    assert np.array_equal(out[outside], frames[outside])
    # in between: the stated integer blend, byte by byte
    mid = T.draw(frames, [2, 0], sig, maps, 1, 1, 7, 5, 160)
    p, f = _rgb(out)[0, 5 + 3, 7 + 4, :3].astype(int), _rgb(frames)[0, 5 + 3, 7 + 4, :3].astype(int)
    assert list(_rgb(mid)[0, 5 + 3, 7 + 4, :3]) == [(a * 160 + b * 95 + 127) // 255 for a, b in zip(p, f)]


@pytest.mark.parametrize("cell,gap", [(1, 0), (3, 2)])
def test_one_planted_taxel_lands_at_its_cell(cell, gap):
    row, col, ch, s = 5, 7, 1, 1  # taxel row * 13 + col of channel 1 of the second signal
    sig = [np.zeros((1, 442), np.float32), np.zeros((1, 442), np.float32)]
    sig[s][0, ch * 221 + row * 13 + col] = 1.0
    maps = [[T.MAP_BINARY] * 2] * 2
    img = T.panel_image([x[0] for x in sig], maps, cell, gap)
    on = (img == T.ON).all(-1)
    y0 = 1 + s * (17 * cell + gap) + row * cell  # grid row `row` from the top
    x0 = 1 + ch * (13 * cell + gap) + col * cell  # grid column `col` from the left
    expect = np.zeros_like(on)
    expect[y0:y0 + cell, x0:x0 + cell] = True
    assert np.array_equal(on, expect)
    # the frame line, the gaps, and every other taxel in the off colour
    assert (img[0] == T.FRAME).all() and (img[-1] == T.FRAME).all() and (img[:, 0] == T.FRAME).all() and (img[:, -1] == T.FRAME).all()
    n_off = (img == T.OFF).all(-1).sum()
    assert n_off == (4 * 221 - 1) * cell * cell
    assert (img == T.GAP).all(-1).sum() == img.shape[0] * img.shape[1] - n_off - cell * cell - 2 * (img.shape[0] + img.shape[1]) + 4


def test_special_values_and_rounding():
    v = np.array([np.nan, -0.0, 1.5, -3.0, np.inf, -np.inf, 0.0, 1.0, 0.5, 127.5 / 255, 0.1, 1e-40], np.float32)
    q = T.intensity(v)
    assert q.dtype == np.int32
    assert list(q[:8]) == [0, 0, 255, 0, 255, 0, 0, 255]
    assert q[8] == 128  # 127.5 is a tie: to even
    assert q[9] in (127, 128) and q[9] == int(np.rint(np.float32(255.0) * v[9]))
    assert q[10] == 26 and q[11] == 0
    assert (T.taxel_colours(np.array([0, 127, 128, 255]), T.MAP_BINARY) == np.array([T.OFF, T.OFF, T.ON, T.ON])).all()
    ramp = T.taxel_colours(np.array([0, 255, 100]), T.MAP_RAMP)
    assert (ramp[0] == T.LO).all() and (ramp[1] == T.HI).all()
    assert list(ramp[2]) == [(int(lo) * 155 + int(hi) * 100 + 127) // 255 for lo, hi in zip(T.LO, T.HI)]
    # the binary map takes the plate tint's pink and grey as the renderer packs them
    assert list(T.ON) == [int(c * 255.0 + 0.5) for c in (0.95, 0.20, 0.55)] and list(T.OFF) == [int(c * 255.0 + 0.5) for c in (0.62, 0.64, 0.66)]
