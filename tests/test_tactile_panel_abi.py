"""include/lt_tactile_panel.h: a header of its own, bound by one row of `_abi.HEADERS`; the host-only size query against the numpy twin;
every refusal of lt_tactile_panel_draw by its field's name, before anything is launched (no device is needed: the pointers here are
made-up addresses that a refused call never follows); and the refusals of the Python front."""
import argparse
import ctypes
import itertools

import pytest

from locotouch_amd import _abi
from locotouch_amd import render as R
from tests import tactile_panel_ref as T

FAKE = 0x10000  # a 4-byte aligned address that is never dereferenced


def _signals(channels, stride=None, n_envs=3, rows=FAKE):
    arr = (_abi.LtPanelSignal * max(1, len(channels)))()
    for s, c in zip(arr, channels):
        s.rows, s.row_stride, s.n_envs, s.channels = rows, (c * 221 if stride is None else stride), n_envs, c
    return arr


def _desc(nsignals, cell=1, gap=0, x0=0, y0=0, opacity=255):
    d = _abi.LtPanelDesc()
    d.nsignals, d.cell, d.gap, d.x0, d.y0, d.opacity = nsignals, cell, gap, x0, y0, opacity
    return d


def test_header_row_and_constants():
    rows = [r for r in _abi.HEADERS if r[1] == "lt_tactile_panel.h"]
    assert len(rows) == 1 and rows[0][0] == "TACTILE_PANEL" and rows[0][3] == ("lt_tactile_panel_launches",)
    assert set(_abi.TACTILE_PANEL_SIGNATURES) == {"lt_tactile_panel_size", "lt_tactile_panel_draw", "lt_tactile_panel_launches"}
    assert _abi.CONSTS["LT_ABI_VERSION"] == 21
    P = _abi.TACTILE_PANEL_CONSTS
    assert P["LT_PANEL_VIEWS_PER_LAUNCH"] == _abi.CONSTS["LT_RENDER_VIEWS_PER_LAUNCH"]
    assert P["LT_PANEL_TAXELS"] == _abi.CONSTS["LT_TACTILE_ROWS"] * _abi.CONSTS["LT_TACTILE_COLS"]
    assert (P["LT_PANEL_MAX_CELL"], P["LT_PANEL_MAX_GAP"], P["LT_PANEL_MAX_CHANNELS"], P["LT_PANEL_MAX_SIGNALS"]) == (32, 16, 4, 4)
    lib = _abi.load()
    for name in _abi.TACTILE_PANEL_SIGNATURES:
        assert hasattr(lib, name)


@pytest.mark.parametrize("cell", [1, 3, 32])
def test_size_matches_the_twin(cell):
    lib = _abi.load()
    for gap in (0, 2, 16):
        for n in range(1, 5):
            for channels in itertools.product(range(1, 5), repeat=n):
                w, h = ctypes.c_int(), ctypes.c_int()
                _abi.call("lt_tactile_panel_size", _desc(n, cell, gap), _signals(channels), ctypes.byref(w), ctypes.byref(h))
                assert (w.value, h.value) == T.panel_size(cell, gap, channels), (cell, gap, channels)
                assert lib.lt_tactile_panel_launches(ctypes.byref(_desc(n, cell, gap)), _signals(channels), 2) == 1
    assert R.panel_size(R.TactilePanel(cell=cell, gap=2), [2, 2, 4, 4]) == T.panel_size(cell, 2, [2, 2, 4, 4])


def _draw(desc, signals, env_ids=(2, 0), nviews=None, rgba=FAKE, width=101, height=67):
    ids = (ctypes.c_int32 * max(1, len(env_ids)))(*env_ids)
    _abi.call("lt_tactile_panel_draw", desc, signals, ids, len(env_ids) if nviews is None else nviews, rgba, width, height, None)


REFUSALS = {
    "cell 0": (lambda: _draw(_desc(1, cell=0), _signals([2])), "desc.cell must be in 1 ... 32"),
    "cell 33": (lambda: _draw(_desc(1, cell=33), _signals([2])), "desc.cell must be in 1 ... 32"),
    "gap -1": (lambda: _draw(_desc(1, gap=-1), _signals([2])), "desc.gap must be in 0 ... 16"),
    "gap 17": (lambda: _draw(_desc(1, gap=17), _signals([2])), "desc.gap must be in 0 ... 16"),
    "channels 0": (lambda: _draw(_desc(2), _signals([2, 0])), r"signals\[1\].channels must be in 1 ... 4"),
    "channels 5": (lambda: _draw(_desc(1), _signals([5])), r"signals\[0\].channels must be in 1 ... 4"),
    "no signals": (lambda: _draw(_desc(0), _signals([2])), "desc.nsignals must be in 1 ... 4"),
    "five signals": (lambda: _draw(_desc(5), _signals([1] * 5)), "desc.nsignals must be in 1 ... 4"),
    "null signals": (lambda: _draw(_desc(1), None), "signals must be non-null"),
    "stride": (lambda: _draw(_desc(2), _signals([2, 4], stride=883)), r"signals\[1\].row_stride must be at least channels \* 221"),
    "opacity": (lambda: _draw(_desc(1, opacity=256), _signals([2])), "desc.opacity must be in 0 ... 255"),
    "map": (lambda: _draw(_desc(1), _with_map(_signals([2]), 7)), r"signals\[0\].maps must be LT_PANEL_MAP_BINARY or LT_PANEL_MAP_RAMP"),
    "too wide": (lambda: _draw(_desc(1, x0=101 - 28 + 1), _signals([2])), r"desc.x0 must be in 0 ... width - 28"),
    "too high": (lambda: _draw(_desc(1, y0=67 - 19 + 1), _signals([2])), r"desc.y0 must be in 0 ... height - 19"),
    "negative x0": (lambda: _draw(_desc(1, x0=-1), _signals([2])), "desc.x0 must be in 0"),
    "negative y0": (lambda: _draw(_desc(1, y0=-1), _signals([2])), "desc.y0 must be in 0"),
    "frame too small": (lambda: _draw(_desc(1, cell=8), _signals([2]), width=101), "desc.x0 must be in 0"),
    "null rgba": (lambda: _draw(_desc(1), _signals([2]), rgba=None), "rgba must be non-null and 4-byte aligned"),
    "misaligned rgba": (lambda: _draw(_desc(1), _signals([2]), rgba=FAKE + 2), "rgba must be non-null and 4-byte aligned"),
    "null rows": (lambda: _draw(_desc(1), _signals([2], rows=None)), r"signals\[0\].rows must be non-null and 4-byte aligned"),
    "misaligned rows": (lambda: _draw(_desc(1), _signals([2], rows=FAKE + 1)), r"signals\[0\].rows must be non-null and 4-byte aligned"),
    "nviews 0": (lambda: _draw(_desc(1), _signals([2]), nviews=0), "nviews must be in 1 ... 32"),
    "nviews -1": (lambda: _draw(_desc(1), _signals([2]), nviews=-1), "nviews must be in 1 ... 32"),
    "nviews 33": (lambda: _draw(_desc(1), _signals([2], n_envs=64), env_ids=tuple(range(33))), "nviews must be in 1 ... 32"),
    "negative env": (lambda: _draw(_desc(1), _signals([2]), env_ids=(0, -1)), r"env_ids\[1\] must be non-negative"),
    "env beyond n_envs": (lambda: _draw(_desc(1), _signals([2], n_envs=3), env_ids=(3,)), r"env_ids\[0\] must be below signals\[0\].n_envs = 3"),
    "width": (lambda: _draw(_desc(1), _signals([2]), width=0), "width must be in 1 ... 8192"),
    "height": (lambda: _draw(_desc(1), _signals([2]), height=8193), "height must be in 1 ... 8192"),
}


def _with_map(signals, m):
    signals[0].maps[1] = m
    return signals


@pytest.mark.parametrize("case", list(REFUSALS))
def test_draw_refuses_by_field_name_before_any_launch(case):
    call, field = REFUSALS[case]
    # LT_EINVAL (-22), not LT_EHIP: the refusal comes from the host-side check, in front of the launch (which has no device here)
    with pytest.raises(RuntimeError, match=r"code -22: lt_tactile_panel_draw: invalid argument: " + field):
        call()


def test_size_and_launches_refuse_too():
    lib = _abi.load()
    w, h = ctypes.c_int(), ctypes.c_int()
    with pytest.raises(RuntimeError, match="lt_tactile_panel_size: invalid argument: desc.cell must be in 1 ... 32"):
        _abi.call("lt_tactile_panel_size", _desc(1, cell=40), _signals([2]), ctypes.byref(w), ctypes.byref(h))
    with pytest.raises(RuntimeError, match="lt_tactile_panel_size: invalid argument: width must be non-null"):
        _abi.call("lt_tactile_panel_size", _desc(1), _signals([2]), None, ctypes.byref(h))
    assert lib.lt_tactile_panel_launches(ctypes.byref(_desc(1, gap=99)), _signals([2]), 1) == _abi.CONSTS["LT_EINVAL"]
    assert b"lt_tactile_panel_launches: invalid argument: desc.gap" in lib.lt_last_error()
    assert lib.lt_tactile_panel_launches(ctypes.byref(_desc(1)), _signals([2]), 33) == _abi.CONSTS["LT_EINVAL"]
    with pytest.raises(TypeError, match="lt_tactile_panel_launches"):  # a value query is not a status
        _abi.call("lt_tactile_panel_launches", _desc(1), _signals([2]), 1)


# ---- the Python front ----
def _bare_env(task, tactile, device="cpu"):
    """A LocoTouchVecEnv that was never constructed (its constructor needs a device): the attributes draw_tactile_panel looks at."""
    import torch
    from locotouch_amd.env import LocoTouchVecEnv

    env = object.__new__(LocoTouchVecEnv)
    env.task, env.tactile, env.device = task, tactile, torch.device(device)
    env.cfg = _abi.preset_cfg(task, num_envs=4)
    env.obs_tactile = torch.zeros(4, 442) if tactile else None
    env.obs_tactile_original = env.obs_tactile_processed = None
    return env


def test_python_front_refuses_a_cpu_env_and_a_task_without_tactile():
    import torch

    student = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"
    teacher = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
    frame = torch.zeros(1, 67, 101, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="draw_tactile_panel needs a HIP device"):  # no fall-back
        _bare_env(student, True).draw_tactile_panel(frame, [0])
    with pytest.raises(RuntimeError, match="draw_tactile_panel needs a HIP device"):
        _bare_env(student, True).draw_tactile_panel(frame, [0], signals={"policy": torch.zeros(4, 442)})
    with pytest.raises(ValueError, match=teacher):
        _bare_env(teacher, False).draw_tactile_panel(frame, [0])
    if not torch.cuda.is_available():
        from locotouch_amd.env import LocoTouchVecEnv

        with pytest.raises(RuntimeError, match="HIP device"):
            LocoTouchVecEnv(student, num_envs=4, device="cpu")
    assert frame.eq(0).all()


def test_video_tactile_flag_is_refused_by_name_for_tasks_without_tactile():
    from locotouch_amd.video import add_video_args, recorder_for, refuse_video_tactile

    ap = argparse.ArgumentParser()
    ap.add_argument("--video", action="store_true")
    add_video_args(ap)
    assert ap.parse_args([]).video_tactile is False and ap.parse_args(["--video", "--video_tactile"]).video_tactile is True
    on = ap.parse_args(["--video", "--video_tactile"])
    refuse_video_tactile(ap.parse_args(["--video"]), "Isaac-Locomotion-LocoTouch-v1")  # without the flag: nothing
    refuse_video_tactile(on, "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-Play-v1")
    for task in ("Isaac-Locomotion-LocoTouch-v1", "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"):
        with pytest.raises(ValueError, match=rf"--video_tactile: task '{task}' has no tactile observation group"):
            refuse_video_tactile(on, task)
        with pytest.raises(ValueError, match=rf"--video_tactile: task '{task}'"):
            recorder_for(_bare_env(task, False), on, "unused-folder")
    with pytest.raises(ValueError, match="--video_tactile draws into the frames --video records"):
        refuse_video_tactile(ap.parse_args(["--video_tactile"]), "Isaac-Locomotion-LocoTouch-v1")


def test_channel_maps_follow_the_tactile_format():
    C = _abi.CONSTS
    assert R.channel_maps(C["LT_TACTILE_BINARY"], 2) == [R.MAP_BINARY, R.MAP_BINARY]
    for fmt in ("LT_TACTILE_NORMALIZED", "LT_TACTILE_DISCRETE", "LT_TACTILE_CONTINUOUS"):
        assert R.channel_maps(C[fmt], 2) == [R.MAP_BINARY, R.MAP_RAMP]
    for fmt in ("LT_TACTILE_BINARY", "LT_TACTILE_PROCESSED", "LT_TACTILE_ORIGINAL"):
        assert R.channel_maps(C[fmt], 4) == [R.MAP_BINARY, R.MAP_RAMP, R.MAP_RAMP, R.MAP_RAMP]
    p = R.TactilePanel()
    assert (p.cell, p.gap, p.corner, p.margin, p.opacity) == (4, 2, "top-right", 8, 224)
    assert p.origin((222, 280), 640, 360) == (640 - 8 - 222, 8)
    assert R.TactilePanel(corner="bottom-left", margin=3).origin((10, 20), 100, 50) == (3, 50 - 3 - 20)
    with pytest.raises(ValueError, match="corner"):
        R.TactilePanel(corner="middle").origin((1, 1), 10, 10)
