"""include/lt_telemetry.h: a header of its own, bound by one row of `_abi.HEADERS`; the host-only size queries against the numpy twin;
every refusal of lt_telemetry_plan, lt_telemetry_record and lt_telemetry_chart_draw by its field's name, before anything is copied or
launched (no device is needed: the pointers here are made-up addresses that a refused call never follows); the launch-count queries;
and the refusals of the Python front."""
import argparse
import ctypes

import pytest

from locotouch_amd import _abi
from locotouch_amd import render as R
from tests import telemetry_ref as T

FAKE = 0x10000  # a 256-byte aligned address that is never dereferenced
C = _abi.TELEMETRY_CONSTS


def test_header_row_and_constants():
    rows = [r for r in _abi.HEADERS if r[1] == "lt_telemetry.h"]
    assert len(rows) == 1 and rows[0][0] == "TELEMETRY" and set(rows[0][3]) == {"lt_telemetry_record_launches", "lt_telemetry_chart_launches"}
    assert set(_abi.TELEMETRY_SIGNATURES) == {"lt_telemetry_plan_bytes", "lt_telemetry_plan", "lt_telemetry_record", "lt_telemetry_record_launches",
                                              "lt_telemetry_chart_size", "lt_telemetry_chart_draw", "lt_telemetry_chart_launches"}
    assert _abi.CONSTS["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67  # lt_env.h is as it was
    assert (C["LT_TELEMETRY_MAX_CHANNELS"], C["LT_TELEMETRY_MAX_ENVS"], C["LT_TELEMETRY_MAX_CAPACITY"]) == (64, 32, 1 << 20)
    assert (C["LT_CHART_MAX_PLOTS"], C["LT_CHART_MAX_SERIES"], C["LT_CHART_MIN_PLOT"], C["LT_CHART_MAX_PLOT_WIDTH"], C["LT_CHART_MAX_PLOT_HEIGHT"]) == (4, 4, 8, 1024, 256)
    assert C["LT_CHART_VIEWS_PER_LAUNCH"] == _abi.CONSTS["LT_RENDER_VIEWS_PER_LAUNCH"]
    colours = [C[k] for k in C if k.startswith("LT_CHART_COLOR_")]
    assert len(colours) == 8 and all(0 <= c <= 0xFFFFFF for c in colours) and len({C[f"LT_CHART_COLOR_SERIES_{s}"] for s in range(4)}) == 4
    ch = _abi.LtTelemetryChannel
    assert [(n, getattr(ch, n).offset) for n, _ in ch._fields_] == [("base", 0), ("dtype", 8), ("env_stride", 16), ("offset", 24)] and ctypes.sizeof(ch) == 32
    sig = _abi.TELEMETRY_SIGNATURES
    assert sig["lt_telemetry_record"][1] == [ctypes.c_void_p] * 4
    assert sig["lt_telemetry_plan"][1][1:] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert sig["lt_telemetry_chart_draw"][1][1:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib = _abi.load()
    for name in sig:
        assert hasattr(lib, name)


def test_plan_bytes_and_chart_size_match_the_formulas():
    n = ctypes.c_size_t()
    for nch in (1, 2, 5, 63, 64):
        for nenvs in (1, 3, 4, 5, 31, 32):
            _abi.call("lt_telemetry_plan_bytes", nch, nenvs, ctypes.byref(n))
            assert n.value == T.plan_bytes(nch, nenvs) == 16 + 16 * ((nenvs + 3) // 4) + 32 * nch
    w, h = ctypes.c_int(), ctypes.c_int()
    for nplots in (1, 2, 3, 4):
        for pw, ph, gap in ((8, 8, 0), (240, 48, 2), (1024, 256, 16), (9, 255, 1)):
            _abi.call("lt_telemetry_chart_size", _desc(nplots, pw, ph, gap), ctypes.byref(w), ctypes.byref(h))
            assert (w.value, h.value) == T.chart_size(nplots, pw, ph, gap) == (2 + pw, 2 + nplots * ph + (nplots - 1) * gap)
    chart = R.TelemetryChart(plots=R.DEFAULT_CHART_PLOTS)
    assert R.chart_size(chart) == T.chart_size(3, 240, 48, 2)


# ---- the plan ----
def _channels(n=1, base=FAKE, dtype=0, env_stride=4, offset=0):
    arr = (_abi.LtTelemetryChannel * max(1, n))()
    for ch in arr:
        ch.base, ch.dtype, ch.env_stride, ch.offset = base, dtype, env_stride, offset
    return arr


def _plan(channels=None, nchannels=None, env_ids=(0, 3), nenvs=None, capacity=16, device_plan=FAKE, nbytes=1 << 16):
    channels = _channels() if channels is None else channels
    ids = None if env_ids is None else (ctypes.c_int32 * max(1, len(env_ids)))(*env_ids)
    _abi.call("lt_telemetry_plan", channels, len(channels) if nchannels is None else nchannels, ids,
              (len(env_ids) if env_ids is not None else 1) if nenvs is None else nenvs, capacity, device_plan, nbytes, None)


PLAN_REFUSALS = {
    "no channels": (lambda: _plan(nchannels=0), "nchannels must be in 1 ... 64"),
    "65 channels": (lambda: _plan(_channels(65)), "nchannels must be in 1 ... 64"),
    "no envs": (lambda: _plan(nenvs=0), "nenvs must be in 1 ... 32"),
    "33 envs": (lambda: _plan(env_ids=tuple(range(33))), "nenvs must be in 1 ... 32"),
    "capacity 0": (lambda: _plan(capacity=0), "capacity must be in 1 ... 1048576"),
    "capacity 2^20 + 1": (lambda: _plan(capacity=(1 << 20) + 1), "capacity must be in 1 ... 1048576"),
    "null channels": (lambda: _abi.call("lt_telemetry_plan", None, 1, (ctypes.c_int32 * 1)(0), 1, 16, FAKE, 1 << 16, None), "channels must be non-null"),
    "null env ids": (lambda: _plan(env_ids=None), "env_ids must be non-null"),
    "dtype 4": (lambda: _plan(_channels(2, dtype=4)), r"channels\[0\].dtype must be in 0 ... 3"),
    "dtype -1": (lambda: _plan(_channels(1, dtype=-1)), r"channels\[0\].dtype must be in 0 ... 3"),
    "null base": (lambda: _plan(_channels(3, base=None)), r"channels\[0\].base must be non-null and aligned to its element"),
    "misaligned f32": (lambda: _plan(_channels(1, base=FAKE + 2)), r"channels\[0\].base must be non-null and aligned to its element"),
    "misaligned i64": (lambda: _plan(_channels(1, base=FAKE + 4, dtype=1)), r"channels\[0\].base must be non-null and aligned to its element"),
    "misaligned i32": (lambda: _plan(_channels(1, base=FAKE + 1, dtype=3)), r"channels\[0\].base must be non-null and aligned to its element"),
    "negative stride": (lambda: _plan(_channels(1, env_stride=-1)), r"channels\[0\].env_stride must be non-negative"),
    "negative offset": (lambda: _plan(_channels(1, offset=-1)), r"channels\[0\].offset must be non-negative"),
    "negative env id": (lambda: _plan(env_ids=(0, -1)), r"env_ids\[1\] must be non-negative"),
    "null plan": (lambda: _plan(device_plan=None), "device_plan must be non-null and 16-byte aligned"),
    "misaligned plan": (lambda: _plan(device_plan=FAKE + 8), "device_plan must be non-null and 16-byte aligned"),
    "too few bytes": (lambda: _plan(nbytes=T.plan_bytes(1, 2) - 1), "bytes must be at least lt_telemetry_plan_bytes"),
}


@pytest.mark.parametrize("case", list(PLAN_REFUSALS))
def test_plan_refuses_by_field_name_before_the_copy(case):
    call, field = PLAN_REFUSALS[case]
    # LT_EINVAL (-22), not LT_EHIP: the refusal comes from the host-side check, in front of the copy (which has no device here)
    with pytest.raises(RuntimeError, match=r"code -22: lt_telemetry_plan: invalid argument: " + field):
        call()


def test_a_later_channel_is_named_by_its_index_and_u8_needs_no_alignment():
    chans = _channels(3)
    chans[2].dtype = 7
    with pytest.raises(RuntimeError, match=r"channels\[2\].dtype must be in 0 ... 3"):
        _plan(chans)
    chans = _channels(2, base=FAKE + 1, dtype=2)  # uint8: any address
    chans[1].dtype, chans[1].base = 1, FAKE + 12
    with pytest.raises(RuntimeError, match=r"channels\[1\].base must be non-null and aligned to its element"):
        _plan(chans)


def test_plan_bytes_refuses_too():
    n = ctypes.c_size_t()
    for nch, nenvs, field in ((0, 1, "nchannels"), (65, 1, "nchannels"), (1, 0, "nenvs"), (1, 33, "nenvs")):
        with pytest.raises(RuntimeError, match=rf"code -22: lt_telemetry_plan_bytes: invalid argument: {field} must be in 1"):
            _abi.call("lt_telemetry_plan_bytes", nch, nenvs, ctypes.byref(n))
    with pytest.raises(RuntimeError, match="lt_telemetry_plan_bytes: invalid argument: bytes must be non-null"):
        _abi.call("lt_telemetry_plan_bytes", 1, 1, None)


# ---- the record ----
RECORD_REFUSALS = {
    "null plan": ((None, FAKE, FAKE), "device_plan must be non-null and 16-byte aligned"),
    "misaligned plan": ((FAKE + 4, FAKE, FAKE), "device_plan must be non-null and 16-byte aligned"),
    "null ring": ((FAKE, None, FAKE), "ring must be non-null and 4-byte aligned"),
    "misaligned ring": ((FAKE, FAKE + 2, FAKE), "ring must be non-null and 4-byte aligned"),
    "null head": ((FAKE, FAKE, None), "head must be non-null and 8-byte aligned"),
    "misaligned head": ((FAKE, FAKE, FAKE + 4), "head must be non-null and 8-byte aligned"),
}


@pytest.mark.parametrize("case", list(RECORD_REFUSALS))
def test_record_refuses_by_field_name_before_the_launch(case):
    (plan, ring, head), field = RECORD_REFUSALS[case]
    with pytest.raises(RuntimeError, match=r"code -22: lt_telemetry_record: invalid argument: " + field):
        _abi.call("lt_telemetry_record", plan, ring, head, None)
    lib = _abi.load()
    assert lib.lt_telemetry_record_launches(plan, ring, head) == _abi.CONSTS["LT_EINVAL"]
    assert b"lt_telemetry_record_launches: invalid argument: " in lib.lt_last_error()


# ---- the chart ----
def _desc(nplots=1, pw=8, ph=8, gap=0, x0=0, y0=0, opacity=255, nseries=1, channel=0, k=1.0, y_zero=7):
    d = _abi.LtChartDesc()
    d.nplots, d.pw, d.ph, d.gap, d.x0, d.y0, d.opacity = nplots, pw, ph, gap, x0, y0, opacity
    for p in d.plots:
        p.nseries, p.k, p.y_zero = nseries, k, y_zero
        for s in range(4):
            p.channels[s] = channel
    return d


def _with_plot(d, index, **fields):
    for name, v in fields.items():
        setattr(d.plots[index], name, v)
    return d


def _draw(desc, ring=FAKE, head=FAKE, nenvs=2, nchannels=3, capacity=16, slots=(1, 0), nviews=None, rgba=FAKE, width=40, height=30):
    s = None if slots is None else (ctypes.c_int32 * max(1, len(slots)))(*slots)
    _abi.call("lt_telemetry_chart_draw", desc, ring, head, nenvs, nchannels, capacity, s, (len(slots) if slots is not None else 1) if nviews is None else nviews,
              rgba, width, height, None)


INF = float("inf")
CHART_REFUSALS = {
    "no plots": (lambda: _draw(_desc(0)), "desc.nplots must be in 1 ... 4"),
    "five plots": (lambda: _draw(_desc(5)), "desc.nplots must be in 1 ... 4"),
    "pw 7": (lambda: _draw(_desc(pw=7)), "desc.pw must be in 8 ... 1024"),
    "pw 1025": (lambda: _draw(_desc(pw=1025), capacity=4096, width=2048), "desc.pw must be in 8 ... 1024"),
    "ph 7": (lambda: _draw(_desc(ph=7)), "desc.ph must be in 8 ... 256"),
    "ph 257": (lambda: _draw(_desc(ph=257), height=1024), "desc.ph must be in 8 ... 256"),
    "gap -1": (lambda: _draw(_desc(gap=-1)), "desc.gap must be in 0 ... 16"),
    "gap 17": (lambda: _draw(_desc(gap=17)), "desc.gap must be in 0 ... 16"),
    "opacity": (lambda: _draw(_desc(opacity=256)), "desc.opacity must be in 0 ... 255"),
    "pw > capacity": (lambda: _draw(_desc(pw=17), capacity=16), "desc.pw must be at most capacity"),
    "no series": (lambda: _draw(_desc(2, nseries=0)), r"desc.plots\[0\].nseries must be in 1 ... 4"),
    "five series": (lambda: _draw(_with_plot(_desc(2), 1, nseries=5)), r"desc.plots\[1\].nseries must be in 1 ... 4"),
    "channel beyond": (lambda: _draw(_desc(channel=3), nchannels=3), r"desc.plots\[0\].channels must be in 0 ... nchannels - 1"),
    "negative channel": (lambda: _draw(_desc(channel=-1)), r"desc.plots\[0\].channels must be in 0 ... nchannels - 1"),
    "k inf": (lambda: _draw(_desc(k=INF)), r"desc.plots\[0\].k must be finite"),
    "k nan": (lambda: _draw(_desc(k=float("nan"))), r"desc.plots\[0\].k must be finite"),
    "y_zero": (lambda: _draw(_desc(y_zero=(1 << 30) + 1)), r"desc.plots\[0\].y_zero must be in -1073741824 ... 1073741824"),
    "no channels": (lambda: _draw(_desc(), nchannels=0), "nchannels must be in 1 ... 64"),
    "65 channels": (lambda: _draw(_desc(), nchannels=65), "nchannels must be in 1 ... 64"),
    "no envs": (lambda: _draw(_desc(), nenvs=0), "nenvs must be in 1 ... 32"),
    "33 envs": (lambda: _draw(_desc(), nenvs=33), "nenvs must be in 1 ... 32"),
    "capacity 0": (lambda: _draw(_desc(), capacity=0), "capacity must be in 1 ... 1048576"),
    "capacity 2^20 + 1": (lambda: _draw(_desc(), capacity=(1 << 20) + 1), "capacity must be in 1 ... 1048576"),
    "too wide": (lambda: _draw(_desc(x0=40 - 10 + 1)), r"desc.x0 must be in 0 ... width - 10"),  # the panel one pixel outside the frame
    "too high": (lambda: _draw(_desc(y0=30 - 10 + 1)), r"desc.y0 must be in 0 ... height - 10"),
    "negative x0": (lambda: _draw(_desc(x0=-1)), "desc.x0 must be in 0"),
    "negative y0": (lambda: _draw(_desc(y0=-1)), "desc.y0 must be in 0"),
    "frame too small": (lambda: _draw(_desc(3, ph=10), height=31), "desc.y0 must be in 0"),
    "null ring": (lambda: _draw(_desc(), ring=None), "ring must be non-null and 4-byte aligned"),
    "misaligned ring": (lambda: _draw(_desc(), ring=FAKE + 1), "ring must be non-null and 4-byte aligned"),
    "null head": (lambda: _draw(_desc(), head=None), "head must be non-null and 8-byte aligned"),
    "misaligned head": (lambda: _draw(_desc(), head=FAKE + 4), "head must be non-null and 8-byte aligned"),
    "null rgba": (lambda: _draw(_desc(), rgba=None), "rgba must be non-null and 4-byte aligned"),
    "misaligned rgba": (lambda: _draw(_desc(), rgba=FAKE + 2), "rgba must be non-null and 4-byte aligned"),
    "null slots": (lambda: _draw(_desc(), slots=None), "slots must be non-null"),
    "nviews 0": (lambda: _draw(_desc(), nviews=0), "nviews must be in 1 ... 32"),
    "nviews 33": (lambda: _draw(_desc(), nenvs=32, slots=tuple(range(32)) + (0,)), "nviews must be in 1 ... 32"),
    "negative slot": (lambda: _draw(_desc(), slots=(0, -1)), r"slots\[1\] must be in 0 ... nenvs - 1"),
    "slot beyond": (lambda: _draw(_desc(), nenvs=2, slots=(2,)), r"slots\[0\] must be in 0 ... nenvs - 1"),
    "width": (lambda: _draw(_desc(), width=0), "width must be in 1 ... 8192"),
    "height": (lambda: _draw(_desc(), height=8193), "height must be in 1 ... 8192"),
    "null desc": (lambda: _draw(None), "desc must be non-null"),
}


@pytest.mark.parametrize("case", list(CHART_REFUSALS))
def test_chart_draw_refuses_by_field_name_before_any_launch(case):
    call, field = CHART_REFUSALS[case]
    with pytest.raises(RuntimeError, match=r"code -22: lt_telemetry_chart_draw: invalid argument: " + field):
        call()


def test_the_panel_may_touch_the_frames_edge_but_not_cross_it():
    # (a fitting panel is not refused for its place: the call gets as far as the launch, which has no device in a CPU run - so only
    # the refusal one pixel further is looked at here, next to the largest origin the message names)
    with pytest.raises(RuntimeError, match=r"desc.x0 must be in 0 ... width - 10 "):
        _draw(_desc(x0=31, y0=20))
    with pytest.raises(RuntimeError, match=r"desc.y0 must be in 0 ... height - 10 "):
        _draw(_desc(x0=30, y0=21))


def test_size_and_launch_queries():
    lib = _abi.load()
    w, h = ctypes.c_int(), ctypes.c_int()
    with pytest.raises(RuntimeError, match="lt_telemetry_chart_size: invalid argument: desc.ph must be in 8 ... 256"):
        _abi.call("lt_telemetry_chart_size", _desc(ph=300), ctypes.byref(w), ctypes.byref(h))
    with pytest.raises(RuntimeError, match="lt_telemetry_chart_size: invalid argument: height must be non-null"):
        _abi.call("lt_telemetry_chart_size", _desc(), ctypes.byref(w), None)
    _abi.call("lt_telemetry_chart_size", _desc(opacity=999, k=INF), ctypes.byref(w), ctypes.byref(h))  # only the sizes are looked at
    assert lib.lt_telemetry_record_launches(FAKE, FAKE, FAKE) == 1
    assert lib.lt_telemetry_chart_launches(ctypes.byref(_desc(3, 240, 48, 2)), 2, 36, 4096, 1) == 1
    assert lib.lt_telemetry_chart_launches(ctypes.byref(_desc(4, 1024, 256, 16, nseries=4)), 32, 64, 1 << 20, 32) == 1
    assert lib.lt_telemetry_chart_launches(ctypes.byref(_desc(pw=17)), 2, 3, 16, 1) == _abi.CONSTS["LT_EINVAL"]
    assert b"lt_telemetry_chart_launches: invalid argument: desc.pw must be at most capacity" in lib.lt_last_error()
    assert lib.lt_telemetry_chart_launches(ctypes.byref(_desc()), 2, 3, 16, 33) == _abi.CONSTS["LT_EINVAL"]
    for name, args in (("lt_telemetry_record_launches", (FAKE, FAKE, FAKE)), ("lt_telemetry_chart_launches", (_desc(), 2, 3, 16, 1))):
        with pytest.raises(TypeError, match=name):  # a value query is not a status
            _abi.call(name, *args)


# ---- the Python front ----
def test_chart_scale_and_default_chart():
    import numpy as np

    chart = R.default_chart(640, 360)
    assert (chart.pw, chart.ph, chart.gap, chart.corner, chart.margin, chart.opacity) == (240, 48, 2, "bottom-left", 8, 224)
    assert [p[1] for p in chart.plots] == [(-1.6, 1.6), (0.0, 150.0), (-0.1, 0.1)] and [len(p[0]) for p in chart.plots] == [3, 4, 1]
    k, y_zero = chart.scale(-1.5, 1.5)
    assert k == float(np.float32(47 / 3.0)) and y_zero == round(1.5 * k) == 24  # 23.5 up to float32's error in k: above
    assert chart.scale(0.0, 150.0) == (float(np.float32(47 / 150.0)), 47)  # value 0 on the bottom row
    assert chart.origin(R.chart_size(chart), 640, 360) == (8, 360 - 8 - 150)
    small = R.default_chart(160, 90)
    w, h = R.chart_size(small)
    assert (small.pw, small.ph) == (60, 10) and w + 8 <= 160 and h + 8 <= 90
    names = ["reward", "cmd.vx", "cmd.vy", "cmd.wz"] + [f"foot_force.{leg}" for leg in ("FR", "FL", "RR", "RL")]
    d = R.chart_desc(chart, names, 8, 202)
    assert (d.nplots, d.pw, d.ph, d.gap, d.x0, d.y0, d.opacity) == (3, 240, 48, 2, 8, 202, 224)
    assert [d.plots[0].channels[s] for s in range(3)] == [1, 2, 3] and d.plots[1].nseries == 4 and d.plots[2].channels[0] == 0
    with pytest.raises(ValueError, match="channel 'reward' is not recorded"):
        R.chart_desc(chart, names[1:])
    with pytest.raises(ValueError, match="lo < hi"):
        chart.scale(1.0, 1.0)
    with pytest.raises(ValueError, match="1 ... 4 channels"):
        R.chart_desc(R.TelemetryChart(plots=((tuple(names[:5]), (0, 1)),)), names)


def test_channel_names_resolve_by_group_and_unknown_ones_are_refused_with_the_list():
    from locotouch_amd.telemetry import DEFAULT_CHANNELS, resolve_names

    known = ["cmd.vx", "cmd.vy", "cmd.wz", "reward", "reward_term.alive", "dones"]
    assert resolve_names(known, ["reward", "cmd", "cmd.vx"]) == ["reward", "cmd.vx", "cmd.vy", "cmd.wz"]
    assert resolve_names(known, ["reward_term"]) == ["reward_term.alive"]
    with pytest.raises(ValueError, match=r"unknown telemetry channel 'cmd.v'; known groups: cmd, dones, reward, reward_term; known channels: cmd.vx, cmd.vy"):
        resolve_names(known, ["cmd.v"])
    assert DEFAULT_CHANNELS == ("cmd", "joint_pos", "applied_torque", "foot_force", "obj_pos", "reward", "dones")


def test_flags_and_refusals_of_the_python_front():
    import torch

    from locotouch_amd.env import LocoTouchVecEnv
    from locotouch_amd.telemetry import Telemetry, add_telemetry_args, telemetry_for
    from locotouch_amd.video import add_video_args, recorder_for, refuse_video_telemetry

    ap = argparse.ArgumentParser()
    ap.add_argument("--video", action="store_true")
    add_video_args(ap)
    add_telemetry_args(ap)
    off = ap.parse_args([])
    assert (off.video_telemetry, off.telemetry, off.telemetry_envs, off.telemetry_capacity) == (False, False, "0", 4096)
    assert off.telemetry_channels == "cmd,joint_pos,applied_torque,foot_force,obj_pos,reward,dones"
    on = ap.parse_args(["--video", "--video_telemetry", "--telemetry", "--telemetry_envs", "0,3"])
    assert on.video_telemetry and on.telemetry and on.telemetry_envs == "0,3"
    refuse_video_telemetry(off)
    refuse_video_telemetry(on)
    with pytest.raises(ValueError, match="--video_telemetry draws into the frames --video records"):
        refuse_video_telemetry(ap.parse_args(["--video_telemetry"]))
    env = object.__new__(LocoTouchVecEnv)  # never constructed (its constructor needs a device): the attributes the front looks at
    env.device, env.step_dt = torch.device("cpu"), 0.02
    assert env.telemetry is None and env.recorder is None  # the hooks: class attributes, off
    assert telemetry_for(env, off) is None and env.telemetry is None  # without the flags nothing is built
    with pytest.raises(ValueError, match="--video_telemetry: recorder_for needs the telemetry.Telemetry"):
        recorder_for(env, on, "unused-folder")
    with pytest.raises(RuntimeError, match="Telemetry needs a HIP device"):  # no fall-back
        Telemetry(env, {"x": (torch.zeros(4, 2), 0)})
    with pytest.raises(RuntimeError, match="draw_telemetry_chart needs a HIP device"):
        env.draw_telemetry_chart(torch.zeros(1, 30, 40, dtype=torch.int32), [0], None)
