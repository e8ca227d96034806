"""GPU tests of the telemetry ring and its strip charts (csrc/lt_telemetry.hip) against the numpy twin (tests/telemetry_ref.py), bit for
bit: a record is a copy with a conversion by value and the chart is integer behind one correctly rounded float32 product, so there is
no tolerance anywhere.  Then the Python front: `Telemetry` on a real env's arena channels, the `env.telemetry` hook, and
`recorder_for(..., --video_telemetry)`."""
import argparse
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TEACHER = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
N = 48
GUARD = 64  # words in front of and behind the frames


class _Env:
    """What Telemetry looks at of an env, for channels that are all the caller's own tensors."""
    device, step_dt = DEV, 0.02

    def telemetry_channels(self):
        return {}


# ---- record ----
def _sources(rng):
    """Host arrays of the four dtypes, N rows each: a wider f32 tensor (its columns are strided), a quad field [N, 3, 4] laid out as the
    arena lays it out (storage [3][N][4]), i64 values that do not fit a float, u8, and i32 pairs."""
    return {"wide": rng.standard_normal((N, 7)).astype(np.float32),
            "quad": rng.standard_normal((3, N, 4)).astype(np.float32),
            "i64": (2 ** 24 + rng.integers(-5, 2 ** 20, size=N)).astype(np.int64) * rng.choice([-1, 1], size=N),
            "u8": rng.integers(0, 256, size=N).astype(np.uint8),
            "i32": rng.integers(-2 ** 31, 2 ** 31, size=(N, 2)).astype(np.int32)}


# every (source, index into a row) the sources offer: 7 + 12 + 1 + 1 + 2 = 23 distinct channels
POOL = [("wide", (c,)) for c in range(7)] + [("quad", (q, lane)) for q in range(3) for lane in range(4)] + [("i64", ()), ("u8", ()), ("i32", (0,)), ("i32", (1,))]
PICK = {1: [3], 5: [3, 13, 19, 20, 22], 64: [(7 * i + 3) % 23 for i in range(64)]}  # 5: one of each kind; 64: repeats, every kind


def _device_sources(host):
    import torch

    dev = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
    views = dict(dev)
    views["quad"] = dev["quad"].permute(1, 0, 2)  # [N, 3, 4] with strides (4, 4 N, 1): component c = q * 4 + lane
    assert views["quad"].stride() == (4, 4 * N, 1)
    return dev, views


def _host_value(host, name, index, env):
    a = host[name]
    return a[index[0], env, index[1]] if name == "quad" else a[(env,) + tuple(index)]


@pytest.mark.parametrize("env_ids", [(0,), (5, 0, 47)])
@pytest.mark.parametrize("nchannels", [1, 5, 64])
def test_record_matches_the_twin_after_every_record(env_ids, nchannels):
    import torch

    from locotouch_amd import _abi
    from locotouch_amd.telemetry import Telemetry
    from tests import telemetry_ref as T

    rng = np.random.default_rng(11)
    host = _sources(rng)
    dev, views = _device_sources(host)
    chosen = [POOL[i] for i in PICK[nchannels]]
    tel = Telemetry(_Env(), {f"c{i}": (views[name], index) for i, (name, index) in enumerate(chosen)}, env_ids=env_ids, capacity=4)
    assert _abi.load().lt_telemetry_record_launches(tel.plan.data_ptr(), tel.ring.data_ptr(), tel.head.data_ptr()) == 1
    twin = T.Ring(nchannels, len(env_ids), 4)
    for t in range(11):  # capacity 4: wraps twice
        fresh = _sources(rng)
        for k in host:
            host[k] = fresh[k]
            dev[k].copy_(torch.from_numpy(fresh[k]))
        tel.record()
        twin.record([[_host_value(host, name, index, e) for name, index in chosen] for e in env_ids])
        torch.cuda.synchronize()
        assert np.array_equal(tel.head.cpu().numpy(), twin.head), t
        assert np.array_equal(tel.ring.cpu().numpy().view(np.uint32), twin.ring.view(np.uint32)), t
    assert tel.count == 11 and np.array_equal(tel.read().cpu().numpy(), twin.read())
    tel.reset()
    torch.cuda.synchronize()
    assert tel.count == 0 and tel.read().shape == (0, len(env_ids), nchannels)


def test_a_captured_record_advances_with_every_replay():
    import torch

    from locotouch_amd.telemetry import Telemetry
    from tests import telemetry_ref as T

    src = torch.zeros(N, 3, device=DEV)
    tel = Telemetry(_Env(), {"a": (src, 0), "b": (src, 2)}, env_ids=(47, 1), capacity=8)
    twin = T.Ring(2, 2, 8)

    def fill(t):
        values = torch.arange(N * 3, dtype=torch.float32).reshape(N, 3) * (t + 1) + 0.5
        src.copy_(values)
        return [[values[e, 0].item(), values[e, 2].item()] for e in (47, 1)]

    twin.record(fill(0))
    tel.record()  # eager
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            tel.record()  # the graph's only node
    torch.cuda.synchronize()
    assert tel.count == 1  # a capture launches nothing
    for t in range(1, 4):
        twin.record(fill(t))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(tel.head.cpu().numpy(), twin.head)
    assert tel.count == 4 and np.array_equal(tel.ring.cpu().numpy(), twin.ring)


# ---- chart ----
def _pattern(v, h, w):
    """Per-pixel pattern, every byte in use (the alpha byte too), between guard words."""
    idx = np.arange(2 * GUARD + v * h * w, dtype=np.uint64)
    return ((idx * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _chart_ring(capacity, nenvs, nchannels, count, pw):
    """A ring as `count` records left it (every slot written where count >= capacity; the rest zero), with integer values in channel 0
    (ties under k = 0.5) and the special values planted among the newest pw records of every env."""
    rng = np.random.default_rng(5)
    ring = np.zeros((capacity, nenvs, nchannels), dtype=np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 30, 1e9, -1e9, -0.0, 0.5, 1.5, 2.5], dtype=np.float32)
    for rec in range(max(0, count - capacity), count):
        ring[rec % capacity] = (4.0 * rng.standard_normal((nenvs, nchannels))).astype(np.float32)
        ring[rec % capacity, :, 0] = rng.integers(-12, 13, size=nenvs)
    newest = [rec % capacity for rec in range(max(0, count - pw), count)]
    for i, slot in enumerate(newest[2::3]):
        ring[slot, i % nenvs, (i // nenvs) % nchannels] = special[i % special.size]
    return ring


SMALL, LARGE = (40, 30), (96, 64)
# (frame, plots as (channels, k, y_zero), pw, ph, gap, count: "short" < pw / "exact" == pw / "wrapped", opacity, where)
ONE = [([1], 1.0, 6)]
ONE_OF_FOUR = [([0, 1, 2, 3], 0.5, 5)]
THREE = [([0], 0.5, 8), ([1, 2, 3, 4], 1.25, 8), ([4, 0, 2, 1], 3.0, 30)]  # the third: the row of 0 below the plot
CHART_CASES = [(SMALL, ONE, 16, 12, 0, "short", 255, "origin"), (SMALL, ONE, 16, 12, 0, "exact", 128, "flush"),
               (SMALL, ONE_OF_FOUR, 38, 12, 0, "wrapped", 255, "flush"), (SMALL, ONE_OF_FOUR, 9, 26, 0, "wrapped", 0, "inside"),
               (LARGE, THREE, 70, 17, 2, "short", 128, "flush"), (LARGE, THREE, 70, 17, 2, "exact", 255, "origin"),
               (LARGE, THREE, 70, 17, 2, "wrapped", 128, "inside"), (LARGE, THREE, 94, 20, 1, "wrapped", 255, "flush"),
               (LARGE, ONE, 64, 8, 0, "wrapped", 0, "flush")]


@pytest.mark.parametrize("size,plots,pw,ph,gap,count,opacity,where", CHART_CASES)
def test_chart_matches_the_twin_bit_for_bit(size, plots, pw, ph, gap, count, opacity, where):
    import torch

    from locotouch_amd import _abi
    from tests import telemetry_ref as T

    w, h = size
    nenvs, nchannels, slots = 3, 5, [2, 0]  # two views with different slots
    capacity = pw + 3
    count = {"short": pw - 5, "exact": pw, "wrapped": 2 * capacity + 5}[count]
    ring = _chart_ring(capacity, nenvs, nchannels, count, pw)
    cw, ch = T.chart_size(len(plots), pw, ph, gap)
    x0, y0 = {"origin": (0, 0), "flush": (w - cw, h - ch), "inside": (1, 1)}[where]
    v = len(slots)
    pattern = _pattern(v, h, w)
    frames = pattern[GUARD:-GUARD].reshape(v, h, w)
    want = T.chart(frames, ring, count, slots, plots, pw, ph, gap, x0, y0, opacity)

    d = _abi.LtChartDesc()
    d.nplots, d.pw, d.ph, d.gap, d.x0, d.y0, d.opacity = len(plots), pw, ph, gap, x0, y0, opacity
    for plot, (channels, k, y_zero) in zip(d.plots, plots):
        plot.nseries, plot.k, plot.y_zero = len(channels), k, y_zero
        for s, c in enumerate(channels):
            plot.channels[s] = c
    assert _abi.load().lt_telemetry_chart_launches(ctypes.byref(d), nenvs, nchannels, capacity, v) == 1
    buf = torch.from_numpy(pattern.view(np.int32).copy()).to(DEV)
    dring = torch.from_numpy(ring).to(DEV)
    head = torch.tensor([count, count % capacity], dtype=torch.int64, device=DEV)
    _abi.call("lt_telemetry_chart_draw", d, dring, head, nenvs, nchannels, capacity, (ctypes.c_int32 * v)(*slots), v, buf[GUARD:GUARD + v * h * w], w, h,
              _abi.stream(torch.device(DEV)))
    torch.cuda.synchronize()
    words = buf.cpu().numpy().view(np.uint32)
    got = words[GUARD:-GUARD].reshape(v, h, w)
    assert np.array_equal(got, want), int((got != want).sum())
    # every guard word and every pixel outside the rectangle is the pattern's (this does not go through the twin)
    assert np.array_equal(words[:GUARD], pattern[:GUARD]) and np.array_equal(words[-GUARD:], pattern[-GUARD:])
    outside = np.ones((v, h, w), bool)
    outside[:, y0:y0 + ch, x0:x0 + cw] = False
    assert np.array_equal(got[outside], frames[outside])
    assert np.array_equal(head.cpu().numpy(), [count, count % capacity]) and np.array_equal(dring.cpu().numpy().view(np.uint32), ring.view(np.uint32))
    inside = got[:, y0:y0 + ch, x0:x0 + cw]
    if opacity == 0:  # the frame shows through: only the alpha byte is set
        assert np.array_equal(inside & 0xFFFFFF, frames[:, y0:y0 + ch, x0:x0 + cw] & 0xFFFFFF)
    else:  # which env slot a view shows matters
        assert not np.array_equal(T.chart(frames, ring, count, slots[::-1], plots, pw, ph, gap, x0, y0, opacity), want)
    if opacity == 255:  # the panel's own colours: a line is in sight
        assert np.isin(inside[0], [c | 255 << 24 for c in T.SERIES]).any()


# ---- the Python front on a real env ----
def _teacher(n=16, **kw):
    from locotouch_amd.env import make

    return make(TEACHER, num_envs=n, device=DEV, seed=3, **kw)


# twelve arena channels, each with the view and the index it must come from, written out by hand (include/lt_layout.h: component
# c = quad * 4 + lane; joints: quad = link type, lane = leg FR FL RR RL; LT_F_FORCE_HIST: quad = slot * 4 + type, newest slot 0)
TWELVE = {"cmd.vx": ("LT_F_CMD", (0, 0)), "joint_pos.FR_hip": ("LT_F_JOINT_POS", (0, 0)), "joint_pos.RL_calf": ("LT_F_JOINT_POS", (2, 3)),
          "applied_torque.FL_thigh": ("LT_F_APPLIED_TORQUE", (1, 1)), "foot_force.RL": ("LT_F_FORCE_HIST", (3, 3)),
          "foot_pos_w.RR_z": ("LT_F_FOOT_POS_W", (2, 2)), "obj_pos.z": ("LT_F_OBJ_POS", (0, 2)), "reward": ("LT_F_REWARD", ()),
          "dones": ("LT_F_DONES", ()), "time_out": ("LT_F_TIME_OUT", ()), "term_bits": ("LT_F_TERM_BITS", ()), "ep_len": ("LT_F_EP_LEN", ())}


def test_env_hook_records_the_arena_views_bit_for_bit():
    import torch

    from locotouch_amd.telemetry import Telemetry

    env = _teacher()
    known = env.telemetry_channels()
    for name in ("root_pos.x", "root_quat.w", "root_lin_vel_w.z", "root_ang_vel_w.y", "joint_vel.RR_thigh", "action.FL_calf", "cmd.wz", "foot_force.FR",
                 "foot_pos_w.FL_x", "obj_quat.z", "obj_lin_vel_w.x", "reward_term.alive", "reward_term.object_dangerous_state", *TWELVE):
        assert name in known, name
    assert len(known) == 3 + 4 + 3 + 3 + 4 * 12 + 3 + 4 + 12 + 3 + 4 + 3 + 1 + 25 + 4 and not any(k.startswith("contact_force_w") for k in known)
    ids = (0, 7)
    tel = Telemetry(env, {n: n for n in TWELVE}, env_ids=ids, capacity=8)
    assert env.telemetry is None
    env.telemetry = tel
    g = torch.Generator(device="cpu").manual_seed(0)
    kept = []
    for _ in range(6):
        env.step((0.5 * torch.randn(16, 12, generator=g)).to(DEV))
        kept.append(torch.stack([env.field(f)[(slice(None),) + idx][list(ids)].clone().to(torch.float32) for f, idx in TWELVE.values()], dim=1))
    got = tel.read()
    assert tel.count == 6 and got.shape == (6, 2, 12)
    assert torch.equal(got, torch.stack(kept))
    assert bool((got[:, :, list(TWELVE).index("ep_len")] > 0).any()) and bool((got[:, :, 1] != 0).all())  # (not a ring of zeros)
    env.telemetry = None
    for _ in range(3):
        env.step(torch.zeros(16, 12, device=DEV))
    torch.cuda.synchronize()
    assert tel.head.tolist() == [6, 6] and torch.equal(tel.read(), got)  # with None nothing is called
    with pytest.raises(ValueError, match="unknown telemetry channel 'cmd.v'; known groups: "):
        Telemetry(env, {"x": "cmd.v"})
    with pytest.raises(ValueError, match="env ids .* do not all lie below"):
        Telemetry(env, {"x": "cmd.vx"}, env_ids=(0, 16))
    with pytest.raises(TypeError, match="channel 'h' is torch.float16; float32, int32, int64 and uint8"):
        Telemetry(env, {"h": (torch.zeros(16, 2, device=DEV, dtype=torch.float16), 0)})
    with pytest.raises(RuntimeError, match="lt_telemetry_plan_bytes: invalid argument: nenvs must be in 1 ... 32"):
        Telemetry(env, {"x": "cmd.vx"}, env_ids=())


def test_contact_force_channels_when_bound_and_save(tmp_path):
    import torch

    from locotouch_amd.telemetry import Telemetry

    env = _teacher(contact_force_vectors=True)
    known = env.telemetry_channels()
    forces = [k for k in known if k.startswith("contact_force_w.")]
    assert len(forces) == 4 * 12 + 6 and "contact_force_w.RL_foot_z" in forces and "contact_force_w.object_x" in forces
    names = ["contact_force_w.FR_foot_z", "contact_force_w.RL_foot_z", "contact_force_w.trunk_x", "contact_force_w.object_z", "cmd.vx"]
    tel = env.telemetry = Telemetry(env, {n: n for n in names}, env_ids=(3, 0), capacity=4)
    want = []
    for _ in range(6):
        env.step(torch.zeros(16, 12, device=DEV))
        robot, obj = env.contact_forces_w_history, env.object_forces_w_history  # (N, 3 slots, 17 bodies, 3), (N, 3, 1, 3): newest slot 0
        want.append(torch.stack([robot[:, 0, 13, 2], robot[:, 0, 16, 2], robot[:, 0, 0, 0], obj[:, 0, 0, 2], env.field("LT_F_CMD")[:, 0, 0]], dim=1)[[3, 0]])
    assert torch.equal(tel.read(), torch.stack(want[2:]))  # capacity 4: the newest four, oldest first
    assert bool((tel.read()[:, :, :2] != 0).any())  # the feet carry the robot
    path = tel.save(str(tmp_path / "telemetry" / "play.npz"))
    z = np.load(path)
    assert z["names"].tolist() == names and z["env_ids"].tolist() == [3, 0] and float(z["step_dt"]) == pytest.approx(env.step_dt)
    assert int(z["first_step"]) == 2 and int(z["dropped"]) == 2 and np.array_equal(z["data"], torch.stack(want[2:]).cpu().numpy())


def _video_args(telemetry, resolution="160x90"):
    return argparse.Namespace(video=True, video_length=4, video_interval=10 ** 6, video_camera="follow", video_resolution=resolution,
                              video_tactile=False, video_telemetry=telemetry, telemetry=False, telemetry_envs="5", telemetry_capacity=64,
                              telemetry_channels="cmd,reward")


def test_video_frames_differ_only_inside_the_chart(tmp_path):
    import torch

    from locotouch_amd import render as R
    from locotouch_amd.telemetry import telemetry_for
    from locotouch_amd.video import recorder_for
    from tests import telemetry_ref as T

    env = _teacher()
    tel = telemetry_for(env, _video_args(True))  # the chart's channels and the filmed env are added to what was asked for
    assert env.telemetry is tel and tel.env_ids == [5, 0] and tel.names[:4] == ["cmd.vx", "cmd.vy", "cmd.wz", "reward"] and len(tel.names) == 8
    on = recorder_for(env, _video_args(True), str(tmp_path / "on"), telemetry=tel)
    off = recorder_for(env, _video_args(False), str(tmp_path / "off"), telemetry=tel)  # without the flag the telemetry is not looked at
    chart = R.default_chart(160, 90)
    cw, ch = R.chart_size(chart)
    x0, y0 = 8, 90 - 8 - ch
    plots = [([tel.names.index(n) for n in names], *chart.scale(lo, hi)) for names, (lo, hi) in chart.plots]
    g = torch.Generator(device="cpu").manual_seed(1)
    for frame in range(2):
        for _ in range(5):
            env.step((0.5 * torch.randn(16, 12, generator=g)).to(DEV))
        with_chart, plain = on.render_fn().cpu().numpy().view(np.uint32), off.render_fn().cpu().numpy().view(np.uint32)
        assert with_chart.shape == plain.shape == (90, 160)
        outside = np.ones((90, 160), bool)
        outside[y0:y0 + ch, x0:x0 + cw] = False
        assert np.array_equal(with_chart[outside], plain[outside]) and not np.array_equal(with_chart, plain)
        want = T.chart(plain[None], tel.ring.cpu().numpy(), tel.count, [tel.slot_of(0)], plots, chart.pw, chart.ph, chart.gap, x0, y0, chart.opacity)[0]
        assert tel.count == 5 * (frame + 1) and np.array_equal(with_chart, want)
    on.close()
    off.close()
    with pytest.raises(ValueError, match="env 0 is not recorded by this Telemetry"):
        from locotouch_amd.telemetry import Telemetry

        recorder_for(env, _video_args(True), str(tmp_path / "x"), telemetry=Telemetry(env, {n: n for n in tel.names}, env_ids=(5,)))
