"""GPU tests of the taxel panel (lt_tactile_panel_draw, csrc/lt_tactile_panel.hip) against the numpy twin (tests/tactile_panel_ref.py),
bit for bit: the panel's arithmetic is integer behind one correctly rounded float32 product, so there is no tolerance anywhere.  Then
the Python front: `env.draw_tactile_panel` on the student -Play- env's own groups, `recorder_for(..., --video_tactile)`, and the promise
that recording with the panel changes nothing a collection stores or a training step computes."""
import argparse
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLAY = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-Play-v1"
N, VIEWS = 3, [2, 0]
W, H = 101, 67  # neither a multiple of the kernel's 64 x 4 pixel tile
GUARD = 64      # words in front of and behind the frames


def _host_signals():
    """(two-channel rows at stride 442, 900-wide rows whose columns 8 ... 892 are the four-channel signal), random in [0, 1) with the
    special values and a few exact ties planted."""
    rng = np.random.default_rng(7)
    a, wide = rng.random((N, 442)).astype(np.float32), rng.random((N, 900)).astype(np.float32)
    special = np.array([np.nan, -0.0, 1.5, -3.0, np.inf, -np.inf, 0.5, 1.0, 0.0, 127.5 / 255, 1e-40, 0.49999997], np.float32)
    for e in range(N):
        a[e, 3:3 + special.size] = special          # channel 0: the binary map by default
        a[e, 221 + 40:221 + 40 + special.size] = special
        wide[e, 8 + 221 + 5:8 + 221 + 5 + special.size] = special  # channel 1 of the slice: the ramp by default
        wide[e, 8 + 3 * 221 + 100:8 + 3 * 221 + 100 + special.size] = special
    wide[:, :8], wide[:, 892:] = np.nan, np.nan      # what lies beside the slice is never drawn
    return a, wide


@pytest.fixture(scope="module")
def signals():
    import torch

    a, wide = _host_signals()
    da, dwide = torch.from_numpy(a).to(DEV), torch.from_numpy(wide).to(DEV)
    return {"host": [a, wide[:, 8:892]], "dev": [da, dwide[:, 8:892]], "keep": (da, dwide)}


def _pattern(v, h, w):
    """Per-pixel pattern, every byte in use (the alpha byte too), between guard words."""
    idx = np.arange(2 * GUARD + v * h * w, dtype=np.uint64)
    return ((idx * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _draw(signals_dev, maps, env_ids, buf, v, h, w, cell, gap, x0, y0, opacity):
    """One lt_tactile_panel_draw into frames [v, h, w] that start GUARD words into the int32 tensor `buf`."""
    import torch

    from locotouch_amd import _abi

    sig = (_abi.LtPanelSignal * len(signals_dev))()
    for s, t, m in zip(sig, signals_dev, maps):
        s.rows, s.row_stride, s.n_envs, s.channels = t.data_ptr(), t.stride(0), t.shape[0], t.shape[1] // 221
        for c, x in enumerate(m):
            s.maps[c] = x
    d = _abi.LtPanelDesc()
    d.nsignals, d.cell, d.gap, d.x0, d.y0, d.opacity = len(signals_dev), cell, gap, x0, y0, opacity
    ids = (ctypes.c_int32 * len(env_ids))(*env_ids)
    assert _abi.load().lt_tactile_panel_launches(ctypes.byref(d), sig, len(env_ids)) == 1
    _abi.call("lt_tactile_panel_draw", d, sig, ids, len(env_ids), buf[GUARD:GUARD + v * h * w], w, h, _abi.stream(torch.device(DEV)))


def _expect(signals_host, maps, env_ids, pattern, v, h, w, cell, gap, x0, y0, opacity):
    from tests import tactile_panel_ref as T

    out = pattern.copy()
    out[GUARD:GUARD + v * h * w] = T.draw(pattern[GUARD:GUARD + v * h * w].reshape(v, h, w), env_ids, signals_host, maps, cell, gap, x0, y0,
                                          opacity).reshape(-1)
    return out


def _as_tensor(words):
    import torch

    return torch.from_numpy(words.view(np.int32).copy())


B, RAMP = 0, 1  # LT_PANEL_MAP_BINARY, LT_PANEL_MAP_RAMP (held to the header in tests/test_tactile_panel_abi.py)
DEFAULT_MAPS = [[B, B], [B, RAMP, RAMP, RAMP]]
SWAPPED_MAPS = [[RAMP, B], [RAMP, B, B, RAMP]]
# (which signals, cell, gap, frame size, where, opacity, maps).  cell 3 fits the 101 x 67 frame with the two-channel signal alone; both
# signals at cell 3 are drawn into a 173 x 131 frame as well.
CASES = [((0, 1), 1, 1, (W, H), where, op, DEFAULT_MAPS) for where in ("origin", "flush") for op in (0, 160, 255)]
CASES += [((0, 1), 1, 0, (W, H), "inside", 160, SWAPPED_MAPS), ((1, 0), 1, 3, (W, H), "flush", 255, SWAPPED_MAPS)]
CASES += [((0,), 3, 2, (W, H), where, op, DEFAULT_MAPS) for where, op in (("origin", 255), ("flush", 160), ("flush", 0))]
CASES += [((0,), 3, 0, (W, H), "inside", 255, SWAPPED_MAPS), ((0, 1), 3, 2, (173, 131), "flush", 160, DEFAULT_MAPS)]


@pytest.mark.parametrize("which,cell,gap,size,where,opacity,maps", CASES)
def test_matches_the_twin_bit_for_bit(signals, which, cell, gap, size, where, opacity, maps):
    import torch

    from tests import tactile_panel_ref as T

    w, h = size
    v = len(VIEWS)
    host, dev, m = [signals["host"][i] for i in which], [signals["dev"][i] for i in which], [maps[i] for i in which]
    pw, ph = T.panel_size(cell, gap, [x.shape[1] // 221 for x in host])
    x0, y0 = {"origin": (0, 0), "flush": (w - pw, h - ph), "inside": (5, 3)}[where]
    pattern = _pattern(v, h, w)
    want = _as_tensor(_expect(host, m, VIEWS, pattern, v, h, w, cell, gap, x0, y0, opacity))
    buf = _as_tensor(pattern).to(DEV)
    _draw(dev, m, VIEWS, buf, v, h, w, cell, gap, x0, y0, opacity)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got, want), int((got != want).sum())
    # every guard word and every pixel outside the rectangle is the pattern's (the twin says so too; this does not go through it)
    words = got.numpy().view(np.uint32)
    assert np.array_equal(words[:GUARD], pattern[:GUARD]) and np.array_equal(words[-GUARD:], pattern[-GUARD:])
    frames = words[GUARD:-GUARD].reshape(v, h, w)
    outside = np.ones((v, h, w), bool)
    outside[:, y0:y0 + ph, x0:x0 + pw] = False
    assert np.array_equal(frames[outside], pattern[GUARD:-GUARD].reshape(v, h, w)[outside])
    if opacity > 0:
        assert not np.array_equal(frames[~outside], pattern[GUARD:-GUARD].reshape(v, h, w)[~outside])
    # a second run from the same frame: the same bits
    again = _as_tensor(pattern).to(DEV)
    _draw(dev, m, VIEWS, again, v, h, w, cell, gap, x0, y0, opacity)
    torch.cuda.synchronize()
    assert torch.equal(again, buf)


@pytest.mark.parametrize("cell", [1, 3])
def test_planted_pattern_is_neither_transposed_nor_mirrored(cell):
    """Taxels (0, 0), (0, 12), (16, 0) and (5, 7), each on another channel of a four-channel signal: where each lands is stated here in
    pixels, not taken from the twin (which must agree as well)."""
    import torch

    from tests import tactile_panel_ref as T

    w, h, gap = 173, 67, 2
    rows = np.zeros((N, 884), np.float32)
    planted = {0: (0, 0), 1: (0, 12), 2: (16, 0), 3: (5, 7)}
    for c, (r, k) in planted.items():
        rows[1, c * 221 + r * 13 + k] = 1.0
    rows[0], rows[2] = 1.0, 1.0  # the other envs' rows must not show
    dev = torch.from_numpy(rows).to(DEV)
    maps = [[B, B, B, B]]
    pattern = _pattern(1, h, w)
    buf = _as_tensor(pattern).to(DEV)
    x0, y0 = 4, 6
    _draw([dev], maps, [1], buf, 1, h, w, cell, gap, x0, y0, 255)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), _as_tensor(_expect([rows], maps, [1], pattern, 1, h, w, cell, gap, x0, y0, 255)))
    frame = buf.cpu().numpy().view(np.uint32)[GUARD:-GUARD].reshape(h, w)
    on = (frame & 0xFFFFFF) == (int(T.ON[0]) | int(T.ON[1]) << 8 | int(T.ON[2]) << 16)
    want = np.zeros_like(on)
    for c, (r, k) in planted.items():
        y, x = y0 + 1 + r * cell, x0 + 1 + c * (13 * cell + gap) + k * cell  # grid row r from the top, grid column k from the left
        want[y:y + cell, x:x + cell] = True
    assert on.sum() == 4 * cell * cell and np.array_equal(on, want)


def test_graph_replay_equals_the_eager_launch(signals):
    """A linear chain on one stream - restore the frame, draw - captured and replayed, against the same two steps run eagerly."""
    import torch

    v, cell, gap, x0, y0, opacity = len(VIEWS), 1, 1, 9, 7, 160
    pattern = _as_tensor(_pattern(v, H, W)).to(DEV)
    eager, replayed = pattern.clone(), torch.zeros_like(pattern)
    _draw(signals["dev"], DEFAULT_MAPS, VIEWS, eager, v, H, W, cell, gap, x0, y0, opacity)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            replayed.copy_(pattern)
            _draw(signals["dev"], DEFAULT_MAPS, VIEWS, replayed, v, H, W, cell, gap, x0, y0, opacity)
    torch.cuda.synchronize()
    for _ in range(2):
        replayed.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(replayed, eager)


# ---- the Python front on the real student -Play- env ----
FW, FH = 253, 307  # the default panel sits 8 pixels inside the corner: 216 x 210 for the env's three groups, 216 x 280 with `policy` on top


def _play_env(n=8, seed=3, steps=30):
    import torch

    from locotouch_amd.env import make

    env = make(PLAY, num_envs=n, device=DEV, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(steps):
        env.step((0.3 * torch.randn(n, 12, generator=g)).to(DEV))
    torch.cuda.synchronize()
    return env


def _twin_of_groups(frames, env_ids, groups, tactile_format, panel):
    """The twin's drawing of `groups` (name -> device tensor) with the front's defaults: maps by format, the corner and margin."""
    from locotouch_amd import render as R
    from tests import tactile_panel_ref as T

    host = [t.cpu().numpy() for t in groups.values()]
    channels = [x.shape[1] // 221 for x in host]
    maps = [R.channel_maps(tactile_format, c) for c in channels]
    pw, ph = T.panel_size(panel.cell, panel.gap, channels)
    assert panel.corner == "top-right"
    x0, y0 = frames.shape[2] - panel.margin - pw, panel.margin
    return T.draw(frames, env_ids, host, maps, panel.cell, panel.gap, x0, y0, panel.opacity)


def test_env_draws_its_own_groups_by_default_and_leaves_the_arena_alone():
    import torch

    from locotouch_amd import render as R

    env = _play_env()
    groups = env.tactile_groups()
    assert list(groups) == ["tactile", "original_tactile", "processed_tactile"]
    assert [tuple(t.shape) for t in groups.values()] == [(8, 442), (8, 884), (8, 884)]
    assert any(bool((t > 0.5).any()) for t in groups.values())  # there is contact to see
    arena = env._arena_aligned.clone()
    pattern = _pattern(2, FH, FW)[GUARD:-GUARD].reshape(2, FH, FW)
    frames = _as_tensor(pattern).to(DEV)
    out = env.draw_tactile_panel(frames, [5, 0])
    torch.cuda.synchronize()
    assert out is frames
    want = _twin_of_groups(pattern, [5, 0], groups, int(env.cfg.tactile_format), R.TactilePanel())
    assert torch.equal(frames.cpu(), _as_tensor(want))
    assert torch.equal(env._arena_aligned, arena)
    assert R.panel_size(R.TactilePanel(), groups) == (216, 210)
    # a mapping of the caller's own, another panel
    panel = R.TactilePanel(cell=2, gap=1, corner="top-right", margin=0, opacity=255)
    mine = {"policy": torch.rand(8, 442, device=DEV), "tactile": env.obs_tactile}
    frames2 = _as_tensor(pattern).to(DEV)
    env.draw_tactile_panel(frames2, torch.tensor([1, 7]), signals=mine, panel=panel)
    torch.cuda.synchronize()
    assert torch.equal(frames2.cpu(), _as_tensor(_twin_of_groups(pattern, [1, 7], mine, int(env.cfg.tactile_format), panel)))
    with pytest.raises(RuntimeError, match=r"env_ids\[1\] must be below"):
        env.draw_tactile_panel(frames2, [0, 8])
    with pytest.raises(RuntimeError, match="desc.x0 must be in 0"):
        env.draw_tactile_panel(torch.zeros(1, FH, 100, dtype=torch.int32, device=DEV), [0])


def _video_args(tactile, length=12, interval=1000):
    return argparse.Namespace(video=True, video_length=length, video_interval=interval, video_camera="follow", video_resolution=f"{FW}x{FH}",
                              video_tactile=tactile)


def test_recorder_frames_are_render_then_twin(tmp_path):
    import torch

    from locotouch_amd import render as R
    from locotouch_amd.scripts.distill import panel_signals_of
    from locotouch_amd.video import recorder_for

    env = _play_env()
    # default signals: the env's own groups
    rec = recorder_for(env, _video_args(True), str(tmp_path / "a"))
    got = rec.render_fn().cpu()
    plain = env.render([0], R.chase_camera(), width=FW, height=FH)["rgba"]
    torch.cuda.synchronize()
    scene = plain.cpu().numpy().view(np.uint32)
    want = _twin_of_groups(scene, [0], env.tactile_groups(), int(env.cfg.tactile_format), R.TactilePanel())
    assert got.shape == (FH, FW) and torch.equal(got, _as_tensor(want)[0])
    assert not np.array_equal(want, scene)
    rec.close()
    # without the flag: the render's own bytes, and the callable is never asked
    def never():
        raise AssertionError("tactile_signals was called without --video_tactile")

    rec = recorder_for(env, _video_args(False), str(tmp_path / "b"), tactile_signals=never)
    assert torch.equal(rec.render_fn().cpu(), plain[0].cpu())
    rec.close()
    # the distillation script's four rows: policy (the delay line's last rows), tactile, original_tactile, processed_tactile
    line = {}
    rec = recorder_for(env, _video_args(True, interval=10 ** 6), str(tmp_path / "c"), tactile_signals=panel_signals_of(env, line))
    delayed = (torch.rand(8, 442, device=DEV) < 0.2).float()

    class Line:
        last_delayed = delayed

    for line_now, policy_rows in (({}, torch.zeros_like(delayed)), ({"recorder": Line}, delayed)):
        line.clear()
        line.update(line_now)
        got = rec.render_fn().cpu()
        groups = {"policy": policy_rows, **env.tactile_groups()}
        assert R.panel_size(R.TactilePanel(), groups) == (216, 280)
        assert torch.equal(got, _as_tensor(_twin_of_groups(scene, [0], groups, int(env.cfg.tactile_format), R.TactilePanel()))[0])
    rec.close()


def _collect_and_train(tmp, tactile, **switches):
    """A short recorded collection on the -Play- env and one training pass of the student, from fixed seeds."""
    import torch

    from locotouch_amd.distill import Distillation, distillation_cfg
    from locotouch_amd.env import make
    from locotouch_amd.scripts.distill import panel_signals_of
    from locotouch_amd.video import recorder_for

    n = 16
    torch.manual_seed(0)
    np.random.seed(0)
    env = make(PLAY, num_envs=n, device=DEV, seed=5)
    env.episode_length_buf = torch.randint(460, 480, (n,), device=DEV)  # every episode ends within 40 steps: 200 kept steps come early
    line: dict = {}
    rec = recorder_for(env, _video_args(tactile, length=12, interval=1000), str(tmp / "videos"),
                       tactile_signals=panel_signals_of(env, line) if tactile else None)
    cfg = distillation_cfg(PLAY)
    cfg.logger, cfg.log_root_path = "tensorboard", str(tmp / "logs")
    cfg.num_iterations, cfg.initial_epoches, cfg.batch_steps = 1, 1, 200
    teacher = lambda obs: 0.5 * torch.tanh(obs[..., :12])  # noqa: E731
    d = Distillation(env, cfg, teacher_policy=teacher, verbose=False, log_dir=str(tmp / "logs" / "run"), **switches)
    line["recorder"] = d.tactile_recorder
    torch.manual_seed(1)
    d.replay_buffer.collect_data(teacher_policy=teacher, student_policy=None, num_steps=200)
    (policy, tactile_rows), _ = d.replay_buffer._materialise()
    policy, tactile_rows = policy.clone(), tactile_rows.clone()
    torch.manual_seed(2)
    np.random.seed(2)
    d.student.train_on_data(d.replay_buffer, 0)
    torch.cuda.synchronize()
    rec.close()
    return policy, tactile_rows, [p.detach().clone() for p in d.student.parameters()], rec, env._arena_aligned.clone()


@pytest.mark.parametrize("collection", ["eager", "fused"])
def test_recording_with_the_panel_is_bit_identical_and_writes_a_video(tmp_path, collection):
    """The rule of test_recording_training_is_bit_identical_and_writes_a_video, for the student: the same collection and training pass
    with `--video` alone and with `--video --video_tactile`.  The training pass runs through the project's own HIP kernels
    (`fused_cnn_training`, `fused_bc_step`: one fixed summation order), because only that pass has bits to compare: the eager pass
    (MIOpen convolutions, torch's loss and AdamW) does not repeat its own bits from one run to the next - measured on the MI355X with
    the flag off in both runs, 22 of the 28 parameter tensors differed, while the two switches gave 0 of 28 (and 0 of 28 flag off
    against flag on).  The collection runs once through the eager loop and once through the fused one (`fused_collection`, where the
    panel's `policy` rows are the store slot `push` wrote: no launch of the panel's own but the draw)."""
    import torch

    from tests.test_render_cpu import parse_apng

    switches = dict(fused_cnn_training=True, fused_bc_step=True)
    if collection == "fused":
        switches.update(fused_student_inference=True, fused_collection=True)
    runs = {flag: _collect_and_train(tmp_path / ("on" if flag else "off"), flag, **switches) for flag in (False, True)}
    off, on = runs[False], runs[True]
    assert off[0].shape[0] >= 200 and off[0].shape == on[0].shape
    assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1])  # the replay buffer's rows
    assert len(off[2]) == len(on[2]) and all(torch.equal(a, b) for a, b in zip(off[2], on[2]))  # the student after the training pass
    assert torch.equal(off[4], on[4])
    frames = {}
    for flag, run in runs.items():
        folder = tmp_path / ("on" if flag else "off") / "videos"
        assert sorted(os.listdir(folder)) == ["rl-video-step-0.apng"]
        info = parse_apng(open(folder / "rl-video-step-0.apng", "rb").read())
        assert info["num_frames"] == 12 and all(f.shape == (FH, FW, 3) for f in info["frames"])
        frames[flag] = info["frames"]
    # the same scene outside the panel's rectangle (216 x 280, 8 pixels inside the top-right corner), the panel inside it
    inside = np.zeros((FH, FW), bool)
    inside[8:8 + 280, FW - 8 - 216:FW - 8] = True
    for a, b in zip(frames[False], frames[True]):
        assert np.array_equal(a[~inside], b[~inside]) and not np.array_equal(a[inside], b[inside])
