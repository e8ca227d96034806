"""CPU tests of the renderer's host side: camera math, the ViewerCfg translation, the APNG writer, RecordVideo semantics, the
reference's train.py with --video, and every refusal of lt_env_render (before any launch)."""
import ctypes
import glob
import math
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from locotouch_amd import _abi
from locotouch_amd import render as R
from locotouch_amd.video import VideoRecorder, apng_bytes, deflate_frame, write_apng

REF = "/root/reference"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- camera math -----------------------------------------------------------------------------------------------------
def test_look_at_basis_and_rays():
    f, r, u = R.basis((0.0, 0.0, 1.0), (1.0, 0.0, 1.0))  # looking along +x
    assert np.allclose(f, [1, 0, 0]) and np.allclose(r, [0, -1, 0]) and np.allclose(u, [0, 0, 1])
    f, r, u = R.basis((0.0, 0.0, 2.0), (0.0, 0.0, 0.0))  # straight down: world y stands in for up
    assert np.allclose(f, [0, 0, -1]) and np.allclose(r, [1, 0, 0]) and np.allclose(u, [0, 1, 0])
    d = R.ray_directions((0, 0, 1), (1, 0, 1), 90.0, 4, 2)
    # vertical FOV 90: the top edge of the image is 45 deg up; pixel centres at +-0.5 of tan(45) vertically, aspect 2
    expect = np.array([1.0, -(2 * (1.5 / 4) - 1) * 2, 0.5])
    assert np.allclose(d[0, 1], expect / np.linalg.norm(expect))
    assert np.allclose(np.linalg.norm(d, axis=-1), 1.0)
    mid = R.ray_directions((0, 0, 0), (0, 5, 0), 30.0, 3, 3)[1, 1]
    assert np.allclose(mid, [0, 1, 0])
    top = R.ray_directions((0, 0, 0), (0, 5, 0), 60.0, 1, 1_000)[0, 0]
    assert abs(math.degrees(math.atan2(top[2], top[1])) - 30.0) < 0.1


def test_viewer_cfg_translation():
    class V:
        eye, lookat, resolution, env_index, asset_name = (5.0, 5.0, 4.0), (-2.0, -2.0, 0.0), (1920, 1080), 3, "robot"
        origin_type = "world"

    for origin_type, mode in (("world", R.ORIGIN_WORLD), ("env", R.ORIGIN_WORLD), ("asset_root", R.ORIGIN_ASSET_ROOT)):
        V.origin_type = origin_type
        cam, idx, res = R.from_viewer_cfg(V)
        assert cam.origin == mode and idx == 3 and res == (1920, 1080) and cam.eye == (5.0, 5.0, 4.0) and cam.lookat == (-2.0, -2.0, 0.0)
    V.origin_type = "nowhere"
    with pytest.raises(ValueError):
        R.from_viewer_cfg(V)
    V.origin_type, V.asset_name = "asset_root", "object"
    with pytest.raises(ValueError):
        R.from_viewer_cfg(V)
    assert R.chase_camera().origin == R.ORIGIN_ASSET_ROOT
    assert R.parse_resolution("640x360") == (640, 360)


# ---- APNG ------------------------------------------------------------------------------------------------------------
def parse_apng(blob: bytes) -> dict:
    """Inline chunk parser: checks the signature and every CRC, returns acTL / fcTL data and the decoded RGB frames."""
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        n = struct.unpack(">I", blob[pos:pos + 4])[0]
        kind, data = blob[pos + 4:pos + 8], blob[pos + 8:pos + 8 + n]
        crc = struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])[0]
        assert zlib.crc32(kind + data) & 0xFFFFFFFF == crc, kind
        chunks.append((kind, data))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1][0] == b"IEND"
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[0][1][:10])
    assert depth == 8 and ctype == 2
    actl = [d for k, d in chunks if k == b"acTL"]
    num_frames, plays = struct.unpack(">II", actl[0])
    seqs, delays, frames, cur = [], [], [], None
    for kind, data in chunks:
        if kind == b"fcTL":
            seq, fw, fh, x, y, dn, dd, _, _ = struct.unpack(">IIIIIHHBB", data)
            assert (fw, fh, x, y) == (w, h, 0, 0)
            seqs.append(seq)
            delays.append(dn / dd)
            cur = []
            frames.append(cur)
        elif kind == b"IDAT":
            cur.append(data)
        elif kind == b"fdAT":
            seqs.append(struct.unpack(">I", data[:4])[0])
            cur.append(data[4:])
    assert seqs == list(range(len(seqs)))
    out = []
    for parts in frames:
        raw = np.frombuffer(zlib.decompress(b"".join(parts)), np.uint8).reshape(h, 1 + 3 * w)
        assert (raw[:, 0] == 0).all()  # filter type None on every row
        out.append(raw[:, 1:].reshape(h, w, 3))
    return {"num_frames": num_frames, "plays": plays, "delays": delays, "frames": out, "size": (w, h)}


def test_apng_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (7, 11, 3), dtype=np.uint8) for _ in range(4)]
    path = str(tmp_path / "a.apng")
    write_apng(path, frames, 0.02)
    info = parse_apng(open(path, "rb").read())
    assert info["num_frames"] == 4 and info["size"] == (11, 7) and info["plays"] == 0
    assert all(abs(d - 0.02) < 1e-12 for d in info["delays"])
    for a, b in zip(frames, info["frames"]):
        assert np.array_equal(a, b)
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("PIL not importable: the independent decoder check is skipped")
    im = Image.open(path)
    assert getattr(im, "n_frames", 1) == 4
    with pytest.raises(ValueError):
        apng_bytes(2, 2, [], 0.02)
    _ = deflate_frame


# ---- RecordVideo semantics -------------------------------------------------------------------------------------------
class _NumberedFrames:
    """Frame k = the state after k steps: a 4 x 6 image filled with k."""

    def __init__(self):
        self.k = 0

    def __call__(self):
        return np.full((4, 6, 3), self.k % 256, dtype=np.uint8)


def test_step_trigger_and_video_length(tmp_path):
    src = _NumberedFrames()
    rec = VideoRecorder(src, str(tmp_path), name_prefix="rl-video", step_trigger=lambda s: s % 5 == 0, video_length=3, disable_logger=True)
    for _ in range(12):
        src.k += 1
        rec.after_step()
    rec.close()
    files = sorted(os.listdir(tmp_path))
    assert files == ["rl-video-step-0.apng", "rl-video-step-10.apng", "rl-video-step-5.apng"], files
    want = {0: [0, 1, 2], 5: [5, 6, 7], 10: [10, 11, 12]}
    for s, ks in want.items():
        info = parse_apng(open(tmp_path / f"rl-video-step-{s}.apng", "rb").read())
        assert [int(f[0, 0, 0]) for f in info["frames"]] == ks and info["num_frames"] == 3


def test_gym_shim_record_video_attaches_to_the_managed_env(tmp_path):
    from locotouch_amd.compat import runtime

    class Vec:
        num_envs, num_actions, num_obs, device, step_dt, max_episode_length = 2, 12, 4, "cpu", 0.02, 10

        def __init__(self):
            self.k = 0

        def step(self, a):
            self.k += 1
            return None, None, None, {}

        def render(self, env_ids, cam, width, height):
            return np.full((height, width, 3), self.k, np.uint8)

    class Cfg:
        class viewer:
            eye, lookat, origin_type, env_index, resolution, asset_name = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), "world", 0, (8, 6), None

    env = runtime.ManagedEnv("x", Cfg, Vec())
    assert env.render() is None
    env.render_mode = "rgb_array"
    assert env.render().shape == (6, 8, 3)
    runtime.install()
    import gymnasium

    out = gymnasium.wrappers.RecordVideo(env, video_folder=str(tmp_path), step_trigger=lambda s: s == 2, video_length=2, disable_logger=True)
    assert out is env and env.recorder is not None
    for _ in range(5):
        env.step(None)
    env.close()
    info = parse_apng(open(tmp_path / "rl-video-step-2.apng", "rb").read())
    assert [int(f[0, 0, 0]) for f in info["frames"]] == [2, 3] and info["size"] == (8, 6)


DRIVER = r"""
import os, runpy, sys
import numpy as np
sys.dont_write_bytecode = True
repo, script = sys.argv[1], sys.argv[2]
sys.path.insert(0, repo)
sys.path.insert(0, os.path.dirname(script))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(script))))
from locotouch_amd.compat import runtime
from tests.oracle_vec_env import OracleVecEnv
from tests import render_ref

class RenderingOracleEnv(OracleVecEnv):
    def render(self, env_ids, cam, width, height):
        e = int(env_ids[0])
        f = lambda name: self.field(name)[e].double().numpy()
        st = {"root_pos": f("LT_F_ROOT_POS")[0, :3], "root_quat": f("LT_F_ROOT_QUAT")[0, :4], "joint_pos": f("LT_F_JOINT_POS").reshape(12),
              "foot_force": f("LT_F_FORCE_HIST")[3], "obj": None, "taxels": None}
        out = render_ref.render(st, cam, 32, 24)
        return np.rint(out["rgb"]).astype(np.uint8)

def factory(task_id, cfg):
    lt, sizes = runtime.translate_env_cfg(task_id, cfg)
    return RenderingOracleEnv(task_id, cfg=lt, object_sizes=sizes)
runtime.install(env_factory=factory)
sys.argv = [script] + sys.argv[3:]
runpy.run_path(script, run_name="__main__")
"""


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present")
def test_reference_train_script_writes_a_video(tmp_path):
    script = os.path.join(REF, "locotouch", "scripts", "train.py")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-c", DRIVER, REPO, script, "--task", "Isaac-Locomotion-LocoTouch-v1", "--num_envs", "16", "--max_iterations", "1",
           "--headless", "--device", "cpu", "--seed", "7", "--video", "--video_length", "4", "--video_interval", "10", "--logger", "tensorboard", "agent.device=cpu"]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    vids = glob.glob(os.path.join(str(tmp_path), "logs", "rsl_rl", "*", "*", "videos", "train", "*.apng"))
    assert vids and all(os.path.getsize(v) > 0 for v in vids), vids
    info = parse_apng(open(sorted(vids)[0], "rb").read())
    assert info["num_frames"] == 4


# ---- ABI refusals ----------------------------------------------------------------------------------------------------
def test_render_refusals_before_any_launch():
    lib = _abi.load()
    cfg = _abi.preset_cfg("Isaac-Locomotion-LocoTouch-v1", num_envs=16)
    h = ctypes.c_void_p()
    assert lib.lt_env_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        desc = _abi.LtRenderDesc()
        desc.width, desc.height, desc.flags = 32, 24, R.DEFAULT_FLAGS
        desc.light_dir[2] = 1.0
        good = R.chase_camera().view(0)
        buf = ctypes.c_void_p(0x10000)  # never dereferenced: every call below is refused before a launch

        def call(views, n=None, rgba=buf, depth=None, d=desc, bind=True):
            arr = (_abi.LtRenderView * len(views))(*views)
            return lib.lt_env_render(h, ctypes.byref(d), arr, len(views) if n is None else n, rgba, depth, None, None, None)

        def refused(rc, words):
            assert rc == _abi.CONSTS["LT_EINVAL"], rc
            msg = lib.lt_last_error().decode()
            assert words in msg, msg

        refused(call([good]), "not bound")  # no arena bound yet
        assert lib.lt_env_bind(h, ctypes.c_void_p(0x100000), 1 << 40) == 0  # a fake, aligned arena: nothing may launch
        refused(call([good], n=0), "nviews")
        refused(call([good], n=-1), "nviews")
        bad = R.Camera(eye=(1, 1, 1), lookat=(0, 0, 0)).view(16)
        refused(call([bad]), "env id")
        bad = R.Camera(eye=(1, 1, 1), lookat=(0, 0, 0)).view(-1)
        refused(call([bad]), "env id")
        for w, hh in ((0, 24), (32, 0), (8193, 24), (32, 8193)):
            d = _abi.LtRenderDesc()
            d.width, d.height, d.flags = w, hh, 7
            d.light_dir[2] = 1.0
            refused(call([good], d=d), "width and height")
        refused(call([good], rgba=ctypes.c_void_p(0x10002)), "aligned")
        refused(call([good], depth=ctypes.c_void_p(0x10001)), "aligned")
        refused(call([good], rgba=None), "rgba")
        for eye in ((float("nan"), 0, 1), (float("inf"), 0, 1)):
            refused(call([R.Camera(eye=eye, lookat=(0, 0, 0)).view(0)]), "non-finite")
        refused(call([R.Camera(eye=(0, 0, 1), lookat=(0, 0, 1)).view(0)]), "eye equals lookat")
        refused(call([R.Camera(eye=(0, 0, 1), lookat=(1, 0, 1), fov_y_deg=0.0).view(0)]), "fov")
        d = _abi.LtRenderDesc()
        d.width, d.height, d.flags = 32, 24, 7
        refused(call([good], d=d), "light_dir")
    finally:
        lib.lt_env_destroy(h)
