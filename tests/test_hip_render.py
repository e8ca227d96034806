"""GPU tests of the renderer (lt_env_render, csrc/lt_render.hip) against an independent numpy twin (tests/render_ref.py), analytic
scenes, the forward kinematics of compat/scene_views.py, and the promise that rendering changes nothing the env computes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TASKS = {"locomotion": "Isaac-Locomotion-LocoTouch-v1", "teacher": "Isaac-RandCylinderTransportTeacher-LocoTouch-v1",
         "student": "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"}


def _env(task, n, seed=3):
    from locotouch_amd.env import make

    return make(TASKS[task], num_envs=n, device="cuda:0", seed=seed)


def _random_steps(env, steps, seed=0):
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(steps):
        env.step((0.6 * torch.randn(env.num_envs, 12, generator=g)).to(env.device))
    torch.cuda.synchronize()


def _cameras():
    from locotouch_amd import render as R

    return [R.chase_camera(), R.Camera(eye=(1.5, 1.0, 0.6), lookat=(0.0, 0.0, 0.2), origin=R.ORIGIN_ASSET_ROOT, fov_y_deg=50.0)]


def _near(mask_a, ids, other):
    """True where a 3x3 neighbour of the pixel carries id `other`."""
    h, w = ids.shape
    pad = np.pad(ids, 1, constant_values=-2)
    out = np.zeros((h, w), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= pad[dy:dy + h, dx:dx + w] == other
    return out & mask_a


def _neighbour_differs(flag):
    h, w = flag.shape
    pad = np.pad(flag, 1, mode="edge")
    out = np.zeros((h, w), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= pad[dy:dy + h, dx:dx + w] != flag
    return out


@pytest.mark.parametrize("task", list(TASKS))
def test_matches_numpy_twin_and_fk(task):
    import torch
    from locotouch_amd import render as R
    from tests import render_ref

    n, W, H = 8, 96, 64
    env = _env(task, n)
    _random_steps(env, 50)
    cams = _cameras()
    for cam in cams:
        out = env.render(list(range(n)), cam, width=W, height=H, depth=True, ids=True, poses=True)
        torch.cuda.synchronize()
        rgb = R.rgba_to_rgb(out["rgba"]).astype(np.int64)
        ids, depth, poses = out["ids"].cpu().numpy(), out["depth"].cpu().numpy(), out["poses"].cpu().numpy()
        feet = env.field("LT_F_FOOT_POS_W").cpu().numpy()  # [N][3 comp][4 legs]
        for e in range(n):
            ref = render_ref.render(render_ref.env_state(env, e), cam, W, H)
            # FK: every body against link_kinematics, the feet against the step kernel's own foot positions
            assert np.abs(poses[e, :, :3] - ref["poses"][:, :3]).max() < 1e-5, (task, e)
            qa, qb = poses[e, :, 3:], ref["poses"][:, 3:]
            assert np.minimum(np.abs(qa - qb).max(1), np.abs(qa + qb).max(1)).max() < 1e-5
            assert np.abs(poses[e, 13:17, :3] - feet[e].T).max() < 1e-5
            agree = ids[e] == ref["ids"]
            assert agree.mean() >= 0.995, (task, e, agree.mean())
            bad = ~agree
            sil = np.zeros_like(bad)
            for other in np.unique(ref["ids"][bad]):
                sil |= _near(bad & (ref["ids"] == other), ids[e], other) | _near(bad & (ids[e] == other), ref["ids"], other)
            dclose = np.abs(depth[e] - ref["depth"]) < 1e-3
            assert (sil | dclose | agree).all(), (task, e, np.argwhere(~(sil | dclose | agree))[:5])
            hit = agree & (ids[e] >= 0)
            dd = np.abs(depth[e] - ref["depth"])[hit]
            assert (dd <= 1e-4 * ref["depth"][hit] + 1e-5).all(), (task, e, dd.max())
            assert (depth[e][ids[e] < 0] == R.DEPTH_MISS).all()
            diff = np.abs(rgb[e] - np.rint(ref["rgb"])).max(-1)
            edge = _neighbour_differs(ref["shadow"]) | _neighbour_differs(ref["taxel"] >= 0) | _neighbour_differs(ref["ids"])
            assert ((diff <= 2) | ~agree | edge).all(), (task, e, int(diff[agree & ~edge].max()))
            assert ((diff <= 2) | ~agree).mean() > 0.995


def test_ground_only_depth_and_checker():
    import torch
    from locotouch_amd import render as R

    env = _env("locomotion", 16)
    cam = R.Camera(eye=(20.0, 20.0, 3.0), lookat=(24.0, 26.0, 0.0), origin=R.ORIGIN_WORLD, fov_y_deg=40.0)
    W, H = 80, 48
    out = env.render([3], cam, width=W, height=H, depth=True, ids=True)
    torch.cuda.synchronize()
    ids, depth = out["ids"][0].cpu().numpy(), out["depth"][0].cpu().numpy()
    assert (ids == R._abi.CONSTS["LT_PRIM_GROUND"]).all()
    d = R.ray_directions(cam.eye, cam.lookat, cam.fov_y_deg, W, H)
    expect = 3.0 / -d[..., 2]
    assert (np.abs(depth - expect) <= 1e-5 * expect).all()
    p = np.asarray(cam.eye) + expect[..., None] * d
    parity = (np.floor(p[..., 0] / 0.5).astype(int) + np.floor(p[..., 1] / 0.5).astype(int)) & 1
    rgb = R.rgba_to_rgb(out["rgba"][0]).astype(int)
    light = rgb[..., 0] > rgb[..., 0].mean()  # the two checker albedos at one Lambert factor (flat ground, no shadow here)
    # pixels whose ray lands within 1 mm of a checker line may round either way
    frac = np.minimum(np.abs(p[..., :2] / 0.5 - np.rint(p[..., :2] / 0.5)).min(-1), 1.0) * 0.5
    sure = frac > 1e-3
    assert (light == (parity == 1))[sure].all()


def test_top_down_centre_pixel_is_plate():
    import torch
    from locotouch_amd import render as R
    from tests import render_ref

    env = _env("teacher", 16)
    torch.cuda.synchronize()
    st = render_ref.env_state(env, 5)
    cam = R.Camera(eye=(0.0, 0.05, 1.5), lookat=(0.0, 0.05, 0.0), origin=R.ORIGIN_ASSET_ROOT, fov_y_deg=30.0)
    env.field("LT_F_OBJ_POS")[5, 0, :3] = torch.tensor([50.0, 50.0, 0.5], device=env.device)  # the object out of the way
    out = env.render([5], cam, width=65, height=65, depth=True, ids=True)
    torch.cuda.synchronize()
    assert out["ids"][0, 32, 32].item() == R._abi.CONSTS["LT_PRIM_PLATE"]
    poses = render_ref.body_poses(st["root_pos"], st["root_quat"], st["joint_pos"])
    Rt = render_ref.quat_mat(poses[0, 3:])
    # plate top: z(x, y) of the plane through root + Rt (0, 0, 0.093) with normal Rt e_z, at the ray x, y
    nrm, p0 = Rt[:, 2], st["root_pos"] + Rt @ np.array([0.0, 0.0, 0.093])
    xy = st["root_pos"][:2] + np.array([0.0, 0.05])
    ztop = p0[2] - (nrm[0] * (xy[0] - p0[0]) + nrm[1] * (xy[1] - p0[1])) / nrm[2]
    assert abs(out["depth"][0, 32, 32].item() - (st["root_pos"][2] + 1.5 - ztop)) < 1e-4


def test_taxel_tint_at_projected_centres():
    import torch
    from locotouch_amd import render as R
    from tests import render_ref

    env = _env("student", 16)
    torch.cuda.synchronize()
    e = 2
    g = torch.Generator(device="cpu").manual_seed(5)
    bits = (torch.rand(221, generator=g) < 0.3).float()
    env.obs_tactile[e, :221] = bits.to(env.device)
    env.field("LT_F_OBJ_POS")[e, 0, :3] = torch.tensor([50.0, 50.0, 0.5], device=env.device)
    cam = R.Camera(eye=(0.0, 0.0, 0.6), lookat=(0.0, 0.0, 0.0), origin=R.ORIGIN_ASSET_ROOT, fov_y_deg=40.0)
    W = H = 160
    out = env.render([e], cam, width=W, height=H, ids=True)
    torch.cuda.synchronize()
    rgb = R.rgba_to_rgb(out["rgba"][0]).astype(int)
    st = render_ref.env_state(env, e)
    poses = render_ref.body_poses(st["root_pos"], st["root_quat"], st["joint_pos"])
    Rt = render_ref.quat_mat(poses[0, 3:])
    eye = np.asarray(cam.eye) + st["root_pos"]
    f, r, u = R.basis(eye, eye - np.asarray(cam.eye) + np.asarray(cam.lookat))
    t = np.tan(np.radians(cam.fov_y_deg) / 2)
    tinted = (rgb[..., 0] > 1.6 * rgb[..., 1]) & (rgb[..., 2] > 1.6 * rgb[..., 1])  # the contact tint: magenta
    for k in range(221):
        row, col = divmod(k, 13)
        c = st["root_pos"] + Rt @ np.array([0.1144 - 0.0143 * row, 0.0768 - 0.0128 * col, 0.093])
        v = c - eye
        px = (v @ r / (v @ f) / (t * W / H) + 1) * W / 2
        py = (1 - v @ u / (v @ f) / t) * H / 2
        assert tinted[int(py), int(px)] == bool(bits[k] > 0.5), (k, px, py)
    ref = render_ref.render(st, cam, W, H)
    on = (ref["taxel"] >= 0) & (np.asarray(bits)[np.clip(ref["taxel"], 0, 220)] > 0.5)
    edge = _neighbour_differs(ref["taxel"])
    assert (tinted == on)[~edge].all()


def test_batch_independence_and_graph_replay():
    import torch
    from locotouch_amd import render as R

    env = _env("teacher", 16)
    _random_steps(env, 10)
    cams = [R.chase_camera(), R.Camera(eye=(2.0, -1.0, 1.0), lookat=(0.0, 0.0, 0.0), origin=R.ORIGIN_WORLD)]
    both = env.render([4, 9], cams, width=96, height=64, depth=True, ids=True, poses=True)
    one = env.render([4], cams[0], width=96, height=64, depth=True, ids=True, poses=True)
    two = env.render([9], cams[1], width=96, height=64, depth=True, ids=True, poses=True)
    torch.cuda.synchronize()
    for k in ("rgba", "depth", "ids", "poses"):
        assert torch.equal(both[k][0], one[k][0]) and torch.equal(both[k][1], two[k][0]), k
    # 40 views: two launches (LT_RENDER_VIEWS_PER_LAUNCH = 32); view 35 equals its single render
    many = env.render(list(range(16)) * 2 + [4] * 8, cams[0], width=64, height=48)
    single = env.render([4], cams[0], width=64, height=48)
    torch.cuda.synchronize()
    assert torch.equal(many["rgba"][35], single["rgba"][0]) and torch.equal(many["rgba"][4], single["rgba"][0])

    # graph capture of step + render replays what eager execution computes
    a = _env("teacher", 16, seed=11)
    b = _env("teacher", 16, seed=11)
    act = torch.zeros(16, 12, device="cuda:0")
    torch.cuda.synchronize()
    bufs = a.render([1], cams[0], width=96, height=64, depth=True)
    a._arena_aligned.copy_(b._arena_aligned)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            a.step_raw(act.data_ptr())
            a.render([1], cams[0], width=96, height=64, depth=True, out=bufs)
    torch.cuda.synchronize()
    a._arena_aligned.copy_(b._arena_aligned)
    for _ in range(3):
        graph.replay()
        b.step(act)
        eager = b.render([1], cams[0], width=96, height=64, depth=True)
        torch.cuda.synchronize()
        assert torch.equal(bufs["rgba"], eager["rgba"]) and torch.equal(bufs["depth"], eager["depth"])
        assert torch.equal(a._arena_aligned, b._arena_aligned)


def test_rendering_changes_no_env_state():
    import torch
    from locotouch_amd import render as R

    a, b = _env("teacher", 64, seed=21), _env("teacher", 64, seed=21)
    g = torch.Generator(device="cpu").manual_seed(2)
    for _ in range(40):
        act = (0.6 * torch.randn(64, 12, generator=g)).to("cuda:0")
        a.step(act)
        b.step(act)
        b.render([0, 7, 33], R.chase_camera(), width=96, height=64, depth=True, ids=True, poses=True)
    torch.cuda.synchronize()
    assert torch.equal(a._arena_aligned, b._arena_aligned)


def _learn(tmp_path, record: bool):
    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.rl import OnPolicyRunner
    from locotouch_amd.video import VideoRecorder

    torch.manual_seed(0)
    env = _env("teacher", 512, seed=1)
    cfg = train_cfg(TASKS["teacher"])
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    rec = None
    if record:
        from locotouch_amd import render as R

        bufs: dict = {}

        def frame():
            bufs.update(env.render([0], R.chase_camera(), width=160, height=96, out=bufs if bufs else None))
            return bufs["rgba"][0]

        rec = VideoRecorder(frame, str(tmp_path), step_trigger=lambda s: s == 3, video_length=30, fps=50.0, disable_logger=True)
        env.recorder = rec
    assert runner._make_fused() is not None
    runner.learn(3, init_at_random_ep_len=True)
    if rec is not None:
        rec.close()
    params = [p.detach().clone() for p in runner.alg.actor_critic.parameters()]
    return [(h["Train/mean_reward"], h["Train/mean_episode_length"]) for h in runner.history], params, rec


def test_recording_training_is_bit_identical_and_writes_a_video(tmp_path):
    import zlib

    from tests.test_render_cpu import parse_apng

    hist0, par0, _ = _learn(tmp_path / "a", False)
    hist1, par1, rec = _learn(tmp_path / "b", True)
    assert hist0 == hist1
    assert all(bool((x == y).all()) for x, y in zip(par0, par1))
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["rl-video-step-3.apng"], files
    info = parse_apng(open(os.path.join(tmp_path / "b", files[0]), "rb").read())
    assert info["num_frames"] == 30 and len(info["frames"]) == 30
    for fr in info["frames"]:
        rgb = fr.astype(int)
        sky = (np.abs(rgb - np.array([140, 179, 230])) <= 2).all(-1)
        ground = (np.abs(rgb[..., 0] - rgb[..., 1]) <= 1) & (rgb[..., 2] <= rgb[..., 0])
        assert (~sky & ~ground).mean() > 0.01
    _ = zlib
