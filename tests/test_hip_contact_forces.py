"""Contact-force vectors on the GPU (LocoTouchVecEnv(contact_force_vectors=True) -> lt_env_bind_contact_forces -> the FVEC
instantiations of lt_step_kernel): they change no dynamics, their norms are the arena's |F| history, they are world-frame forces
ON the bodies (statics of a standing robot), both kernel forms and a captured graph write the same vectors, and a user term that
reads force components sees them through the slow path.  (CPU side: tests/test_contact_forces_abi.py.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEACHER = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
LOCO = "Isaac-Locomotion-LocoTouch-v1"
STUDENT = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"


def _norms(env):
    """(N, 3, 17) |F| the arena keeps: trunk (LT_F_TRUNK_FORCE_HIST lanes 0-2), then body 1 + type * 4 + leg (LT_F_FORCE_HIST)."""
    import torch

    n = env.num_envs
    fh = env.field("LT_F_FORCE_HIST").reshape(n, 3, 16)
    tr = env.field("LT_F_TRUNK_FORCE_HIST")[:, 0, :3]
    return torch.cat([tr.unsqueeze(-1), fh], dim=-1)


def _check_vectors_against_norms(env, dones):
    import torch

    vec = env.contact_forces_w_history
    want = _norms(env)
    got = torch.linalg.norm(vec, dim=-1)
    assert torch.all((got - want).abs() <= 1e-5 * want + 1e-4), float((got - want).abs().max())
    fin = dones != 0
    assert torch.all(vec[fin] == 0) and torch.all(env.object_forces_w_history[fin] == 0)


def _assert_same_dynamics(a, b, exact, n, bad, t):
    import torch

    if exact:
        assert torch.equal(a._arena_aligned, b._arena_aligned), f"arenas differ after step {t + 1}"
        return
    # the FVEC instantiations of the teacher's one-wave form and of the tactile task fuse one more multiply-add into an FMA than the
    # plain ones (a last-bit rounding difference, amplified by contact switches): the forms-test band (test_hip_forms.py), dones exact
    assert torch.equal(a.dones_buf, b.dones_buf), f"dones differ after step {t + 1}"
    for x, y in ((a.obs_policy, b.obs_policy), (a.obs_critic, b.obs_critic), (a.reward_buf.unsqueeze(1), b.reward_buf.unsqueeze(1))):
        bad |= ((x - y).abs() > 2e-4 * (1.0 + y.abs())).any(dim=1)
    assert int(bad.sum()) <= max(2, n // 100), f"{int(bad.sum())} of {n} envs drifted by step {t + 1}"


@pytest.mark.parametrize("task,n,rows,exact,steps", [(TEACHER, 4096, None, True, 50), (TEACHER, 8208, None, False, 6),
                                                     (LOCO, 4096, None, True, 50), (LOCO, 8208, None, True, 50),
                                                     (STUDENT, 405, None, False, 6), (TEACHER, 4096, "bf16", True, 50)])
def test_vectors_leave_the_dynamics_untouched(task, n, rows, exact, steps):
    """Two envs, same seed and actions, one writing vectors.  Byte-equal arenas after every one of 50 steps: the helper form (4096:
    teacher, locomotion, the bf16-row step_rows path) and the locomotion one-wave form (8208).  The teacher's one-wave form (8208)
    and the tactile student (405) are not bit-identical (see _assert_same_dynamics): like the two forms in test_hip_forms.py they
    are held to that band over 6 steps, before contact switches let trajectories fork.  The vectors' norms are the |F| history
    after every step."""
    import torch

    from locotouch_amd.env import LocoTouchVecEnv

    envs = [LocoTouchVecEnv(task, num_envs=n, device="cuda:0", seed=31, contact_force_vectors=v) for v in (False, True)]
    if rows:
        for e in envs:
            e.set_row_format(torch.bfloat16)
        slots = [[torch.zeros(n, e.num_obs, dtype=torch.bfloat16, device="cuda:0") for _ in range(4)] for e in envs]
        for e, s in zip(envs, slots):
            s[0].copy_(e.obs_policy)
            s[1].copy_(e.obs_critic)
    g = torch.Generator(device="cpu").manual_seed(9)
    resets = 0
    bad = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    for t in range(steps):
        act = (0.8 * torch.randn(n, 12, generator=g)).to("cuda:0")
        for i, e in enumerate(envs):
            if rows:
                s = slots[i]
                p, q = (0, 2) if t % 2 == 0 else (2, 0)
                e.step_rows_raw(act.data_ptr(), s[p].data_ptr(), s[p + 1].data_ptr(), s[q].data_ptr(), s[q + 1].data_ptr())
            else:
                e.step(act)
        torch.cuda.synchronize()
        _assert_same_dynamics(envs[0], envs[1], exact, n, bad, t)
        if rows:
            assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(*slots)), f"rows differ after step {t + 1}"
        dones = envs[1].dones_buf
        resets += int(dones.sum())
        _check_vectors_against_norms(envs[1], dones)
    if steps >= 50:
        assert resets > 0  # the zeroing of resetting envs was exercised
    assert float(envs[1].contact_forces_w_history.abs().sum()) > 0
    if task != LOCO:
        assert float(envs[1].object_forces_w_history.abs().sum()) > 0
    else:
        assert float(envs[1].object_forces_w_history.abs().sum()) == 0


def _total_robot_mass():
    src = open(os.path.join(REPO, "include", "lt_go1_model.h")).read()
    return float(re.search(r"#define LT_TOTAL_MASS ([0-9.]+)f", src).group(1))


@pytest.mark.parametrize("task", [LOCO, TEACHER])
def test_standing_statics_fix_frame_and_sign(task):
    """A robot standing on zero actions (zero commands, no pushes, 100 steps to settle).  It does not come fully to rest in this
    engine - it sags to ~0.2 m and keeps bobbing a little - so the locomotion statics are checked on the average over 100 further
    steps of the envs that did not reset (momentum balance: mean net contact force = m g + m dv/T): the forces ON the robot's
    bodies sum to (0, 0, m_robot g) - world frame, +z up, body order complete, m_robot counting trunk_mass_add.  The teacher does
    not hold that stand long enough for a quiet window (base-height terminations); there, at every step, where the object lies on
    the plate the trunk's force is exactly -F_obj (the plate pair is the trunk's only contact when standing), which ties the
    object's force and the plate reaction on the trunk to the same frame and opposite signs.

    Friction cone of the feet, from the implicit contact law (DESIGN.md §4 "Physics model", contact_law in csrc/lt_physics_crba.h):
    the tangential force is F_t = -c_t v_t' with c_t <= mu f0n / max(|v_t|, 1e-6) (v_t, v_t' the slip velocity before and after
    the substep) and the normal force is F_n = f0n - h B_n a_n.  Where the contact is steady over the substep (v_t' ~ v_t,
    a_n ~ 0) that is |F_t| <= mu F_n, mu = foot friction x ground friction; the bobbing leaves some substeps outside it, so the
    bound (with 5 % + 0.05 N) is required of 95 % of the loaded foot samples.  Likewise the ground pushes (F_z >= 0) except where the
    damping term pulls for a substep: required of 99 % of the leg-body samples."""
    import torch

    from locotouch_amd import _abi
    from locotouch_amd.env import LocoTouchVecEnv

    n = 4096
    cfg = _abi.preset_cfg(task, num_envs=n, seed=13)
    for i in range(3):
        cfg.cmd_range_init[i][0] = cfg.cmd_range_init[i][1] = 0.0
        cfg.cmd_range_max[i] = 0.0
    cfg.cmd_rel_standing = cfg.cmd_rel_standing_final = 1.0
    cfg.cur_enabled = 0
    for r in (cfg.push_robot_interval, cfg.push_obj_interval):
        r[0] = r[1] = 1e9
    for i in range(6):
        cfg.reset_root_vel[i][0] = cfg.reset_root_vel[i][1] = 0.0
    env = LocoTouchVecEnv(task, device="cuda:0", cfg=cfg, contact_force_vectors=True)
    zero = torch.zeros(n, 12, device="cuda:0")
    for _ in range(100):
        env.step(zero)
    g = float(cfg.gravity)
    has_obj = task != LOCO
    quiet = torch.ones(n, dtype=torch.bool, device="cuda:0")
    acc_r = torch.zeros(n, 3, device="cuda:0")
    pushes = cone = cone_n = legs_n = plate_n = 0.0
    K = 100
    for _ in range(K):
        _, _, dones, _ = env.step(zero)
        quiet &= dones == 0
        rob = env.contact_forces_w_history  # (n, 3, 17, 3)
        obj = env.object_forces_w_history[:, :, 0]
        acc_r += rob.sum(dim=2).mean(dim=1)
        legs = rob[:, :, 1:, 2]
        pushes += float((legs >= -1e-3).sum())
        legs_n += legs.numel()
        mu = (env.field("LT_F_FOOT_FRICTION")[:, 0, :] * float(cfg.ground_mu)).unsqueeze(1)  # (n, 1, leg)
        ft, fz = rob[:, :, 13:17, :2].norm(dim=-1), rob[:, :, 13:17, 2]
        loaded = fz > 1.0
        cone += float(((ft <= 1.05 * mu * fz + 0.05) & loaded).sum())
        cone_n += float(loaded.sum())
        if has_obj:
            on_plate = (dones == 0) & (obj[:, 0, 2] > 0) & (env.field("LT_F_OBJ_POS")[:, 0, 2] > 0.25)
            plate_n += float(on_plate.sum())
            tr, ob = rob[on_plate][:, :, 0], obj[on_plate]
            assert torch.all((tr + ob).norm(dim=-1) <= 1e-5 * ob.norm(dim=-1) + 1e-6)
        else:
            assert torch.all(obj == 0)
    assert pushes / legs_n >= 0.99, pushes / legs_n
    assert cone / max(cone_n, 1.0) >= 0.95, cone / max(cone_n, 1.0)
    if has_obj:  # (the teacher does not hold a zero-action stand for long - base-height terminations - so no window is quiet)
        assert plate_n >= 0.25 * n * K
        return
    assert float(quiet.float().mean()) >= 0.9  # (some envs end by a termination while standing, tools/stand_probe.py)
    m_robot = _total_robot_mass() + env.field("LT_F_ENV_PARAMS")[:, 0, 0]
    fr = acc_r[quiet] / K / (m_robot[quiet] * g).unsqueeze(1)  # mean force / weight
    assert abs(float(fr[:, 2].median()) - 1.0) <= 0.02, float(fr[:, 2].median())
    assert float(((fr[:, 2] - 1.0).abs() <= 0.05).float().mean()) >= 0.9
    assert float(fr[:, :2].norm(dim=-1).median()) <= 0.02


def _dump(tmp_path, task, n, steps, max_wg):
    out = str(tmp_path / f"fvec_{max_wg}.npz")
    env = dict(os.environ)
    if max_wg is not None:
        env["LT_STEP_HELPERS_MAX_WG"] = str(max_wg)
    else:
        env.pop("LT_STEP_HELPERS_MAX_WG", None)
    r = subprocess.run([sys.executable, "-m", "tests.contact_force_dump", task, str(n), str(steps), out], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


def test_four_wave_and_one_wave_forms_write_the_same_vectors(tmp_path):
    """The same env in the two forms of the step kernel (fresh processes; LT_STEP_HELPERS_MAX_WG=0 forces the one-wave form).  As in
    test_hip_forms.py the forms may differ by FMA contraction: an env whose contact switched in one form only may drift."""
    n, steps = 1000, 6
    a = _dump(tmp_path, TEACHER, n, steps, None)
    b = _dump(tmp_path, TEACHER, n, steps, 0)
    bad = np.zeros(n, bool)
    for t in range(steps):
        assert np.array_equal(a[f"done{t}"], b[f"done{t}"]), f"dones differ at step {t}"
        for k in (f"robot{t}", f"object{t}"):
            x, y = a[k].reshape(n, -1), b[k].reshape(n, -1)
            bad |= (np.abs(x - y) > 1e-2 * (1.0 + np.abs(y))).any(axis=1)
    # (contact forces of stiff penalty contacts amplify the forms' state differences: a wider band and envs than for the observations)
    assert bad.sum() <= max(2, n // 33), f"{int(bad.sum())} of {n} envs differ between the forms"
    assert np.abs(a[f"robot{steps - 1}"]).sum() > 0


def test_captured_rollout_writes_the_vectors_of_eager_steps():
    """A FusedRollout captured into a CUDA graph after the buffer was bound (at construction) records the vector-writing step
    kernel: replaying it leaves the same vectors as the same rollout launched eagerly on a twin env."""
    import torch

    from locotouch_amd.env import LocoTouchVecEnv
    from locotouch_amd.rl import PPO, ActorCritic, FusedRollout

    n, T = 4096, 4
    runs = []
    for graph in (False, True):
        env = LocoTouchVecEnv(TEACHER, num_envs=n, device="cuda:0", seed=42, contact_force_vectors=True)
        torch.manual_seed(1234)
        ac = ActorCritic(env.num_obs, env.num_obs, 12, init_noise_std=1.0, actor_hidden_dims=[512, 256, 128],
                         critic_hidden_dims=[512, 256, 128], activation="elu")
        alg = PPO(ac, device="cuda:0")
        alg.init_storage(n, T, [env.num_obs], [env.num_obs], [12])
        fused = FusedRollout(env, alg)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fused.rollout(T)  # warm-up (both runs take it, so both envs are T steps in)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fused.rollout(T)
            g.replay()
        else:
            fused.rollout(T)
        torch.cuda.synchronize()
        runs.append((env.contact_forces_w_history, env.object_forces_w_history, env._arena_aligned.clone()))
        del fused, alg, ac
    (r0, o0, a0), (r1, o1, a1) = runs
    assert float(r0.abs().sum()) > 0
    torch.testing.assert_close(r1, r0, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(o1, o0, rtol=1e-5, atol=1e-4)


def test_component_reading_user_term_through_the_slow_path():
    """A stumble-style user term (|F_xy| > k |F_z| on any foot) through ExtraTerms equals the same formula on
    contact_forces_w_history.  k = 4 (the reference's stumble ratio) lies outside the feet's friction cone on flat ground, so k = 0.2
    is run as well: that one fires (it never can on the |F|-in-z views of an env without vectors)."""
    import torch

    from locotouch_amd.compat.scene_views import ROBOT_SENSOR, ExtraTerms
    from locotouch_amd.env import LocoTouchVecEnv

    def stumble(env, sensor_name, body_ids, ratio):
        f = env.scene.sensors[sensor_name].data.net_forces_w[:, body_ids]
        return torch.any(torch.norm(f[..., :2], dim=-1) > ratio * torch.abs(f[..., 2]), dim=1).float()

    n = 2048
    env = LocoTouchVecEnv(TEACHER, num_envs=n, device="cuda:0", seed=5, contact_force_vectors=True)
    extra = ExtraTerms(env)
    ratios = (4.0, 0.2)
    for k in ratios:
        extra.add_reward(f"stumble_{k}", stumble, -1.0, {"sensor_name": ROBOT_SENSOR, "body_ids": [13, 14, 15, 16], "ratio": k})
    g = torch.Generator(device="cpu").manual_seed(2)
    fired = dict.fromkeys(ratios, 0.0)
    for _ in range(30):
        _, rew, dones, _ = env.step((1.0 * torch.randn(n, 12, generator=g)).to("cuda:0"))
        extra.apply(rew, dones)
        f = env.contact_forces_w_history[:, 0, 13:17]
        for k in ratios:
            want = torch.any(f[..., :2].norm(dim=-1) > k * f[..., 2].abs(), dim=1).float()
            assert torch.equal(extra.last_values[f"stumble_{k}"], want)
            fired[k] += float(want.sum())
    assert fired[0.2] > 0, fired
