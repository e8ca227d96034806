"""SURVEY.md §8(b) B3 - the slow path speaks the reference's data contract: the reference's OWN reward / termination functions
(locotouch/mdp/rewards.py, terminations.py - imported from the read-only checkout, unmodified) are registered as extra terms under
new names with their original `SceneEntityCfg("robot_contact_senosr", ...)` parameters, run on the views of
compat/scene_views.py, and each must equal the fused implementation's column of LT_F_REWARD_TERMS for the same state.

CPU: the oracle env stands in for the HIP env (same arena layout, same `field()` surface).  The GPU twin with locally restated
term bodies (no reference file travels to the GPU box) is tests/test_hip_reference_contract.py.
"""
import copy
import os
import re
import sys

import numpy as np
import pytest
import torch

from locotouch_amd import _abi

REF = "/root/reference"
TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
C = _abi.CONSTS


@pytest.fixture(scope="module")
def rt():
    """The reference's own cfg classes and terms; only the tests that take this fixture need the checkout."""
    if not os.path.isdir(REF):
        pytest.skip("reference checkout not present")
    sys.dont_write_bytecode = True
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import warnings

    from locotouch_amd.compat import runtime

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        runtime.install()
        import locotouch  # noqa: F401
    return runtime


def _reference_cfg_with_its_own_terms_as_user_terms(rt, n):
    """The teacher's env cfg; every function-valued reward term of it is registered a second time as `ref_<name>` - the
    reference's function object with a deep copy of the reference's own params (sensor names and all)."""
    from isaaclab.managers import RewardTermCfg as RewTerm

    cfg = rt.load_cfg_from_registry(TASK, "env_cfg_entry_point")
    cfg.scene.num_envs = n
    # the two terms the teacher keeps at weight 0 are never evaluated by the fused kernel then: switch them on
    cfg.rewards.object_xy_velocity.weight = -0.01
    cfg.rewards.object_z_contact.weight = -0.01
    # interval pushes change the root velocity AFTER the reward stage of the same step (SURVEY.md 3.3 stage 8): off, so that the
    # state a step leaves is the state its reward stage saw (stated limit of the slow path, compat/scene_views.py)
    cfg.events.push_robot = None
    cfg.events.push_object = None
    names = []
    for name, term in list(vars(cfg.rewards).items()):
        if name.startswith("_") or term is None or name == "alive":  # `alive` is a stock IsaacLab term (not in the checkout)
            continue
        setattr(cfg.rewards, "ref_" + name, RewTerm(func=term.func, weight=float(term.weight), params=copy.deepcopy(term.params)))
        names.append(name)
    return cfg, names


def test_model_constants_of_the_views_match_the_generated_header():
    from locotouch_amd.compat import scene_views as V

    hdr = open(os.path.join(os.path.dirname(_abi.HEADER), "lt_go1_model.h")).read()
    nums = lambda macro: [float(x.rstrip("f")) for x in re.findall(r"-?\d+\.\d+(?:e-?\d+)?f", re.search(rf"#define {macro} (.*)", hdr).group(1))]  # noqa: E731
    off = np.array(nums("LT_JOINT_OFFSET_INIT")).reshape(4, 3, 3)
    np.testing.assert_allclose(off[:, 0], np.array(V.HIP_OFFSET), atol=1e-7)
    np.testing.assert_allclose(off[:, 1], np.array(V.THIGH_OFFSET), atol=1e-7)
    np.testing.assert_allclose(off[:, 2], np.tile(np.array(V.CALF_OFFSET), (4, 1)), atol=1e-7)
    np.testing.assert_allclose(nums("LT_FOOT_OFFSET_INIT"), V.FOOT_OFFSET, atol=1e-7)


def test_link_kinematics_of_the_views_reproduce_the_engines_foot_kinematics():
    """`body_pos_w / body_lin_vel_w / body_quat_w` are torch forward kinematics; the engine computes the feet itself
    (LT_F_FOOT_POS_W / _VEL_W): both must agree, which pins offsets, axes, joint order and the velocity recursion."""
    from locotouch_amd.compat.scene_views import link_kinematics
    from tests.oracle_vec_env import OracleVecEnv

    n = 32
    vec = OracleVecEnv(TASK, num_envs=n, seed=3)
    g = torch.Generator().manual_seed(0)
    for _ in range(12):
        vec.step(0.8 * torch.randn(n, 12, generator=g))
    f = vec.field
    pos, quat, lin, ang = link_kinematics(f("LT_F_ROOT_POS")[:, 0, :3], f("LT_F_ROOT_QUAT")[:, 0, :4], f("LT_F_ROOT_LIN_VEL_W")[:, 0, :3],
                                          f("LT_F_ROOT_ANG_VEL_W")[:, 0, :3], f("LT_F_JOINT_POS").reshape(n, 12), f("LT_F_JOINT_VEL").reshape(n, 12))
    assert pos.shape == (n, 17, 3) and quat.shape == (n, 17, 4) and lin.shape == (n, 17, 3) and ang.shape == (n, 17, 3)
    keep = vec.field("LT_F_DONES") == 0  # (a finished env holds its reset state; the foot fields are refreshed by the next step)
    torch.testing.assert_close(pos[keep][:, 13:17], f("LT_F_FOOT_POS_W").permute(0, 2, 1)[keep], atol=2e-6, rtol=0)
    torch.testing.assert_close(lin[keep][:, 13:17], f("LT_F_FOOT_VEL_W").permute(0, 2, 1)[keep], atol=2e-5, rtol=1e-5)
    torch.testing.assert_close(quat.norm(dim=-1), torch.ones(n, 17), atol=1e-5, rtol=0)
    torch.testing.assert_close(pos[:, 0], f("LT_F_ROOT_POS")[:, 0, :3])
    # feet share the calf's orientation and angular velocity (fixed joint), the hips hang 0.04675 m beside the trunk axis
    assert torch.equal(quat[:, 9:13], quat[:, 13:17]) and torch.equal(ang[:, 9:13], ang[:, 13:17])
    torch.testing.assert_close((pos[:, 1:5] - pos[:, :1]).norm(dim=-1), torch.full((n, 4), float(np.hypot(0.1881, 0.04675))), atol=1e-5, rtol=0)


def test_the_references_own_reward_functions_run_on_the_views_and_equal_the_fused_columns(rt):
    from locotouch_amd.compat.runtime import ManagedEnv
    from tests.oracle_vec_env import OracleVecEnv

    n = 96
    cfg, names = _reference_cfg_with_its_own_terms_as_user_terms(rt, n)
    lt, sizes = rt.translate_env_cfg(TASK, cfg)
    lt.debug_terms = 1
    extra = {t[0]: t for t in lt.extra_reward_terms}
    assert sorted(extra) == sorted("ref_" + k for k in names) and len(names) == 24
    import locotouch.mdp as ref_mdp

    assert extra["ref_foot_slip"][1] is ref_mdp.foot_slipping_ngt and extra["ref_thigh_calf_collision"][1] is ref_mdp.thigh_calf_collision_ngt
    assert extra["ref_foot_slip"][3]["sensor_cfg"].name == "robot_contact_senosr"  # (sic) the reference's sensor name, as it stands
    assert extra["ref_gait"][1] is ref_mdp.AdaptiveSymmetricGaitRewardwithObject
    vec = OracleVecEnv(TASK, cfg=lt, object_sizes=sizes)
    env = ManagedEnv(TASK, cfg, vec, extra_rewards=lt.extra_reward_terms)
    idx = {k: i for i, k in enumerate(["alive", "track_lin_vel_xy", "track_ang_vel_z", "foot_slip", "foot_dragging", "gait", "track_base_height",
                                       "base_z_velocity", "base_roll_pitch_angle", "base_roll_pitch_velocity", "joint_position_limit",
                                       "joint_position", "joint_acceleration", "joint_velocity", "joint_torque", "action_rate",
                                       "thigh_calf_collision", "object_xy_position", "object_xy_velocity", "object_z_contact", "object_z_velocity",
                                       "object_roll_pitch_angle", "object_roll_pitch_velocity", "object_yaw_alignment", "object_dangerous_state"])}
    g = torch.Generator().manual_seed(0)
    nonzero = {k: 0 for k in names}
    compared = 0
    gait_bad = 0
    for t in range(60):
        act = (0.9 if t % 20 < 12 else 0.05) * torch.randn(n, 12, generator=g)
        _, _, dones, _ = env.step(act)
        fused = vec.field("LT_F_REWARD_TERMS").reshape(n, -1)
        keep = dones == 0
        compared += int(keep.sum())
        for k in names:
            got, want = env.extra.last_values["ref_" + k][keep], fused[keep, idx[k]]
            nonzero[k] += int((want != 0).sum())
            if k == "gait":  # a class with its own state: one thresholded timer compare may differ in the last bit; counted
                gait_bad += int((~torch.isclose(got, want, rtol=1e-4, atol=1e-5)).sum())
                continue
            torch.testing.assert_close(got, want, rtol=2e-4, atol=2e-5, msg=lambda m, k=k, t=t: f"{k} at step {t}: {m}")
    assert compared > 0.8 * 60 * n
    assert gait_bad <= 2e-3 * compared, f"reference gait class on the views vs fused gait term: {gait_bad} of {compared} differ"
    for k in names:  # every term was exercised (the comparison is not 0 == 0)
        assert nonzero[k] > 0 or k in ("joint_position_limit",), f"{k} never left 0"
    # cross-term reach-ins of the reference (rewards.py:380-381, commands.py:399-401, curriculums.py:238,259)
    te = env.extra.env
    assert te.reward_manager.get_term_cfg("object_dangerous_state").params["x_max"] == pytest.approx(0.125)
    assert te.reward_manager.get_term_cfg("gait").func.valid_last_air_time.shape == (n, 4)
    torch.testing.assert_close(te.reward_manager._episode_sums["track_lin_vel_xy"], vec.field("LT_F_EPISODE_SUMS").reshape(n, -1)[:, 1])
    assert te.reward_manager._episode_sums["ref_foot_slip"].shape == (n,)
    assert te.termination_manager.terminated.shape == (n,) and te.common_step_counter in (60, 61)  # (lt_env_reset_all's pass counts as one)
    a = te.action_manager.get_term("joint_pos")
    torch.testing.assert_close(a.processed_actions, a.raw_actions + te.scene["robot"].data.default_joint_pos)


def test_reference_functions_on_any_state_through_the_terms_hook(rt):
    """The same comparison without the reset / event caveats: `eval_terms` evaluates the fused terms on the arena AS IT IS, the
    reference functions read the views of the very same bytes - every env counts, including freshly reset ones."""
    import locotouch.mdp as ref
    from isaaclab.managers import SceneEntityCfg

    from locotouch_amd.compat.scene_views import TermEnv
    from tests.oracle_vec_env import OracleVecEnv

    n = 128
    lt = _abi.preset_cfg(TASK, num_envs=n, seed=11)
    lt.debug_terms = 1
    lt.reward_weight[C["LT_R_OBJECT_XY_VELOCITY"]] = -0.01
    lt.reward_weight[C["LT_R_OBJECT_Z_CONTACT"]] = -0.01
    vec = OracleVecEnv(TASK, cfg=lt)
    te = TermEnv(vec)
    sc = lambda name, **kw: (lambda c: (c.resolve(te.scene), c)[1])(SceneEntityCfg(name, **kw))  # noqa: E731
    g = torch.Generator().manual_seed(5)
    checks = 0
    for t in range(40):
        vec.step(0.9 * torch.randn(n, 12, generator=g))
        if t % 4:
            continue
        vec.o.eval_terms()
        fused = vec.field("LT_F_REWARD_TERMS").reshape(n, -1)
        bits = vec.field("LT_F_TERM_BITS")
        want = {
            "LT_R_FOOT_SLIP": ref.foot_slipping_ngt(te, threshold=0.5, asset_cfg=sc("robot", body_names=".*foot"), sensor_cfg=sc("robot_contact_senosr", body_names=".*foot")),
            "LT_R_FOOT_DRAGGING": ref.foot_dragging_ngt(te, asset_cfg=sc("robot", body_names=".*foot"), height_threshold=0.03, foot_vel_xy_threshold=0.1),
            "LT_R_THIGH_CALF_COLLISION": ref.thigh_calf_collision_ngt(te, threshold=0.1, sensor_cfg=sc("robot_contact_senosr", body_names=[".*thigh", ".*calf"])),
            "LT_R_ACTION_RATE": ref.action_rate_ngt(te),
            "LT_R_OBJECT_Z_CONTACT": ref.object_lose_contact_ngt(te, sensor_cfg=sc("object_contact_sensor", body_names="Object")),
            "LT_R_OBJECT_DANGEROUS_STATE": ref.object_dangerous_state_ngt(te, x_max=0.125, y_max=0.097, z_min=0.095, roll_pitch_max=None, vel_xy_max=2.5),
            "LT_R_JOINT_POSITION_LIMIT": ref.joint_position_limit_ngt(te, asset_cfg=sc("robot")),
            "LT_R_JOINT_TORQUE": ref.joint_torque_ngt(te, asset_cfg=sc("robot")),
        }
        for k, v in want.items():
            torch.testing.assert_close(v.float(), fused[:, C[k]], rtol=2e-4, atol=2e-5, msg=lambda m, k=k: f"{k}: {m}")
        # the reference's termination functions against the fused bits (terminations.py:10-23)
        assert torch.equal(ref.object_below_robot(te), ((bits >> C["LT_T_OBJECT_BELOW_ROBOT"]) & 1).bool())
        roll = ref.bad_roll(te, limit_angle=float(lt.term_object_roll_limit), asset_cfg=sc("object"))
        assert int((roll != ((bits >> C["LT_T_OBJECT_BAD_ROLL"]) & 1).bool()).sum()) == 0
        # roll_pitch_max: the branch the fused term does not implement, against a hand computation on the same views
        od = te.scene["object"].data
        base = ref.object_dangerous_state_ngt(te, x_max=0.125, y_max=0.097, z_min=0.095, roll_pitch_max=None, vel_xy_max=2.5)
        tilt = ref.object_dangerous_state_ngt(te, x_max=0.125, y_max=0.097, z_min=0.095, roll_pitch_max=20.0, vel_xy_max=2.5)
        assert torch.equal(tilt, base | (torch.acos(-od.projected_gravity_b[:, 2]).abs() > np.deg2rad(20.0)))
        checks += 1
    assert checks == 10


def test_terms_under_fused_names_that_the_kernel_cannot_honour_go_to_the_slow_path(rt):
    """VERDICT r03 missing #4: `object_dangerous_state(roll_pitch_max=...)`, `work_only_when_cmd = 0`, the roll+pitch object terms and
    user TIME-OUT terminations were refused (UnsupportedCfg); now the cfg's own function serves them on the views."""
    import locotouch.mdp as ref
    from isaaclab.managers import SceneEntityCfg
    from isaaclab.managers import TerminationTermCfg as DoneTerm

    from locotouch_amd.compat import cfg_translate as T
    from locotouch_amd.compat.runtime import ManagedEnv
    from tests.oracle_vec_env import OracleVecEnv

    n = 64
    cfg = rt.load_cfg_from_registry(TASK, "env_cfg_entry_point")
    cfg.scene.num_envs = n
    cfg.rewards.object_dangerous_state.params["roll_pitch_max"] = 25.0
    cfg.rewards.object_xy_position.params["work_only_when_cmd"] = 0
    cfg.rewards.object_roll_pitch_angle.func = ref.object_relative_roll_pitch_angle_ngt
    cfg.rewards.object_roll_pitch_velocity.func = ref.object_relative_roll_pitch_velocity_ngt

    def long_enough(env, steps: int):
        return env.episode_length_buf >= steps

    cfg.terminations.user_time_out = DoneTerm(func=long_enough, time_out=True, params={"steps": 9})
    with pytest.raises(T.UnsupportedCfg):
        T.translate(cfg)  # the strict form still refuses
    lt, sizes = rt.translate_env_cfg(TASK, cfg)
    assert sorted(t[0] for t in lt.extra_reward_terms) == ["object_dangerous_state", "object_roll_pitch_angle", "object_roll_pitch_velocity", "object_xy_position"]
    for k in ("LT_R_OBJECT_DANGEROUS_STATE", "LT_R_OBJECT_XY_POSITION", "LT_R_OBJECT_ROLL_PITCH_ANGLE", "LT_R_OBJECT_ROLL_PITCH_VELOCITY"):
        assert lt.reward_weight[C[k]] == 0.0  # the fused implementation stays off: the term is not counted twice
    assert lt.danger_x_max == pytest.approx(0.125)  # still what the gait-with-object class reads (rewards.py:380-381)
    assert [(t[0], t[3]) for t in lt.extra_termination_terms] == [("user_time_out", True)]
    vec = OracleVecEnv(TASK, cfg=lt, object_sizes=sizes)
    plain = OracleVecEnv(TASK, cfg=lt, object_sizes=sizes)
    env = ManagedEnv(TASK, cfg, vec, extra_rewards=lt.extra_reward_terms, extra_terminations=lt.extra_termination_terms)
    g = torch.Generator().manual_seed(2)
    timed_out = 0
    for t in range(24):
        act = 0.5 * torch.randn(n, 12, generator=g)
        _, rew, dones, extras = env.step(act)
        bits = vec.field("LT_F_TERM_BITS")
        user_to = ((bits >> C["LT_T_USER_TIME_OUT"]) & 1).bool()
        # a user time-out ends the env by TIME-OUT: not `terminated`, reported in time_outs (what PPO bootstraps on)
        assert bool((extras["time_outs"][user_to]).all()) and bool((dones[user_to] != 0).all())
        only = user_to & (((bits & ~(1 << C["LT_T_USER_TIME_OUT"])) & 0xFF) == 0)
        assert not bool(vec.field("LT_F_TERMINATED")[only].any())
        timed_out += int(user_to.sum())
        if t < 9:
            assert not bool(user_to.any())
        keep = (dones == 0).float()
        od, rd = env.extra.env.scene["object"].data, env.extra.env.scene["robot"].data
        # hand computation of the four slow-path terms on the views (the cfg's own weights)
        if t == 5:
            from locotouch_amd.compat import math as M

            rel = M.quat_apply_inverse(rd.root_quat_w, od.root_pos_w - rd.root_pos_w)
            relv = M.quat_apply_inverse(rd.root_quat_w, od.root_lin_vel_w - rd.root_lin_vel_w)
            danger = (rel[:, 0].abs() > 0.125) | (rel[:, 1].abs() > 0.097) | (rel[:, 2] < 0.095) | (relv[:, :2].norm(dim=1) > 2.5) | \
                (torch.acos(-od.projected_gravity_b[:, 2]).abs() > np.deg2rad(25.0))
            torch.testing.assert_close(env.extra.last_values["object_dangerous_state"], danger.float())
            torch.testing.assert_close(env.extra.last_values["object_xy_position"], (od.root_pos_w - rd.root_pos_w)[:, :2].norm(dim=1))
        _ = keep, rew
    assert timed_out >= n // 2, "the user time-out term must have ended episodes"
    _ = plain
