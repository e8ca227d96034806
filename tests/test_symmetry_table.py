"""The mirror map of locotouch_amd/rl/symmetry.py for both registered task families (locomotion: 270-wide rows; transport teacher:
348-wide rows), without a GPU: an involution, term by term what a left-right reflection does to a hand-written frame, the same in every
history copy, with the poses and patterns that must be fixed points, on the joint order the project exposes, and the reference's
`data_augmentation_func` contract."""
import os
import re

import pytest
import torch

from locotouch_amd import _abi
from locotouch_amd.compat.scene_views import JOINT_NAMES
from locotouch_amd.distill.export import OBS_LAYOUT, OBS_TERMS
from locotouch_amd.rl import symmetry as S

TASKS = {"locomotion": ("Isaac-Locomotion-LocoTouch-v1", 270), "teacher": ("Isaac-RandCylinderTransportTeacher-LocoTouch-v1", 348)}
FR, FL, RR, RL = 0, 1, 2, 3  # include/lt_go1_model.h:5 "Leg order FR, FL, RR, RL"; joint j = 4 * type + leg


class _Env:
    """what `mirror_tables` reads of an env: its lt_cfg and its row width"""

    def __init__(self, family, **over):
        task, width = TASKS[family]
        self.cfg = _abi.preset_cfg(task)
        self.num_obs = width
        for k, v in over.items():
            setattr(self.cfg, k, v)


@pytest.fixture(scope="module", params=list(TASKS))
def env(request):
    return _Env(request.param)


def _mirror(x, src, sign):
    return x[..., src.long()] * sign.to(x.dtype)


def _frame(env):
    """a hand-written newest frame per term, and what its mirror must be"""
    j = torch.arange(12, dtype=torch.float32)
    joints = lambda base: base + j  # noqa: E731  (value = base + joint index: tells every joint apart)

    def mirrored_joints(base):
        v = joints(base)
        out = torch.empty(12)
        for typ in range(3):
            for leg, other in ((FR, FL), (FL, FR), (RR, RL), (RL, RR)):
                out[4 * typ + leg] = (-1.0 if typ == 0 else 1.0) * v[4 * typ + other]
        return out

    frame = {"velocity_commands": (torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1.0, -2.0, -3.0])),
             "base_ang_vel": (torch.tensor([4.0, 5.0, 6.0]), torch.tensor([-4.0, 5.0, -6.0])),
             "projected_gravity": (torch.tensor([7.0, 8.0, 9.0]), torch.tensor([7.0, -8.0, 9.0])),
             "joint_pos": (joints(10.0), mirrored_joints(10.0)), "joint_vel": (joints(30.0), mirrored_joints(30.0)),
             "last_action": (joints(50.0), mirrored_joints(50.0)),
             # position, linear velocity, quaternion wxyz, angular velocity
             "object_state": (torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0]),
                              torch.tensor([1.0, -2.0, 3.0, 4.0, -5.0, 6.0, 7.0, -8.0, 9.0, -10.0, -11.0, 12.0, -13.0]))}
    return {k: v for k, v in frame.items() if k != "object_state" or env.num_obs == 348}


def _terms(env):
    """(name, dim, first column) of the env's terms, term-major blocks of dim * history columns"""
    out, off, H = [], 0, int(env.cfg.obs_history)
    for name, dim in OBS_TERMS:
        if name == "object_state" and env.num_obs != 348:
            continue
        out.append((name, dim, off))
        off += dim * H
    assert off == env.num_obs
    return out


def test_the_layout_the_table_is_built_from(env):
    assert [d for _, d in OBS_TERMS] == [3, 3, 3, 12, 12, 12, 13] == OBS_LAYOUT["term_dims"] and int(env.cfg.obs_history) == 6 == OBS_LAYOUT["history_length"]
    assert OBS_LAYOUT["object_state_terms"] == [3, 3, 4, 3]


def test_the_joint_order_is_the_one_the_project_exposes():
    # compat/scene_views.py JOINT_NAMES: type-major, legs FR, FL, RR, RL within a type - joint j = 4 * type + leg
    assert len(JOINT_NAMES) == 12
    for j, name in enumerate(JOINT_NAMES):
        assert ("hip", "thigh", "calf")[j // 4] in name and ("FR", "FL", "RR", "RL")[j % 4] in name, (j, name)
    assert "a_FR, b_FL, c_RR, d_RL per joint type" in OBS_LAYOUT["joint_order"]
    src, sign = S.joint_mirror()
    assert src == [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10] and sign == [-1.0] * 4 + [1.0] * 8
    # a renamed or reordered robot is followed, an unknown joint refused by name
    assert S.joint_mirror(["x_FL_calf_joint", "x_FR_calf_joint", "x_FR_hip_joint", "x_FL_hip_joint"]) == ([1, 0, 3, 2], [1.0, 1.0, -1.0, -1.0])
    with pytest.raises(ValueError, match="tail_joint"):
        S.joint_mirror(["a_FR_hip_joint", "tail_joint"])


def test_tables_are_involutions_bit_for_bit(env):
    t = S.mirror_tables(env)
    gen = torch.Generator().manual_seed(1)
    for kind, width in (("policy", env.num_obs), ("critic", env.num_obs), ("action", 12)):
        src, sign = t.of(kind)
        assert src.dtype == torch.int32 and sign.dtype == torch.float32 and src.shape == sign.shape == (width,) and not src.is_cuda
        assert sorted(src.tolist()) == list(range(width)) and set(sign.tolist()) <= {1.0, -1.0}
        for dtype in (torch.float32, torch.float64, torch.bfloat16):
            x = torch.randn(7, width, generator=gen).to(dtype)
            twice = _mirror(_mirror(x, src, sign), src, sign)
            assert torch.equal(twice.contiguous().view(torch.uint8), x.contiguous().view(torch.uint8))
            assert not torch.equal(_mirror(x, src, sign), x)
    assert torch.equal(t.policy_src, t.critic_src) and torch.equal(t.policy_sign, t.critic_sign)  # the same terms, corruption off


def test_a_hand_written_frame_is_mirrored_term_by_term_in_every_history_copy(env):
    t = S.mirror_tables(env)
    H = int(env.cfg.obs_history)
    frame = _frame(env)
    row, want = torch.zeros(env.num_obs), torch.zeros(env.num_obs)
    for name, dim, off in _terms(env):
        for h in range(H):  # copy h holds (h + 1) * the frame: every history copy is told apart and must use the same frame map
            row[off + h * dim: off + (h + 1) * dim] = (h + 1) * frame[name][0]
            want[off + h * dim: off + (h + 1) * dim] = (h + 1) * frame[name][1]
    got = _mirror(row, t.policy_src, t.policy_sign)
    for name, dim, off in _terms(env):
        assert torch.equal(got[off:off + dim * H], want[off:off + dim * H]), name
    a, am = frame["last_action"]
    assert torch.equal(_mirror(a, t.action_src, t.action_sign), am)
    # a column never leaves its term's history copy
    for name, dim, off in _terms(env):
        for h in range(H):
            cols = t.policy_src[off + h * dim: off + (h + 1) * dim]
            assert int(cols.min()) >= off + h * dim and int(cols.max()) < off + (h + 1) * dim, (name, h)


def test_fixed_points_and_trot_pairs(env):
    t = S.mirror_tables(env)
    header = open(os.path.join(os.path.dirname(_abi.HEADER), "lt_go1_model.h")).read()
    init = re.search(r"#define LT_JOINT_DEFAULT_INIT \{(.*)\}\s*$", header, flags=re.M).group(1)
    legs = [[float(v.rstrip("f")) for v in leg.split(",")] for leg in re.findall(r"\{([^{}]*)\}", init)]
    assert len(legs) == 4 and all(len(leg) == 3 for leg in legs)
    default = torch.tensor([legs[j % 4][j // 4] for j in range(12)])  # joint j = 4 * type + leg
    assert default[:4].tolist() == pytest.approx([-0.1, 0.1, -0.1, 0.1])
    assert torch.equal(_mirror(default, t.action_src, t.action_sign), default), "the default joint pose is its own mirror image"
    zero = torch.zeros(12)
    assert torch.equal(_mirror(zero, t.action_src, t.action_sign).abs(), zero)
    # trot pairs (FR, RL) and (FL, RR): an action on one pair's joints alone lands on the other pair's joints alone
    pair_a = torch.tensor([1.0 if j % 4 in (FR, RL) else 0.0 for j in range(12)])
    pair_b = torch.tensor([1.0 if j % 4 in (FL, RR) else 0.0 for j in range(12)])
    assert torch.equal(_mirror(pair_a, t.action_src, t.action_sign).abs(), pair_b) and torch.equal(_mirror(pair_b, t.action_src, t.action_sign).abs(), pair_a)
    if env.num_obs == 348:
        non_contact = torch.tensor([0.0] * 6 + [1.0] + [0.0] * 6)
        off = [o for n, _, o in _terms(env) if n == "object_state"][0]
        row = torch.zeros(env.num_obs)
        row[off:off + 13 * 6] = non_contact.repeat(6)
        assert torch.equal(_mirror(row, t.policy_src, t.policy_sign).abs(), row) and float(_mirror(row, t.policy_src, t.policy_sign).sum()) == 6.0


def test_mirror_go1_honours_the_augmentation_contract(env):
    assert S.string_to_callable("locotouch_amd.rl.symmetry:mirror_go1") is S.mirror_go1 and S.MIRROR_GO1 == "locotouch_amd.rl.symmetry:mirror_go1"
    t = S.mirror_tables(env)
    B = 5
    for dtype in (torch.float32, torch.float64):
        obs, act = torch.randn(B, env.num_obs, dtype=dtype), torch.randn(B, 12, dtype=dtype)
        o, a = S.mirror_go1(obs=obs, actions=act, env=env, is_critic=False)
        assert o.shape == (2 * B, env.num_obs) and a.shape == (2 * B, 12) and o.dtype == dtype and a.dtype == dtype
        assert torch.equal(o[:B], obs) and torch.equal(a[:B], act)
        assert torch.equal(o[B:], _mirror(obs, t.policy_src, t.policy_sign)) and torch.equal(a[B:], _mirror(act, t.action_src, t.action_sign))
        co, none = S.mirror_go1(obs=obs, actions=None, env=env, is_critic=True)
        assert none is None and torch.equal(co[B:], _mirror(obs, t.critic_src, t.critic_sign))
        none, a2 = S.mirror_go1(obs=None, actions=act, env=env, is_critic=False)
        assert none is None and torch.equal(a2, a)
    with pytest.raises(ValueError, match="wide"):
        S.mirror_go1(obs=torch.zeros(2, env.num_obs + 1), actions=None, env=env)
    with pytest.raises(ValueError, match="module:function"):
        S.string_to_callable("locotouch_amd.rl.symmetry.mirror_go1")


def test_what_has_no_rule_is_refused_by_name():
    user = _Env("teacher")
    user.cfg.extra_observation_terms = [dict(group="policy", name="foot_heights", history_length=6)]
    with pytest.raises(ValueError, match=r"extra_observation_terms.*policy\.foot_heights"):
        S.mirror_tables(user)
    with pytest.raises(ValueError, match=r"extra_observation_terms.*policy\.foot_heights"):
        S.mirror_go1(torch.zeros(1, 348), None, user)
    with pytest.raises(ValueError, match="task 7"):
        S.mirror_tables(_Env("teacher", task=7))
    with pytest.raises(ValueError, match="tactile"):
        S.mirror_tables(_Env("teacher", tactile_enabled=1))
    wide = _Env("locomotion")
    wide.num_obs = 271
    with pytest.raises(ValueError, match="271"):
        S.mirror_tables(wide)
    with pytest.raises(ValueError, match="no lt_cfg"):
        S.mirror_tables(object())
