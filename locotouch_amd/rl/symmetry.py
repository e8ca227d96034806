"""The left-right mirror of the Go1 tasks as a SIGNED PERMUTATION of observation and action columns, and the reference's
`data_augmentation_func` built on it (loco_rl/loco_rl/algorithms/ppo.py:232-237,310-326).

Under the reflection y -> -y of the trunk frame a vector keeps x, z and flips y, a pseudo-vector (an angular velocity, the axis of
a rotation) flips x, z and keeps y, and the legs trade places FR <-> FL, RR <-> RL with the hip joints (x axis) changing sign.
Every observation term of the two registered task families is such a quantity, in every one of its history copies, so

    mirrored[c] = sign[c] * row[src[c]]

with one (src, sign) table per row kind.  The table is built from the env's own description - `lt_cfg.obs_history`, the task,
the term order and widths compat/cfg_translate.py enforces and distill/export.py publishes, the joint names of
compat/scene_views.py - never from literal column numbers.  The model is only approximately mirror-symmetric:
the map is exact on the observation algebra and approximate on the dynamics.

    symmetry_cfg = dict(use_data_augmentation=True, use_mirror_loss=False, mirror_loss_coeff=0.0,
                        data_augmentation_func="locotouch_amd.rl.symmetry:mirror_go1")
"""
from __future__ import annotations

import importlib
from typing import NamedTuple

import torch

MIRROR_GO1 = "locotouch_amd.rl.symmetry:mirror_go1"
_MIRROR_LEG = {"FR": "FL", "FL": "FR", "RR": "RL", "RL": "RR"}
# frame maps of the non-joint terms, (source component, sign) per component
_VECTOR, _PSEUDO = (1.0, -1.0, 1.0), (-1.0, 1.0, -1.0)
_FRAME_SIGNS = {
    "velocity_commands": (1.0, -1.0, -1.0),  # (vx, vy, wz): a vector's x, y and a pseudo-vector's z
    "base_ang_vel": _PSEUDO,
    "projected_gravity": _VECTOR,
    # position, linear velocity, quaternion wxyz (w and the rotation axis, a pseudo-vector), angular velocity (mdp/observations.py:55-59)
    "object_state": _VECTOR + _VECTOR + (1.0,) + _PSEUDO + _PSEUDO,
}
_JOINT_TERMS = ("joint_pos", "joint_vel", "last_action")


class MirrorTables(NamedTuple):
    """CPU tables: int32 src[D], float32 sign[D] for the policy rows, the critic rows and the actions."""
    policy_src: torch.Tensor
    policy_sign: torch.Tensor
    critic_src: torch.Tensor
    critic_sign: torch.Tensor
    action_src: torch.Tensor
    action_sign: torch.Tensor

    def of(self, kind: str):
        return getattr(self, kind + "_src"), getattr(self, kind + "_sign")


def string_to_callable(name: str):
    """`module:function` -> the function (the reference's loco_rl.utils.string_to_callable form)"""
    try:
        mod, attr = name.split(":")
        fn = getattr(importlib.import_module(mod), attr)
    except (ValueError, ImportError, AttributeError) as e:
        raise ValueError(f"cannot resolve {name!r} to a callable (expected 'module:function'): {e}") from None
    if not callable(fn):
        raise ValueError(f"{name!r} is not callable")
    return fn


def joint_mirror(joint_names=None):
    """(src, sign) lists of the joint map from the joint NAMES (default: the order the project exposes, compat/scene_views.py
    JOINT_NAMES): joint `<x>_<LEG>_<part>_joint` takes the value of the same part of the mirrored leg, negated for a hip."""
    if joint_names is None:
        from ..compat.scene_views import JOINT_NAMES as joint_names
    parsed = []
    for n in joint_names:
        parts = n.split("_")
        leg = next((p for p in parts if p in _MIRROR_LEG), None)
        part = next((p for p in parts if p in ("hip", "thigh", "calf")), None)
        if leg is None or part is None:
            raise ValueError(f"mirror_tables: the joint {n!r} has no mirror rule (expected <x>_<FR|FL|RR|RL>_<hip|thigh|calf>_joint)")
        parsed.append((leg, part))
    src, sign = [], []
    for leg, part in parsed:
        src.append(parsed.index((_MIRROR_LEG[leg], part)))
        sign.append(-1.0 if part == "hip" else 1.0)
    return src, sign


def _lt_cfg(env):
    """the lt_cfg behind `env`: the HIP env itself or one of the scripts' wrappers around it"""
    seen = []
    for e in (env, getattr(env, "vec", None), getattr(env, "unwrapped", None), getattr(getattr(env, "unwrapped", None), "vec", None)):
        cfg = getattr(e, "cfg", None)
        if cfg is not None and hasattr(cfg, "obs_history") and hasattr(cfg, "task"):
            return cfg
        seen.append(type(e).__name__)
    raise ValueError(f"mirror_tables: no lt_cfg behind the env ({' / '.join(seen)}): its observation layout is unknown")


def mirror_tables(env) -> MirrorTables:
    from .. import _abi
    from ..distill.export import OBS_LAYOUT, OBS_TERMS

    cfg = _lt_cfg(env)
    user = list(getattr(cfg, "extra_observation_terms", None) or ())
    if user:
        names = [f"{o.get('group', '?')}.{o.get('name', '?')}" if isinstance(o, dict) else str(o) for o in user]
        raise ValueError(f"mirror_tables: the env carries extra_observation_terms {names}: their mirror rule is unknown")
    task = int(cfg.task)
    if task == _abi.CONSTS["LT_TASK_LOCOMOTION"]:
        has_obj = False
    elif task == _abi.CONSTS["LT_TASK_TRANSPORT_TEACHER"]:
        has_obj = True
    else:
        raise ValueError(f"mirror_tables: task {task} has no mirror rule (LT_TASK_LOCOMOTION and LT_TASK_TRANSPORT_TEACHER have)")
    if int(getattr(cfg, "tactile_enabled", 0)):
        raise ValueError("mirror_tables: the tactile observation groups of the student tasks have no mirror rule")
    history = int(cfg.obs_history)
    if history < 1:
        raise ValueError(f"mirror_tables: obs_history is {history}")
    jsrc, jsign = joint_mirror()
    src, sign, off = [], [], 0
    for name, dim in OBS_TERMS:
        if name == "object_state" and not has_obj:
            continue
        if name in _JOINT_TERMS:
            fsrc, fsign = jsrc, jsign
        elif name in _FRAME_SIGNS:
            fsrc, fsign = list(range(dim)), list(_FRAME_SIGNS[name])
        else:
            raise ValueError(f"mirror_tables: the observation term {name!r} has no mirror rule")
        if len(fsrc) != dim or (name == "object_state" and sum(OBS_LAYOUT["object_state_terms"]) != dim):
            raise ValueError(f"mirror_tables: the observation term {name!r} is {dim} wide, its mirror rule covers {len(fsrc)}")
        for h in range(history):  # term-major: the term's frames oldest -> newest, the same frame map for each
            src += [off + h * dim + s for s in fsrc]
            sign += fsign
        off += dim * history
    num_obs = getattr(env, "num_obs", None)
    if num_obs is not None and int(num_obs) != off:
        raise ValueError(f"mirror_tables: the env's rows are {int(num_obs)} wide, the known terms cover {off}")
    osrc, osign = torch.tensor(src, dtype=torch.int32), torch.tensor(sign, dtype=torch.float32)
    # the critic group holds the policy group's terms with corruption off (compat/cfg_translate.py): the same table today
    return MirrorTables(osrc, osign, osrc.clone(), osign.clone(), torch.tensor(jsrc, dtype=torch.int32), torch.tensor(jsign, dtype=torch.float32))


_cache: dict = {}


def _tables_on(env, device):
    cfg = _lt_cfg(env)
    user = getattr(cfg, "extra_observation_terms", None) or ()
    key = (int(cfg.task), int(cfg.obs_history), int(getattr(cfg, "tactile_enabled", 0)), len(user), getattr(env, "num_obs", None), str(device))
    if key not in _cache:
        t = mirror_tables(env)
        _cache[key] = {k: (t.of(k)[0].to(device=device, dtype=torch.int64), t.of(k)[1].to(device)) for k in ("policy", "critic", "action")}
    return _cache[key]


def mirror_go1(obs, actions, env, is_critic=False):
    """The reference's data-augmentation contract: (obs_aug, actions_aug), each [2 B, .] as [original; mirrored]; None in, None out.
    Any device and floating dtype; the mirrored half is a column gather and a multiplication by +-1, exact in every format."""
    def both(x, kind):
        if x is None:
            return None
        src, sign = _tables_on(env, x.device)[kind]
        if x.shape[-1] != src.numel():
            raise ValueError(f"mirror_go1: {kind} rows are {x.shape[-1]} wide, the env's table covers {src.numel()}")
        return torch.cat((x, x[..., src] * sign.to(x.dtype)), dim=0)

    return both(obs, "critic" if is_critic else "policy"), both(actions, "action")
