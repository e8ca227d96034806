"""CPU-only checks of the observation normaliser's C ABI (include/lt_obs_norm.h, part of the lt_env.h ABI): the binding is derived
from the header, the library exports the entry points, and bad arguments are refused on the host before any launch."""
import ctypes
import re

from locotouch_amd import _abi

_vp, _int, _i64, _f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
C = _abi.CONSTS


def test_header_is_part_of_the_abi_and_its_binding_is_derived():
    assert C["LT_ABI_VERSION"] == 21 and _abi.load().lt_abi_version() == 21
    assert re.search(r'^#include "lt_obs_norm.h"', open(_abi.HEADER).read(), flags=re.M)
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.OBS_NORM_HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_\w+)\s*\([^()]*\)\s*;", src))
    assert protos == set(_abi.OBS_NORM_SIGNATURES) == {"lt_obs_norm_ws_floats", "lt_obs_norm_update", "lt_obs_norm_apply"}
    S = _abi.OBS_NORM_SIGNATURES
    net = [_vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    assert S["lt_obs_norm_ws_floats"] == (_int, [_i64, _int, ctypes.POINTER(ctypes.c_size_t)])
    assert S["lt_obs_norm_update"] == (_int, [_i64, _int, _i64, ctypes.c_double] + net + net + [_vp])
    assert S["lt_obs_norm_apply"] == (_int, [_vp, _i64, _int, _vp, _i64, _i64, _vp, _vp])
    lib = _abi.load()
    for name, (restype, argtypes) in S.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name


def test_entry_points_validate_their_arguments_before_touching_the_gpu():
    lib = _abi.load()
    one, null, bad = _vp(16), _vp(None), C["LT_EINVAL"]
    floats = ctypes.c_size_t()
    # header (4) + 12 column vectors (f64 state, last f32 values, the values before the merge) + one f64 (mean, M2) pair per 128 rows,
    # columns padded to a multiple of 4
    assert lib.lt_obs_norm_ws_floats(4096, 348, ctypes.byref(floats)) == 0 and floats.value == 4 + (12 + 4 * 32) * 348
    assert lib.lt_obs_norm_ws_floats(1, 7, ctypes.byref(floats)) == 0 and floats.value == 4 + 16 * 8
    assert lib.lt_obs_norm_ws_floats(4100, 270, ctypes.byref(floats)) == 0 and floats.value == 4 + (12 + 4 * 33) * 272
    assert lib.lt_obs_norm_ws_floats(0, 7, ctypes.byref(floats)) == bad and lib.lt_obs_norm_ws_floats(16, 1025, ctypes.byref(floats)) == bad
    net = [one, 348, one, one, one, one, one, one, one]
    none = [null, 0, null, null, null, null, null, null, null]
    assert lib.lt_obs_norm_update(0, 1, -1, 1e-2, *net, *none, null) == bad
    assert lib.lt_obs_norm_update(64, 1, -1, 0.0, *net, *none, null) == bad
    assert lib.lt_obs_norm_update(64, 1, -1, 1e-2, *(net[:1] + [1025] + net[2:]), *none, null) == bad
    assert lib.lt_obs_norm_update(64, 1, -1, 1e-2, *(net[:5] + [null] + net[6:]), *none, null) == bad     # no count
    assert lib.lt_obs_norm_update(64, 1, -1, 1e-2, *(net[:8] + [null]), *none, null) == bad               # merging without a workspace
    assert lib.lt_obs_norm_update(64, 1, -1, 1e-2, *(net[:8] + [_vp(20)]), *none, null) == bad            # misaligned workspace
    assert lib.lt_obs_norm_update(64, 1, -1, 1e-2, *net, *(net[:2] + [null] + net[3:]), null) == bad      # second network incomplete
    assert b"lt_obs_norm_update" in lib.lt_last_error()
    assert lib.lt_obs_norm_apply(null, 64, 348, one, 696, 64, one, null) == bad
    assert lib.lt_obs_norm_apply(one, 64, 348, one, 696, 0, one, null) == bad
    assert lib.lt_obs_norm_apply(one, 64, 2048, one, 696, 64, one, null) == bad and b"lt_obs_norm_apply" in lib.lt_last_error()


def test_runner_without_the_hip_env_keeps_the_eager_normaliser():
    """A CPU env is not served by the fused rollout, with or without the switch: `_make_fused` is None and the torch class runs."""
    import torch
    from locotouch_amd.rl import EmpiricalNormalization, OnPolicyRunner
    from tests.rl_synth import POLICY_CFG, PPO_CFG

    class Env:
        num_envs, num_actions, max_episode_length = 8, 12, 10
        device = "cpu"

        def __init__(self):
            self.episode_length_buf = torch.zeros(8, dtype=torch.long)

        def get_observations(self):
            o = torch.randn(8, 20)
            return o, {"observations": {"critic": o}}

        def step(self, a):
            o = torch.randn(8, 20)
            return o, torch.zeros(8), torch.zeros(8, dtype=torch.long), {"observations": {"critic": o}, "time_outs": torch.zeros(8)}

    torch.manual_seed(0)
    cfg = {"algorithm": dict(PPO_CFG), "policy": dict(POLICY_CFG), "num_steps_per_env": 4, "empirical_normalization": True}
    runner = OnPolicyRunner(Env(), cfg, log_dir=None, device="cpu")
    assert runner._make_fused() is None and isinstance(runner.obs_normalizer, EmpiricalNormalization)
    runner.learn(1)
    assert int(runner.obs_normalizer.count) == 8 * (1 + 4)
