"""include/lt_ledger.h: part of the lt_env.h ABI, bound by locotouch_amd/_abi.py from the header itself; the host-only size query and
argument validation; `DeviceEpisodeLedger` and `ReplayBuffer(..., device_ledger=True)` refuse a device without the kernels.  No device is
touched: every call below is refused on the host before anything is launched (the pointers are made-up addresses that are never
dereferenced)."""
import ctypes
import os
import re
import types

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
NAMES = {"lt_ledger_state_bytes", "lt_ledger_begin", "lt_ledger_step", "lt_ledger_end"}
STATE, REWARD, DONE, EP_R, EP_L, TRAJ, OUT = 1 << 20, 1 << 30, 1 << 32, 1 << 34, 1 << 36, 1 << 38, 1 << 40


def test_header_is_part_of_the_abi_and_bound_from_itself():
    env_h = open(_abi.HEADER).read()
    assert re.search(r'^#include "lt_ledger\.h"$', env_h, flags=re.M) and os.path.samefile(_abi.LEDGER_HEADER, os.path.join(_abi.REPO, "include", "lt_ledger.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.LEDGER_HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_\w+)\s*\(", src))
    assert protos == set(_abi.LEDGER_SIGNATURES) == NAMES
    assert all(res is ctypes.c_int for res, _ in _abi.LEDGER_SIGNATURES.values())
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67 and len(_abi.OBS_NORM_SIGNATURES) == 3 and len(_abi.STUDENT_SIGNATURES) == 6
    others = set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES) | set(_abi.COLLECT_SIGNATURES)
    assert not set(_abi.LEDGER_SIGNATURES) & others
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name in NAMES:
        assert getattr(lib, name) is not None and name in _abi._calls  # exported, and launched through `_abi.call`
    fields = ["STEP", "KEPT_STEPS", "EPISODES", "TRAJS", "STOPPED_AT", "OVERFLOW", "KEEP_TARGET", "EPISODE_TARGET"]  # the 64-byte head
    assert [_abi.LEDGER_CONSTS["LT_LEDGER_" + f] for f in fields] == list(range(8)) and _abi.LEDGER_CONSTS["LT_LEDGER_HEAD_FIELDS"] == 8


@pytest.mark.parametrize("n", [1, 37, 4112])
def test_state_bytes_is_the_documented_layout(n):
    size = ctypes.c_size_t()
    _abi.call("lt_ledger_state_bytes", n, ctypes.byref(size))
    assert size.value == 64 + 8 * n + 8 * n  # head | double reward_sum[n] | int64 start[n]
    assert size.value % 16 == 0


def refused(name, args, field):
    lib = _abi.load()
    rc = getattr(lib, name)(*[_abi.ptr(x) if t is ctypes.c_void_p else x for x, t in zip(args, _abi.LEDGER_SIGNATURES[name][1])])
    assert rc == C["LT_EINVAL"], (name, field, rc)
    msg = lib.lt_last_error().decode()
    assert name in msg and re.search(rf"\b{re.escape(field)}\b", msg), msg
    with pytest.raises(RuntimeError, match=re.escape(field)):
        _abi.call(name, *args)


def step_args(**kw):
    a = dict(state=STATE, n=37, reward=REWARD, done=DONE, ep_reward=EP_R, ep_length=EP_L, ep_first=0, ep_cap=64, traj=TRAJ, traj_first=0,
             traj_cap=64, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def test_every_entry_point_refuses_n_below_one_and_a_bad_state():
    size = ctypes.c_size_t()
    for n in (0, -3):
        refused("lt_ledger_state_bytes", [n, ctypes.byref(size)], "n")
        refused("lt_ledger_begin", [STATE, n, None, -1, -1, None], "n")
        refused("lt_ledger_step", step_args(n=n), "n")
        refused("lt_ledger_end", [STATE, n, OUT, None], "n")
    refused("lt_ledger_state_bytes", [37, None], "bytes")
    for state in (None, STATE + 8):  # NULL, and 8- but not 16-byte aligned
        refused("lt_ledger_begin", [state, 37, None, -1, -1, None], "state")
        refused("lt_ledger_step", step_args(state=state), "state")
        refused("lt_ledger_end", [state, 37, OUT, None], "state")


@pytest.mark.parametrize("field, kw", [
    ("reward", dict(reward=None)),
    ("done", dict(done=None)),
    ("ep_reward", dict(ep_reward=None)),                      # a NULL list with a non-zero cap
    ("ep_length", dict(ep_length=None)),
    ("traj", dict(traj=None)),
    ("ep_cap", dict(ep_cap=-1)),                              # a negative cap
    ("ep_cap", dict(ep_reward=None, ep_length=None, ep_cap=-1)),
    ("traj_cap", dict(traj_cap=-1)),
    ("traj_cap", dict(traj=None, traj_cap=-5)),
    ("ep_first", dict(ep_first=-1)),
    ("traj_first", dict(traj_first=-1)),
    ("ep_reward", dict(ep_reward=EP_R + 4)),                  # misaligned lists
    ("traj", dict(traj=TRAJ + 4)),
])
def test_step_names_what_it_refuses(field, kw):
    refused("lt_ledger_step", step_args(**kw), field)


def test_end_and_begin_name_what_they_refuse():
    refused("lt_ledger_end", [STATE, 37, None, None], "reward_sums_out")
    refused("lt_ledger_begin", [STATE, 37, REWARD + 2, -1, -1, None], "reward_sums_in")


def test_the_python_front_refuses_a_device_without_the_kernels():
    import torch

    from locotouch_amd.distill import DeviceEpisodeLedger, ReplayBuffer, TactileRecorder

    with pytest.raises(ValueError, match="CUDA"):
        DeviceEpisodeLedger("cpu", 37, 16)
    cpu_env = types.SimpleNamespace(num_envs=37, device=torch.device("cpu"))
    rec = TactileRecorder("cpu", 37, 442, 3, 7)
    assert ReplayBuffer(cpu_env, rec, 270)._ledger is None   # the default keeps the books on the host
    with pytest.raises(ValueError, match="CUDA"):
        ReplayBuffer(cpu_env, rec, 270, device_ledger=True)
