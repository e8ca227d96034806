"""include/lt_bc.h: part of the lt_env.h ABI, bound by locotouch_amd/_abi.py from the header itself; the host-only size query and the
argument validation of every entry point; the Python fronts refuse a device without the kernels.  No device is touched: every call below
is refused on the host before anything is launched (the pointers are made-up addresses that are never dereferenced)."""
import ctypes
import os
import re
import types

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
NAMES = {"lt_bc_gather", "lt_bc_loss_ws_floats", "lt_bc_loss_forward", "lt_bc_loss_backward", "lt_adamw_step"}
A0 = 1 << 30  # made-up, 16-byte aligned addresses


def addr(k):
    return A0 + (k << 24)


def test_header_is_part_of_the_abi_and_bound_from_itself():
    env_h = open(_abi.HEADER).read()
    assert re.search(r'^#include "lt_bc\.h"$', env_h, flags=re.M) and os.path.samefile(_abi.BC_HEADER, os.path.join(_abi.REPO, "include", "lt_bc.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.BC_HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_\w+)\s*\(", src))
    assert protos == set(_abi.BC_SIGNATURES) == NAMES
    assert all(res is ctypes.c_int for res, _ in _abi.BC_SIGNATURES.values())
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67 and len(_abi.OBS_NORM_SIGNATURES) == 3 and len(_abi.STUDENT_SIGNATURES) == 6
    others = (set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES) | set(_abi.COLLECT_SIGNATURES)
              | set(_abi.LEDGER_SIGNATURES) | set(_abi.CNN_TRAIN_SIGNATURES))
    assert not set(_abi.BC_SIGNATURES) & others
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name in NAMES:
        assert getattr(lib, name) is not None and name in _abi._calls  # exported, and launched through `_abi.call`
    fields = ["LOSS", "ACTION_MSE", "ACTION_MAE", "DENOM"]  # the stats record
    assert [_abi.BC_CONSTS["LT_BC_" + f] for f in fields] == list(range(4)) and _abi.BC_CONSTS["LT_BC_STATS_FIELDS"] == 4


@pytest.mark.parametrize("R", [1, 256, 257, 48000])
def test_ws_floats_is_four_per_group_of_rows(R):
    size = ctypes.c_size_t()
    _abi.call("lt_bc_loss_ws_floats", R, ctypes.byref(size))
    assert size.value == 4 * -(-R // _abi.BC_CONSTS["LT_BC_ROWS_PER_GROUP"])


def refused(name, args, field):
    lib = _abi.load()
    rc = getattr(lib, name)(*[_abi.ptr(x) if t is ctypes.c_void_p else x for x, t in zip(args, _abi.BC_SIGNATURES[name][1], strict=True)])
    assert rc == C["LT_EINVAL"], (name, field, rc)
    msg = lib.lt_last_error().decode()
    assert msg and name in msg and re.search(rf"\b{re.escape(field)}\b", msg), msg
    with pytest.raises(RuntimeError, match=re.escape(field)):
        _abi.call(name, *args)


def gather_args(**kw):
    a = dict(policy=addr(1), tactile=addr(2), rows_total=100, pe=348, td=442, first=addr(3), len=addr(4), num_trajs=5, traj_idx=addr(5), nb=3,
             num_envs=5, L=7, B=3, pol=addr(6), tac=addr(7), mask=addr(8), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def forward_args(**kw):
    a = dict(pred=addr(1), target=addr(2), W=64, sa=addr(3), ta=addr(4), A=12, mask=addr(5), R=21, clip_range=1.0, action_scale=0.25,
             stats=addr(6), ws=addr(7), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def backward_args(**kw):
    a = dict(pred=addr(1), target=addr(2), W=64, mask=addr(5), R=21, g=addr(8), stats=addr(6), d_pred=addr(9), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def adamw_args(**kw):
    a = dict(params=addr(1), grads=addr(2), exp_avg=addr(3), exp_avg_sq=addr(4), n=1000, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
             weight_decay=1e-2, step=1, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("field, kw", [
    ("L", dict(L=0)), ("L", dict(L=-2)), ("B", dict(B=0)), ("B", dict(B=-1)), ("L", dict(L=1 << 20, B=1 << 20)),
    ("rows_total", dict(rows_total=0)), ("pe", dict(pe=0)), ("td", dict(td=-4)), ("num_trajs", dict(num_trajs=0)),
    ("nb", dict(nb=4)), ("nb", dict(nb=-1)), ("num_envs", dict(num_envs=0)),
    ("policy", dict(policy=None)), ("tactile", dict(tactile=None)), ("first", dict(first=None)), ("len", dict(len=None)),
    ("traj_idx", dict(traj_idx=None)), ("pol", dict(pol=None)), ("tac", dict(tac=None)), ("mask", dict(mask=None)),
    ("policy", dict(policy=addr(1) + 2)), ("first", dict(first=addr(3) + 4)), ("traj_idx", dict(traj_idx=addr(5) + 4)),
])
def test_gather_names_what_it_refuses(field, kw):
    refused("lt_bc_gather", gather_args(**kw), field)


@pytest.mark.parametrize("field, kw", [
    ("R", dict(R=0)), ("R", dict(R=-7)), ("R", dict(R=1 << 31)), ("W", dict(W=0)), ("W", dict(W=4097)), ("A", dict(A=0)), ("A", dict(A=4097)),
    ("pred", dict(pred=None)), ("target", dict(target=None)), ("sa", dict(sa=None)), ("ta", dict(ta=None)), ("mask", dict(mask=None)),
    ("stats", dict(stats=None)), ("stats", dict(stats=addr(6) + 8)), ("ws", dict(ws=None)), ("pred", dict(pred=addr(1) + 1)),
])
def test_loss_forward_names_what_it_refuses(field, kw):
    refused("lt_bc_loss_forward", forward_args(**kw), field)


@pytest.mark.parametrize("field, kw", [
    ("R", dict(R=0)), ("R", dict(R=-1)), ("W", dict(W=0)), ("W", dict(W=5000)), ("pred", dict(pred=None)), ("target", dict(target=None)),
    ("mask", dict(mask=None)), ("g", dict(g=None)), ("stats", dict(stats=None)), ("d_pred", dict(d_pred=None)), ("d_pred", dict(d_pred=addr(9) + 2)),
])
def test_loss_backward_names_what_it_refuses(field, kw):
    refused("lt_bc_loss_backward", backward_args(**kw), field)


@pytest.mark.parametrize("field, kw", [
    ("n", dict(n=0)), ("n", dict(n=-64)), ("step", dict(step=0)), ("params", dict(params=None)), ("grads", dict(grads=None)),
    ("exp_avg", dict(exp_avg=None)), ("exp_avg_sq", dict(exp_avg_sq=None)), ("params", dict(params=addr(1) + 3)), ("lr", dict(lr=-1e-3)),
    ("beta1", dict(beta1=1.0)), ("beta2", dict(beta2=-0.1)), ("eps", dict(eps=-1.0)),
    ("weight_decay", dict(weight_decay=-1e-2)),
])
def test_adamw_names_what_it_refuses(field, kw):
    refused("lt_adamw_step", adamw_args(**kw), field)


def test_ws_floats_refuses_r_below_one_and_a_null_result():
    size = ctypes.c_size_t()
    for R in (0, -3):
        refused("lt_bc_loss_ws_floats", [R, ctypes.byref(size)], "R")
    refused("lt_bc_loss_ws_floats", [21, None], "floats")


def test_the_python_fronts_refuse_a_device_without_the_kernels(tmp_path):
    import torch

    from locotouch_amd.distill import Distillation, ReplayBuffer, Student, TactileRecorder, bc_loss, distillation_cfg
    from locotouch_amd.rl.flat_adam import FlatAdam
    from locotouch_amd.rl.flat_adamw import FlatAdamW
    from tests.distill_synth import ScriptedEnv, teacher_policy

    cpu_env = types.SimpleNamespace(num_envs=37, device=torch.device("cpu"))
    rec = TactileRecorder("cpu", 37, 442, 3, 7)
    assert ReplayBuffer(cpu_env, rec, 270)._fused_batches is False   # the default assembles batches with torch ops
    with pytest.raises(ValueError, match="CUDA"):
        ReplayBuffer(cpu_env, rec, 270, fused_batches=True)
    x = torch.zeros(7, 3, 12)
    with pytest.raises(ValueError, match="CUDA"):
        bc_loss(x, x, torch.ones(7, 3, dtype=torch.bool))
    lin = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match="CUDA"):
        FlatAdamW(torch.optim.AdamW(lin.parameters()))
    with pytest.raises(TypeError, match="AdamW"):
        FlatAdamW(torch.optim.Adam(lin.parameters()))
    with pytest.raises(TypeError, match="Adam"):
        FlatAdam(torch.optim.AdamW(lin.parameters()))   # FlatAdam keeps to torch.optim.Adam
    cfg = distillation_cfg("Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1")
    cfg.device, cfg.log_dir = "cpu", str(tmp_path)
    student = Student(cfg, 270, 442, 12, teacher_policy_inference=teacher_policy(), verbose=False)
    with pytest.raises(ValueError, match="CUDA"):
        student.enable_fused_bc_step()
    with pytest.raises(ValueError, match="CUDA"):
        Distillation(ScriptedEnv(), cfg, teacher_policy=teacher_policy(), log_dir=str(tmp_path), verbose=False, fused_bc_step=True)
    with pytest.raises(ValueError, match="fused_bc_step"):
        Distillation(ScriptedEnv(), cfg, training=False, verbose=False, fused_bc_step=True)
