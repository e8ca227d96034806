"""include/lt_cnn_train.h: bound by locotouch_amd/_abi.py from the header itself; the host-only validator and the argument validation
of every entry point.  No device is touched: every call below is refused (or answered) on the host before anything is launched (the
pointers are made-up addresses that are never dereferenced)."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
NAMES = {"lt_cnn_validate", "lt_cnn_ws_floats", "lt_cnn_forward", "lt_cnn_backward", "lt_cnn_launches"}
X, EMB, WS, P0 = 1 << 30, 1 << 32, 1 << 34, 1 << 36


def registered(**kw):
    """The registered student's stack: 2 x 17 x 13, channels 24/24/24, kernels 4/3/2, configured strides 2/1/1 with max-pool, head 64."""
    d = _abi.LtCnnDesc()
    d.img_channels, d.img_height, d.img_width, d.num_convs = 2, 17, 13, 3
    for i, (c, k, s) in enumerate(zip((24, 24, 24), (4, 3, 2), (2, 1, 1))):
        d.conv_channels[i], d.conv_kernel[i], d.conv_stride[i], d.conv_padding[i] = c, k, s, 0
    d.use_maxpool, d.conv_activation, d.conv_norm, d.head_out = 1, C["LT_ACT_RELU"], 0, 64
    for name, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(d, name)[i] = x
        else:
            setattr(d, name, v)
    return d


def pointers(cls, fill=P0):
    p = cls()
    for i in range(3):
        p.conv_w[i], p.conv_b[i] = fill + 4096 * i, fill + 4096 * i + 2048
    p.head_w, p.head_b = fill + 65536, fill + 2 * 65536
    return p


def test_header_is_bound_from_itself():
    assert os.path.samefile(_abi.CNN_TRAIN_HEADER, os.path.join(_abi.REPO, "include", "lt_cnn_train.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.CNN_TRAIN_HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_\w+)\s*\(", src))
    assert protos == set(_abi.CNN_TRAIN_SIGNATURES) == NAMES
    assert all(res is ctypes.c_int for res, _ in _abi.CNN_TRAIN_SIGNATURES.values())
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67 and len(_abi.STUDENT_SIGNATURES) == 6
    others = (set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES) | set(_abi.COLLECT_SIGNATURES)
              | set(_abi.LEDGER_SIGNATURES))
    assert not set(_abi.CNN_TRAIN_SIGNATURES) & others
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name in NAMES:
        assert getattr(lib, name) is not None
        assert (name in _abi._calls) == (name != "lt_cnn_launches")  # the value query is never launched through `_abi.call`
    assert _abi.CNN_TRAIN_VALUE_QUERIES == {"lt_cnn_launches"}
    assert _abi.CNN_TRAIN_CONSTS["LT_CNN_MAX_CONVS"] == _abi.STUDENT_CONSTS["LT_STUDENT_MAX_CONVS"]
    assert _abi.CNN_TRAIN_CONSTS["LT_CNN_TILE"] == _abi.STUDENT_CONSTS["LT_STUDENT_ENV_TILE"]
    # lt_cnn_desc is the conv-stack part of lt_student_desc, field for field
    student = [(n, t) for n, t in _abi.LtStudentDesc._fields_ if n.startswith(("img_", "num_convs", "conv_", "use_maxpool", "head_out"))]
    assert [n for n, _ in student] == [n for n, _ in _abi.LtCnnDesc._fields_]
    assert [ctypes.sizeof(t) for _, t in student] == [ctypes.sizeof(t) for _, t in _abi.LtCnnDesc._fields_]


def test_the_registered_stack_is_served():
    lib = _abi.load()
    d = registered()
    assert lib.lt_cnn_validate(ctypes.byref(d)) == 0, lib.lt_last_error()
    assert lib.lt_cnn_launches(ctypes.byref(d), 1, 0) == lib.lt_cnn_launches(ctypes.byref(d), 50000, 0) > 0   # independent of n
    assert lib.lt_cnn_launches(ctypes.byref(d), 1, 1) == lib.lt_cnn_launches(ctypes.byref(d), 50000, 1) > 0
    size = ctypes.c_size_t()
    weights = 24 * 2 * 16 + 24 * 24 * 9 + 24 * 24 * 4 + 64 * 192
    sizes = []
    for n in (1, 8, 9, 2051, 50000):
        _abi.call("lt_cnn_ws_floats", d, n, ctypes.byref(size))
        sizes.append(size.value)
        tiles = -(-n // 8)
        slabs = -(-tiles // -(-tiles // _abi.CNN_TRAIN_CONSTS["LT_CNN_MAX_SLABS"]))   # equal slabs of whole tiles, none empty
        assert size.value >= weights + slabs * (weights + 24 * 3 + 64)      # packed weights + one partial per workgroup
    assert sizes[-1] == max(sizes) < 8 << 20                                # capped: the scratch does not grow with n


@pytest.mark.parametrize("field, kw", [
    ("conv_padding", dict(conv_padding=[0, 1, 0])),
    ("conv_norm", dict(conv_norm=1)),
    ("conv_activation", dict(conv_activation=C["LT_ACT_ELU"])),
    ("num_convs", dict(num_convs=4)),
    ("conv_stride", dict(conv_stride=[3, 1, 1])),   # a pool of 3
    ("head_out", dict(head_out=10)),
])
def test_validate_names_what_it_refuses(field, kw):
    lib = _abi.load()
    d = registered(**kw)
    assert lib.lt_cnn_validate(ctypes.byref(d)) == C["LT_EINVAL"]
    msg = lib.lt_last_error().decode()
    assert "lt_cnn_desc" in msg and re.search(rf"\b{field}\b", msg), msg
    # every other entry point validates the same way first
    size = ctypes.c_size_t()
    assert lib.lt_cnn_ws_floats(ctypes.byref(d), 8, ctypes.byref(size)) == C["LT_EINVAL"]
    assert lib.lt_cnn_launches(ctypes.byref(d), 8, 0) == C["LT_EINVAL"]
    with pytest.raises(RuntimeError, match=field):
        _abi.call("lt_cnn_forward", d, pointers(_abi.LtCnnParams), X, 8, EMB, WS, None)
    with pytest.raises(RuntimeError, match=field):
        _abi.call("lt_cnn_backward", d, pointers(_abi.LtCnnParams), X, EMB, 8, pointers(_abi.LtCnnGrads, P0 << 1), WS, None)


def einval(name, *args):
    lib = _abi.load()
    conv = [_abi.ptr(a) if t is ctypes.c_void_p else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a
            for a, t in zip(args, _abi.CNN_TRAIN_SIGNATURES[name][1], strict=True)]
    assert getattr(lib, name)(*conv) == C["LT_EINVAL"], (name, args)
    return lib.lt_last_error().decode()


def test_null_pointers_and_n_below_one_are_refused_by_every_entry_point():
    d, p, g, size = registered(), pointers(_abi.LtCnnParams), pointers(_abi.LtCnnGrads, P0 << 1), ctypes.c_size_t()
    assert "desc" in einval("lt_cnn_validate", None)
    assert "desc" in einval("lt_cnn_ws_floats", None, 8, ctypes.byref(size))
    assert "desc" in einval("lt_cnn_launches", None, 8, 0)
    assert "desc" in einval("lt_cnn_forward", None, p, X, 8, EMB, WS, None)
    assert "desc" in einval("lt_cnn_backward", None, p, X, EMB, 8, g, WS, None)
    assert "floats" in einval("lt_cnn_ws_floats", d, 8, None)
    for n in (0, -3):
        assert "n" in einval("lt_cnn_ws_floats", d, n, ctypes.byref(size))
        assert "n" in einval("lt_cnn_launches", d, n, 1)
        assert "lt_cnn_forward" in einval("lt_cnn_forward", d, p, X, n, EMB, WS, None)
        assert "lt_cnn_backward" in einval("lt_cnn_backward", d, p, X, EMB, n, g, WS, None)
    fwd = dict(params=p, x=X, n=8, emb_out=EMB, ws=WS)
    for name in ("params", "x", "emb_out", "ws"):
        a = dict(fwd, **{name: None})
        assert name in einval("lt_cnn_forward", d, a["params"], a["x"], a["n"], a["emb_out"], a["ws"], None)
    bwd = dict(params=p, x=X, d_emb=EMB, n=8, grads_out=g, ws=WS)
    for name in ("params", "x", "d_emb", "grads_out", "ws"):
        a = dict(bwd, **{name: None})
        assert name in einval("lt_cnn_backward", d, a["params"], a["x"], a["d_emb"], a["n"], a["grads_out"], a["ws"], None)
    # a parameter / gradient pointer the descriptor needs
    hole = pointers(_abi.LtCnnParams)
    hole.conv_b[2] = None
    assert "params" in einval("lt_cnn_forward", d, hole, X, 8, EMB, WS, None)
    ghole = pointers(_abi.LtCnnGrads, P0 << 1)
    ghole.head_w = None
    assert "grads_out" in einval("lt_cnn_backward", d, p, X, EMB, 8, ghole, WS, None)
    assert "ws" in einval("lt_cnn_forward", d, p, X, 8, EMB, WS + 4, None)   # not 16-byte aligned


def test_the_switch_refuses_a_cpu_env_and_a_cpu_module(tmp_path):
    import torch

    from locotouch_amd.distill import Distillation, distillation_cfg
    from locotouch_amd.rl.models import CNN2dHead
    from tests.distill_synth import ScriptedEnv, teacher_policy

    head = CNN2dHead((2, 17, 13), (24, 24, 24), (4, 3, 2), (2, 1, 1), None, None, 64, "relu", True)
    x = torch.rand(5, 2, 17, 13)
    before = head(x)
    with pytest.raises(ValueError, match="CUDA"):
        head.enable_fused_training((2, 17, 13))
    assert head._fused_cnn is None and torch.equal(head(x), before)   # refused: the module path, bit for bit
    cfg = distillation_cfg("Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1")
    cfg.logger = None
    with pytest.raises(ValueError, match="CUDA"):
        Distillation(ScriptedEnv(), cfg, teacher_policy=teacher_policy(), log_dir=str(tmp_path), verbose=False, fused_cnn_training=True)
    with pytest.raises(ValueError, match="CUDA"):   # play trains nothing, but the switch never passes quietly
        Distillation(ScriptedEnv(), cfg, training=False, verbose=False, fused_cnn_training=True)
    # an unserved stack is refused with the validator's message before the device matters
    tanh = CNN2dHead((2, 17, 13), (24, 24, 24), (4, 3, 2), (2, 1, 1), None, None, 64, "tanh", True)
    with pytest.raises(ValueError, match="Tanh"):
        tanh.enable_fused_training((2, 17, 13))
    odd = CNN2dHead((2, 17, 13), (24, 24, 24), (4, 3, 2), (2, 1, 1), None, None, 10, "relu", True)
    with pytest.raises(ValueError, match="head_out"):
        odd.enable_fused_training((2, 17, 13))
