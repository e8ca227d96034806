"""include/lt_student.h: part of the lt_env.h ABI, bound by locotouch_amd/_abi.py from the header itself; the host-only validator and
size queries; `FusedStudent.for_student` refuses what the kernels do not serve.  No device is touched."""
import ctypes
import os
import re

import pytest
import torch

from locotouch_amd import _abi
from locotouch_amd.distill import Student, distillation_cfg
from tests import distill_synth as S
from tests import student_ref as R

TASK = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"
C = _abi.CONSTS


def registered_desc():
    return R.desc_of(R.CASES["reg"])


def test_header_is_part_of_the_abi_and_bound_from_itself():
    env_h = open(_abi.HEADER).read()
    assert re.search(r'^#include "lt_student\.h"$', env_h, flags=re.M) and os.path.samefile(_abi.STUDENT_HEADER, os.path.join(_abi.REPO, "include", "lt_student.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.STUDENT_HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_student_\w+)\s*\(", src))
    assert protos == set(_abi.STUDENT_SIGNATURES) and len(protos) == 6
    assert _abi.STUDENT_VALUE_QUERIES == {"lt_student_step_launches"}
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67 and len(_abi.OBS_NORM_SIGNATURES) == 3
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name in _abi.STUDENT_SIGNATURES:
        assert getattr(lib, name) is not None
        if name in _abi.STUDENT_VALUE_QUERIES:
            with pytest.raises(TypeError):
                _abi.call(name)
        else:
            assert name in _abi._calls


def test_size_queries_agree_with_the_documented_layout():
    d = registered_desc()
    lib = _abi.load()
    assert lib.lt_student_validate(ctypes.byref(d)) == 0
    pad16, pad4 = (lambda v: (v + 15) // 16 * 16), (lambda v: (v + 3) // 4 * 4)
    want = 0
    cin = 2
    for c, k in zip((24, 24, 24), (4, 3, 2)):
        want += pad4(cin * k * k * c) + pad4(c)
        cin = c
    want += pad4(192 * 64) + 64                       # head: maps 14x10 -> pool 7x5 -> 5x3 -> 4x2, 24 * 8 = 192
    want += 3 * 512 * (64 + 512) + 2 * 3 * 512        # [W_ih | W_hh], b_ih, b_hh
    for dims in ((512, 256, 128, 64, 64), (336, 512, 256, 128, 12)):  # the backbone's input row is padded to 336
        for a, b in zip(dims[:-1], dims[1:]):
            want += pad16(b) * pad16(a) + pad16(b)
    size = ctypes.c_size_t()
    _abi.call("lt_student_packed_floats", d, ctypes.byref(size))
    assert size.value == want
    for n in (1, 37, 405, 4112):
        _abi.call("lt_student_ws_floats", d, n, ctypes.byref(size))
        assert size.value == n * (64 + 512)
        assert 1 <= lib.lt_student_step_launches(ctypes.byref(d), n) <= 4
    with pytest.raises(RuntimeError, match="lt_student_ws_floats"):
        _abi.call("lt_student_ws_floats", d, 0, ctypes.byref(size))


@pytest.mark.parametrize("name", list(R.CASES))
def test_size_queries_agree_with_the_documented_layout_over_the_family(name):
    case = R.CASES[name]
    d = R.desc_of(case)
    lib = _abi.load()
    assert lib.lt_student_validate(ctypes.byref(d)) == 0, lib.lt_last_error().decode()
    pad16, pad4 = R.pad16, R.pad4
    maps = R.geometry(case)
    D, H, P = case["D"], case["H"], case["P"]
    want = 0
    for (cin, _, _), (c, k, _) in zip(maps, case["convs"]):
        want += pad4(cin * k * k * c) + pad4(c)                  # transposed weight [Cin K K][Cout], bias
    flat = maps[-1][0] * maps[-1][1] * maps[-1][2]
    want += pad4(flat * D) + D                                   # head [flat][D], bias
    want += 3 * H * (D + H) + 2 * 3 * H                          # [W_ih | W_hh], b_ih, b_hh
    cat_pad = pad16(P + pad16(case["enc"][-1]))                  # the backbone's input row: proprioception | padded embedding
    assert case["bb"][0] == P + case["enc"][-1] and cat_pad == R.cat_pad(case)
    for dims in (case["enc"], (cat_pad,) + tuple(case["bb"][1:])):
        for a, b in zip(dims[:-1], dims[1:]):
            want += pad16(b) * pad16(a) + pad16(b)
    if name == "wide":
        assert cat_pad == 528 and flat == 1444
    if name == "reg":
        assert cat_pad == 336 and flat == 192
    blocks, total = R.packed_blocks(case)
    assert total == want and all(off % 4 == 0 for _, off, _, _ in blocks)
    size = ctypes.c_size_t()
    _abi.call("lt_student_packed_floats", d, ctypes.byref(size))
    assert size.value == want
    for n in R.NS + (4112,):
        _abi.call("lt_student_ws_floats", d, n, ctypes.byref(size))
        assert size.value == n * (D + H)
        assert 1 <= lib.lt_student_step_launches(ctypes.byref(d), n) <= 4


@pytest.mark.parametrize("field, mutate", [
    ("rnn_type", lambda d: setattr(d, "rnn_type", _abi.LT_STUDENT_RNN_LSTM)),
    ("rnn_layers", lambda d: setattr(d, "rnn_layers", 2)),
    ("conv_norm", lambda d: setattr(d, "conv_norm", 1)),
    ("conv_padding", lambda d: d.conv_padding.__setitem__(1, 1)),
    ("conv_activation", lambda d: setattr(d, "conv_activation", C["LT_ACT_ELU"])),
    ("conv_stride", lambda d: d.conv_stride.__setitem__(0, 3)),
    ("num_convs", lambda d: setattr(d, "num_convs", 4)),
    ("head_out", lambda d: setattr(d, "head_out", 60)),
    ("rnn_hidden", lambda d: setattr(d, "rnn_hidden", 480)),
    ("encoder.dims", lambda d: d.encoder.dims.__setitem__(2, 1024)),
    ("encoder.dims", lambda d: d.encoder.dims.__setitem__(0, 256)),
    ("backbone.num_layers", lambda d: setattr(d.backbone, "num_layers", 7)),
    ("backbone.activation", lambda d: setattr(d.backbone, "activation", C["LT_ACT_TANH"])),
    ("backbone.input_format", lambda d: setattr(d.backbone, "input_format", C["LT_ROWS_BF16"])),
    ("encoder.input_format", lambda d: setattr(d.encoder, "input_format", C["LT_ROWS_BF16"])),
    ("proprio_dim", lambda d: setattr(d, "proprio_dim", -1)),
])
def test_validator_refuses_what_the_kernels_do_not_serve_and_names_the_field(field, mutate):
    d = registered_desc()
    mutate(d)
    lib = _abi.load()
    assert lib.lt_student_validate(ctypes.byref(d)) == C["LT_EINVAL"]
    assert field in lib.lt_last_error().decode()
    size = ctypes.c_size_t()
    with pytest.raises(RuntimeError, match=re.escape(field)):
        _abi.call("lt_student_packed_floats", d, ctypes.byref(size))
    assert lib.lt_student_step_launches(ctypes.byref(d), 405) == C["LT_EINVAL"]


def make_student(tmp, **enc):
    cfg = distillation_cfg(TASK)
    cfg.device, cfg.log_dir = "cpu", str(tmp)
    for k, v in enc.items():
        setattr(cfg.tactile_encoder, k, v)
    torch.manual_seed(0)
    return Student(cfg, S.PROPRIO, S.TACTILE, S.ACTIONS, teacher_policy_inference=S.teacher_policy(), verbose=False)


def test_describe_gives_the_registered_descriptor_and_an_lstm_student_is_refused(tmp_path):
    from locotouch_amd.distill.fused_student import FusedStudent, describe

    d, tensors = describe(make_student(tmp_path))
    assert bytes(d) == bytes(registered_desc())
    assert len(tensors["conv_w"]) == 3 and len(tensors["enc_w"]) == 4 and tensors["gru_w_hh"].shape == (1536, 512)
    with pytest.raises(ValueError, match="rnn_type"):
        FusedStudent.for_student(make_student(tmp_path, rnn_type="lstm"))
    with pytest.raises(ValueError, match="rnn_layers"):
        FusedStudent.for_student(make_student(tmp_path, rnn_num_layers=2))
    with pytest.raises(ValueError, match="CUDA"):  # served architecture, but the parameters are not on the device: no fall-back
        FusedStudent.for_student(make_student(tmp_path))
