"""include/lt_collect.h: part of the lt_env.h ABI, bound by locotouch_amd/_abi.py from the header itself; the host-only size query and
argument validation; `DeviceTactileRecorder` refuses a device without the kernels.  No device is touched: every call below is refused
on the host before anything is launched (the pointers are made-up addresses that are never dereferenced)."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
NAMES = {"lt_delay_state_bytes", "lt_delay_reset", "lt_delay_push", "lt_delay_read", "lt_collect_after_step"}
STATE, ROWS, OUT, SRC, DST = 1 << 20, 1 << 30, 1 << 32, 1 << 34, 1 << 36  # far apart: no spans overlap at the sizes used here


def test_header_is_part_of_the_abi_and_bound_from_itself():
    env_h = open(_abi.HEADER).read()
    assert re.search(r'^#include "lt_collect\.h"$', env_h, flags=re.M) and os.path.samefile(_abi.COLLECT_HEADER, os.path.join(_abi.REPO, "include", "lt_collect.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.COLLECT_HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_\w+)\s*\(", src))
    assert protos == set(_abi.COLLECT_SIGNATURES) == NAMES
    assert all(res is ctypes.c_int for res, _ in _abi.COLLECT_SIGNATURES.values())
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67 and len(_abi.OBS_NORM_SIGNATURES) == 3 and len(_abi.STUDENT_SIGNATURES) == 6
    assert not set(_abi.COLLECT_SIGNATURES) & (set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES))
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name in NAMES:
        assert getattr(lib, name) is not None and name in _abi._calls  # exported, and launched through `_abi.call`


@pytest.mark.parametrize("n, d, depth", [(1, 1, 1), (37, 442, 7), (4112, 442, 7)])
def test_state_bytes_is_the_documented_layout(n, d, depth):
    size = ctypes.c_size_t()
    _abi.call("lt_delay_state_bytes", n, d, depth, ctypes.byref(size))
    assert size.value >= 4 * n * depth * d + 12 * n
    assert size.value == (4 * n * depth * d + 15) // 16 * 16 + 12 * n  # the padding lt_collect.h documents: the ring rounded up to 16 bytes
    assert size.value % 4 == 0


def push_args(**kw):
    a = dict(state=STATE, n=37, d=442, depth=7, rows=ROWS, rows_stride=442, out0=OUT, out0_stride=442, out1=None, out1_stride=0,
             copy_src=None, copy_src_stride=0, copy_dst=None, copy_dst_stride=0, copy_d=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def refused(name, args, field):
    lib = _abi.load()
    rc = getattr(lib, name)(*[_abi.ptr(x) if t is ctypes.c_void_p else x for x, t in zip(args, _abi.COLLECT_SIGNATURES[name][1])])
    assert rc == C["LT_EINVAL"], (name, field, rc)
    msg = lib.lt_last_error().decode()
    assert name in msg and re.search(rf"\b{re.escape(field)}\b", msg), msg
    with pytest.raises(RuntimeError, match=re.escape(field)):
        _abi.call(name, *args)


@pytest.mark.parametrize("field", ["n", "d", "depth"])
def test_zero_sizes_are_refused_by_every_entry_point(field):
    size = ctypes.c_size_t()
    shape = dict(n=37, d=442, depth=7)
    shape[field] = 0
    refused("lt_delay_state_bytes", [shape["n"], shape["d"], shape["depth"], ctypes.byref(size)], field)
    refused("lt_delay_push", push_args(**shape), field)
    refused("lt_delay_read", [STATE, shape["n"], shape["d"], shape["depth"], OUT, 442, None], field)
    refused("lt_delay_reset", [STATE, shape["n"], shape["d"], shape["depth"], None, SRC, None], field)
    refused("lt_collect_after_step", [STATE, shape["n"], shape["d"], shape["depth"], ROWS, SRC, DST, OUT, OUT + (1 << 20), None], field)


@pytest.mark.parametrize("field, kw", [
    ("out0", dict(out0=None)),
    ("out0", dict(out0=ROWS)),                                            # out0 == rows
    ("out0", dict(out0=ROWS + 4 * 442 * 36)),                             # ... or its last row alone
    ("out0", dict(out0=STATE + 4 * 37 * 442 * 7)),                        # inside the state: the three int columns behind the ring
    ("out1", dict(out1=ROWS - 4 * 441, out1_stride=442)),                 # one float of overlap with the first input row
    ("out1", dict(out1=STATE, out1_stride=442)),
    ("copy_dst", dict(copy_src=SRC, copy_src_stride=348, copy_d=348)),    # copy_src without copy_dst
    ("copy_src", dict(copy_dst=DST, copy_dst_stride=348, copy_d=348)),    # and the reverse
    ("copy_d", dict(copy_src=SRC, copy_src_stride=348, copy_dst=DST, copy_dst_stride=348, copy_d=0)),
    ("copy_dst", dict(copy_src=SRC, copy_src_stride=348, copy_dst=ROWS, copy_dst_stride=348, copy_d=348)),
    ("copy_dst", dict(copy_src=SRC, copy_src_stride=348, copy_dst=SRC, copy_dst_stride=348, copy_d=348)),
    ("rows", dict(rows=None)),
    ("state", dict(state=None)),
])
def test_push_refuses_null_and_aliasing_operands_and_names_them(field, kw):
    refused("lt_delay_push", push_args(**kw), field)


def test_the_other_entry_points_name_what_they_refuse():
    refused("lt_delay_read", [STATE, 37, 442, 7, None, 442, None], "out0")
    refused("lt_delay_read", [STATE, 37, 442, 7, STATE + 16, 442, None], "out0")
    refused("lt_delay_reset", [None, 37, 442, 7, None, SRC, None], "state")
    refused("lt_delay_reset", [STATE, 37, 442, 7, None, None, None], "fresh_delays")
    after = dict(state=STATE, n=37, d=442, depth=7, reward=ROWS, dones=SRC, fresh=DST, reward_out=OUT, done_out=OUT + (1 << 20), stream=None)
    for field, name in (("reward", "reward"), ("dones", "dones"), ("fresh", "fresh_delays"), ("reward_out", "reward_out"), ("done_out", "done_mask_out")):
        refused("lt_collect_after_step", list({**after, field: None}.values()), name)
    refused("lt_collect_after_step", list({**after, "n": 0, "state": None}.values()), "n")


def test_device_recorder_refuses_a_device_without_the_kernels():
    from locotouch_amd.distill import DeviceTactileRecorder

    with pytest.raises(ValueError, match="CUDA"):
        DeviceTactileRecorder("cpu", 37, 442, 3, 7)
