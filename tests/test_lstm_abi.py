"""include/lt_lstm.h: part of the lt_env.h ABI, bound by locotouch_amd/_abi.py from the header itself, and the argument validation of
its two entry points.  No device is touched: every call below is decided on the host before anything is launched (the pointers are
made-up addresses that are never dereferenced) - the LSTM counterpart of the GRU lines of tests/test_abi.py."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
_vp, _int = ctypes.c_void_p, ctypes.c_int
A0 = 1 << 30  # made-up, 16-byte aligned addresses


def addr(k):
    return A0 + (k << 24)


def forward_args(**kw):
    a = dict(ig=addr(1), h0=addr(2), c0=addr(3), w_hh=addr(4), b_ih=addr(5), b_hh=addr(6), L=4, B=8, H=128, out=addr(7), cell=addr(8),
             ws=addr(9), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def backward_args(**kw):
    a = dict(dout=addr(1), dhn=addr(2), dcn=addr(3), out=addr(4), cell=addr(5), ws=addr(6), h0=addr(7), c0=addr(8), w_hh=addr(9), L=4, B=8,
             H=128, dgates=addr(10), scratch=addr(11), dh0=addr(12), dc0=addr(13), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def status(name, args):
    lib = _abi.load()
    return getattr(lib, name)(*[_abi.ptr(x) if t is _vp else x for x, t in zip(args, _abi.LSTM_SIGNATURES[name][1], strict=True)])


def refused(name, args, field):
    assert status(name, args) == C["LT_EINVAL"], (name, field)
    msg = _abi.load().lt_last_error().decode()
    assert msg.startswith(name + ":") and re.search(rf"\b{re.escape(field)} must be\b", msg), msg
    with pytest.raises(RuntimeError, match=name):
        _abi.call(name, *args)


SIZES = [("H", dict(H=96)), ("H", dict(H=0)), ("H", dict(H=32)), ("L", dict(L=0)), ("L", dict(L=-1)), ("B", dict(B=0)), ("B", dict(B=-3))]


def test_header_is_part_of_the_abi_and_bound_from_itself():
    env_h = open(_abi.HEADER).read()
    assert re.search(r'^#include "lt_lstm\.h"$', env_h, flags=re.M) and os.path.samefile(_abi.LSTM_HEADER, os.path.join(_abi.REPO, "include", "lt_lstm.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.LSTM_HEADER).read(), flags=re.S))
    assert set(re.findall(r"\b(lt_\w+)\s*\(", src)) == set(_abi.LSTM_SIGNATURES) == {"lt_lstm_forward", "lt_lstm_backward"}
    # the signatures as literals: (ig, h0, c0, w_hh, b_ih, b_hh, L, B, H, out, cell, ws, stream) and
    # (dout, dhn, dcn, out, cell, ws, h0, c0, w_hh, L, B, H, dgates, scratch, dh0, dc0, stream)
    assert _abi.LSTM_SIGNATURES["lt_lstm_forward"] == (_int, [_vp] * 6 + [_int] * 3 + [_vp] * 4)
    assert _abi.LSTM_SIGNATURES["lt_lstm_backward"] == (_int, [_vp] * 9 + [_int] * 3 + [_vp] * 5)
    others = (set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES) | set(_abi.COLLECT_SIGNATURES)
              | set(_abi.LEDGER_SIGNATURES) | set(_abi.CNN_TRAIN_SIGNATURES) | set(_abi.BC_SIGNATURES))
    assert not set(_abi.LSTM_SIGNATURES) & others
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67  # lt_env.h's own prototypes and the version are unchanged
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name, (restype, argtypes) in _abi.LSTM_SIGNATURES.items():
        fn = getattr(lib, name)  # exported ...
        assert list(fn.argtypes) == argtypes and fn.restype is restype and name in _abi._calls  # ... and launched through `_abi.call`


@pytest.mark.parametrize("field, kw", SIZES + [(k, {k: None}) for k in ("ig", "h0", "c0", "w_hh", "b_ih", "b_hh", "out", "cell", "ws")]
                         + [("ig", dict(ig=addr(1) + 4))], ids=str)
def test_forward_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_lstm_forward", forward_args(**kw), field)


@pytest.mark.parametrize("field, kw", SIZES + [(k, {k: None}) for k in ("dout", "out", "cell", "ws", "h0", "c0", "w_hh", "dgates", "scratch", "dh0", "dc0")]
                         + [("dhn", dict(dhn=addr(2) + 8)), ("dcn", dict(dcn=addr(3) + 4))], ids=str)
def test_backward_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_lstm_backward", backward_args(**kw), field)


@pytest.mark.parametrize("kw", [dict(dhn=None), dict(dcn=None), dict(dhn=None, dcn=None)], ids=str)
def test_backward_accepts_null_dhn_and_dcn_at_the_validation_stage(kw):
    """The pointers are validated before the sizes and the refusal names the first fault.  A call whose only other fault is H = 96 is
    refused for H with dhn / dcn NULL: the NULLs passed the pointer stage (a NULL `dout` in the same call is named instead).  A fully
    valid call would launch, so it belongs to the GPU tests: tests/test_rl_lstm.py runs both NULL forms."""
    refused("lt_lstm_backward", backward_args(H=96, **kw), "H")
    refused("lt_lstm_backward", backward_args(H=96, dout=None, **kw), "dout")
