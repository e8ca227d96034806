"""The argument validation of lt_gru_forward / lt_gru_backward (include/lt_env.h): the check lt_lstm_* has (tests/test_lstm_abi.py),
shared through csrc/lt_seq_tile.h.  No device is touched: every call below is decided on the host before anything is launched (the
pointers are made-up addresses that are never dereferenced)."""
import ctypes
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
_vp = ctypes.c_void_p
A0 = 1 << 30  # made-up, 16-byte aligned addresses


def addr(k):
    return A0 + (k << 24)


def forward_args(**kw):
    a = dict(ig=addr(1), h0=addr(2), w_hh=addr(3), b_ih=addr(4), b_hh=addr(5), L=4, B=8, H=128, out=addr(6), ws=addr(7), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def backward_args(**kw):
    a = dict(dout=addr(1), dhn=addr(2), out=addr(3), ws=addr(4), h0=addr(5), w_hh=addr(6), L=4, B=8, H=128, dig=addr(7), dhg=addr(8),
             scratch=addr(9), dh0=addr(10), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def status(name, args):
    lib = _abi.load()
    return getattr(lib, name)(*[_abi.ptr(x) if t is _vp else x for x, t in zip(args, _abi.SIGNATURES[name][1], strict=True)])


def refused(name, args, field):
    assert status(name, args) == C["LT_EINVAL"], (name, field)
    msg = _abi.load().lt_last_error().decode()
    assert msg.startswith(name + ":") and re.search(rf"\b{re.escape(field)} must be\b", msg), msg
    with pytest.raises(RuntimeError, match=name):
        _abi.call(name, *args)


SIZES = [("H", dict(H=96)), ("H", dict(H=0)), ("H", dict(H=32)), ("L", dict(L=0)), ("L", dict(L=-1)), ("B", dict(B=0)), ("B", dict(B=-3)),
         ("B", dict(B=16 * 65535 + 1))]


def test_signatures_are_the_headers():
    """(ig, h0, w_hh, b_ih, b_hh, L, B, H, out, ws, stream) and (dout, dhn, out, ws, h0, w_hh, L, B, H, dig, dhg, scratch, dh0, stream)"""
    _int = ctypes.c_int
    assert _abi.SIGNATURES["lt_gru_forward"] == (_int, [_vp] * 5 + [_int] * 3 + [_vp] * 3)
    assert _abi.SIGNATURES["lt_gru_backward"] == (_int, [_vp] * 6 + [_int] * 3 + [_vp] * 5)
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67


@pytest.mark.parametrize("field, kw", SIZES + [(k, {k: None}) for k in ("ig", "h0", "w_hh", "b_ih", "b_hh", "out", "ws")]
                         + [("ig", dict(ig=addr(1) + 4))], ids=str)
def test_forward_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_gru_forward", forward_args(**kw), field)
    if field == "H":
        assert "multiple of 64" in _abi.load().lt_last_error().decode()


@pytest.mark.parametrize("field, kw", SIZES + [(k, {k: None}) for k in ("dout", "out", "ws", "h0", "w_hh", "dig", "dhg", "scratch", "dh0")]
                         + [("dhn", dict(dhn=addr(2) + 4))], ids=str)
def test_backward_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_gru_backward", backward_args(**kw), field)
    if field == "H":
        assert "multiple of 64" in _abi.load().lt_last_error().decode()


def test_backward_accepts_a_null_dhn_at_the_validation_stage():
    """The pointers are validated before the sizes and the refusal names the first fault.  A call whose only other fault is H = 96 is
    refused for H with dhn NULL: the NULL passed the pointer stage (a NULL `dout` in the same call is named instead).  A fully valid
    call would launch, so it belongs to the GPU tests: tests/test_rl_gru.py compares NULL with zeros on the device."""
    refused("lt_gru_backward", backward_args(H=96, dhn=None), "H")
    refused("lt_gru_backward", backward_args(H=96, dhn=None, dout=None), "dout")
