"""include/lt_memory.h: part of the lt_env.h ABI, bound by locotouch_amd/_abi.py from the header itself, and the argument validation of
its two entry points.  No device is touched: every call below is decided on the host before anything is launched (the pointers are
made-up addresses that are never dereferenced) - the rollout-step counterpart of tests/test_lstm_abi.py."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
_vp, _int = ctypes.c_void_p, ctypes.c_int
A0 = 1 << 30  # made-up, 16-byte aligned addresses
NET_FIELDS = ("x", "I", "w_ih", "w_hh", "b_ih", "b_hh", "h_in", "c_in", "h_out", "c_out", "saved_h", "saved_c")


def addr(k):
    return A0 + (k << 24)


def net(base, **kw):
    a = {f: addr(base + k) for k, f in enumerate(NET_FIELDS)}
    a["I"] = 270
    assert set(kw) <= set(a)
    a.update(kw)
    return _abi.LtMemoryNet(**a)


def step_args(actor=None, critic=None, **kw):
    a = dict(actor=net(1, **(actor or {})), critic=net(20, **{'I': 301, **(critic or {})}), dones=addr(40), N=64, H=128, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def finish_args(**kw):
    a = dict(h_a=addr(1), c_a=addr(2), h_c=addr(3), c_c=addr(4), dones=addr(5), N=64, H=128, out_h_a=addr(6), out_c_a=addr(7),
             out_h_c=addr(8), out_c_c=addr(9), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def refused(name, args, field):
    """LT_EINVAL through the raw function and a RuntimeError through `_abi.call`, the text naming the function and the field."""
    _abi.load()
    fn, conv = _abi._calls[name]
    assert fn(*[a if c is None else c(a) for c, a in zip(conv, args, strict=True)]) == C["LT_EINVAL"], (name, field)
    msg = _abi.load().lt_last_error().decode()
    assert msg.startswith(name + ":") and re.search(rf"(?<![\w.]){re.escape(field)} must be\b", msg), msg
    with pytest.raises(RuntimeError, match=name):
        _abi.call(name, *args)


def test_header_is_part_of_the_abi_and_bound_from_itself():
    env_h = open(_abi.HEADER).read()
    assert re.search(r'^#include "lt_memory\.h"$', env_h, flags=re.M)
    assert os.path.samefile(_abi.MEMORY_HEADER, os.path.join(_abi.REPO, "include", "lt_memory.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.MEMORY_HEADER).read(), flags=re.S))
    assert set(re.findall(r"\b(lt_\w+)\s*\(", src)) == set(_abi.MEMORY_SIGNATURES) == {"lt_memory_step", "lt_memory_finish"}
    net_p = ctypes.POINTER(_abi.LtMemoryNet)
    # (actor, critic, dones, N, H, stream) and (h_a, c_a, h_c, c_c, dones, N, H, out_h_a, out_c_a, out_h_c, out_c_c, stream)
    assert _abi.MEMORY_SIGNATURES["lt_memory_step"] == (_int, [net_p, net_p, _vp, _int, _int, _vp])
    assert _abi.MEMORY_SIGNATURES["lt_memory_finish"] == (_int, [_vp] * 5 + [_int] * 2 + [_vp] * 5)
    assert [(n, t) for n, t in _abi.LtMemoryNet._fields_] == [(f, _int if f == "I" else _vp) for f in NET_FIELDS]
    others = (set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES) | set(_abi.COLLECT_SIGNATURES)
              | set(_abi.LEDGER_SIGNATURES) | set(_abi.CNN_TRAIN_SIGNATURES) | set(_abi.BC_SIGNATURES) | set(_abi.LSTM_SIGNATURES))
    assert not set(_abi.MEMORY_SIGNATURES) & others
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67  # lt_env.h's own prototypes and the version are unchanged
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name, (restype, argtypes) in _abi.MEMORY_SIGNATURES.items():
        fn = getattr(lib, name)  # exported ...
        assert list(fn.argtypes) == argtypes and fn.restype is restype and name in _abi._calls  # ... and launched through `_abi.call`


STEP_REFUSALS = [("H", dict(H=96)), ("H", dict(H=576)), ("H", dict(H=0)), ("N", dict(N=0)), ("N", dict(N=-4)),
                 ("actor.I", dict(actor=dict(I=0))), ("critic.I", dict(critic=dict(I=0))), ("critic.I", dict(critic=dict(I=1200))),
                 ("actor.w_ih", dict(actor=dict(w_ih=None))), ("critic.w_hh", dict(critic=dict(w_hh=None))),
                 ("actor.b_ih", dict(actor=dict(b_ih=None))), ("critic.b_hh", dict(critic=dict(b_hh=None))),
                 ("actor.saved_h", dict(actor=dict(saved_h=None))), ("critic.saved_c", dict(critic=dict(saved_c=None))),
                 ("actor.x", dict(actor=dict(x=None))), ("actor.h_in", dict(actor=dict(h_in=None))),
                 ("critic.c_out", dict(critic=dict(c_out=None))), ("critic.w_hh", dict(critic=dict(w_hh=addr(23) + 4))),
                 ("actor.x", dict(actor=dict(x=addr(1) + 2)))]


@pytest.mark.parametrize("field, kw", STEP_REFUSALS, ids=str)
def test_step_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_memory_step", step_args(**kw), field)


def test_step_refuses_a_state_written_over_itself():
    """h_out == h_in would let one workgroup read what another has already written in the same launch."""
    refused("lt_memory_step", step_args(actor=dict(h_out=addr(1 + NET_FIELDS.index("h_in")))), "actor.h_out / .c_out")


def test_step_refuses_a_null_network():
    args = step_args()
    args[1] = None
    refused("lt_memory_step", args, "critic")


@pytest.mark.parametrize("field, kw", [("H", dict(H=96)), ("H", dict(H=576)), ("N", dict(N=0))]
                         + [(k, {k: None}) for k in ("h_a", "c_a", "h_c", "c_c", "out_h_a", "out_c_a", "out_h_c", "out_c_c")]
                         + [("out_c_c", dict(out_c_c=addr(9) + 8))], ids=str)
def test_finish_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_memory_finish", finish_args(**kw), field)


def test_null_dones_pass_the_validation_stage():
    """dones may be NULL (t = 0 of a rollout; a plain copy in the finish): a call whose only other fault is H = 96 is refused for H."""
    refused("lt_memory_step", step_args(dones=None, H=96), "H")
    refused("lt_memory_finish", finish_args(dones=None, H=96), "H")
