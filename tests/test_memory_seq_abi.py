"""include/lt_memory_seq.h: a header of its own, bound by locotouch_amd/_abi.py from the header itself, and the argument validation of its
two entry points.  No device is touched: every call below is decided on the host before anything is launched (the pointers are made-up
addresses that are never dereferenced) - the whole-rollout counterpart of tests/test_memory_abi.py."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
_vp, _int, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
A0 = 1 << 30  # made-up, 16-byte aligned addresses, 16 MiB apart (the largest array below, gates, is 4 * 64 * 4 * 128 * 4 B = 512 KiB)
NET_FIELDS = ("x", "x_stride", "I", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0", "out", "cell", "gates", "h_prev", "c_prev")
GRAD_FIELDS = ("dout", "w_hh", "cell", "gates", "c_prev", "dgates", "dc_carry")
T, E, H = 4, 64, 128


def addr(k):
    return A0 + (k << 24)


def net(base, I=270, **kw):
    a = {f: addr(base + k) for k, f in enumerate(NET_FIELDS)}
    a["I"], a["x_stride"] = I, 100 * I  # a block of a storage of 100 envs
    assert set(kw) <= set(a)
    a.update(kw)
    return _abi.LtMemorySeqNet(**a)


def grad(base, **kw):
    a = {f: addr(base + k) for k, f in enumerate(GRAD_FIELDS)}
    assert set(kw) <= set(a)
    a.update(kw)
    return _abi.LtMemorySeqGrad(**a)


def forward_args(actor=None, critic=None, **kw):
    a = dict(actor=net(1, **(actor or {})), critic=net(20, **{"I": 301, **(critic or {})}), dones=addr(40), dones_stride=100, T=T, E=E, H=H,
             stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def backward_args(actor=None, critic=None, **kw):
    a = dict(actor=grad(1, **(actor or {})), critic=grad(20, **(critic or {})), dones=addr(40), dones_stride=100, T=T, E=E, H=H, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def refused(name, args, field):
    """LT_EINVAL through the raw function and a RuntimeError through `_abi.call`, the text naming the function and the field."""
    _abi.load()
    fn, conv = _abi._calls[name]
    assert fn(*[a if c is None else c(a) for c, a in zip(conv, args, strict=True)]) == C["LT_EINVAL"], (name, field)
    msg = _abi.load().lt_last_error().decode()
    assert msg.startswith(name + ": invalid argument: ") and re.search(rf"(?<![\w.]){re.escape(field)} must be\b", msg), msg
    with pytest.raises(RuntimeError, match=name):
        _abi.call(name, *args)


def test_header_is_bound_from_itself_and_leaves_the_abi_pins_alone():
    assert os.path.samefile(_abi.MEMORY_SEQ_HEADER, os.path.join(_abi.REPO, "include", "lt_memory_seq.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.MEMORY_SEQ_HEADER).read(), flags=re.S))
    assert set(re.findall(r"\b(lt_\w+)\s*\(", src)) == set(_abi.MEMORY_SEQ_SIGNATURES) == {"lt_memory_seq_forward", "lt_memory_seq_backward",
                                                                                            "lt_memory_seq_backward_units"}
    assert _abi.MEMORY_SEQ_VALUE_QUERIES == {"lt_memory_seq_backward_units"}
    assert _abi.MEMORY_SEQ_SIGNATURES["lt_memory_seq_backward_units"] == (_int, [_int, _int])
    net_p, grad_p = ctypes.POINTER(_abi.LtMemorySeqNet), ctypes.POINTER(_abi.LtMemorySeqGrad)
    # (actor, critic, dones, dones_stride, T, E, H, stream), both
    assert _abi.MEMORY_SEQ_SIGNATURES["lt_memory_seq_forward"] == (_int, [net_p, net_p, _vp, _i64, _int, _int, _int, _vp])
    assert _abi.MEMORY_SEQ_SIGNATURES["lt_memory_seq_backward"] == (_int, [grad_p, grad_p, _vp, _i64, _int, _int, _int, _vp])
    assert [(n, t) for n, t in _abi.LtMemorySeqNet._fields_] == [(f, _i64 if f == "x_stride" else _int if f == "I" else _vp) for f in NET_FIELDS]
    assert [(n, t) for n, t in _abi.LtMemorySeqGrad._fields_] == [(f, _vp) for f in GRAD_FIELDS]
    others = (set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES) | set(_abi.COLLECT_SIGNATURES)
              | set(_abi.LEDGER_SIGNATURES) | set(_abi.CNN_TRAIN_SIGNATURES) | set(_abi.BC_SIGNATURES) | set(_abi.LSTM_SIGNATURES)
              | set(_abi.MEMORY_SIGNATURES))
    assert not set(_abi.MEMORY_SEQ_SIGNATURES) & others
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67  # lt_env.h's own prototypes and the version are unchanged
    assert set(_abi.MEMORY_SIGNATURES) == {"lt_memory_step", "lt_memory_finish"} and set(_abi.LSTM_SIGNATURES) == {"lt_lstm_forward", "lt_lstm_backward"}
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name, (restype, argtypes) in _abi.MEMORY_SEQ_SIGNATURES.items():
        fn = getattr(lib, name)  # exported ...
        assert list(fn.argtypes) == argtypes and fn.restype is restype
        assert (name in _abi._calls) != (name in _abi.MEMORY_SEQ_VALUE_QUERIES)  # ... and launched through `_abi.call`, or a value query


SIZE_REFUSALS = [("H", dict(H=96)), ("H", dict(H=576)), ("H", dict(H=0)), ("E", dict(E=0)), ("E", dict(E=16 * 65535 + 1)), ("T", dict(T=0)),
                 ("T", dict(T=-1)), ("dones_stride", dict(dones_stride=E - 1))]
FORWARD_REFUSALS = SIZE_REFUSALS + [
    ("actor.I", dict(actor=dict(I=0))), ("critic.I", dict(critic=dict(I=1249 - H))), ("actor.x_stride", dict(actor=dict(x_stride=E * 270 - 1))),
    ("actor.x", dict(actor=dict(x=None))), ("actor.x", dict(actor=dict(x=addr(1) + 2))), ("critic.w_ih", dict(critic=dict(w_ih=None)))
] + [(f"{who}.{f}", {who: {f: bad}}) for who, base in (("actor", 1), ("critic", 20))
     for f in NET_FIELDS[4:] for bad in (None, addr(base + NET_FIELDS.index(f)) + 4)]


@pytest.mark.parametrize("field, kw", FORWARD_REFUSALS, ids=str)
def test_forward_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_memory_seq_forward", forward_args(**kw), field)


def test_forward_accepts_the_largest_panel_and_refuses_one_float_more():
    """I + H = 1248 passes the validation stage (a call whose only other fault is T = 0 is refused for T); 1249 is refused for I."""
    refused("lt_memory_seq_forward", forward_args(actor=dict(I=1248 - H), T=0), "T")
    refused("lt_memory_seq_forward", forward_args(actor=dict(I=1249 - H), T=0), "T")  # (the sizes come first)
    refused("lt_memory_seq_forward", forward_args(actor=dict(I=1249 - H)), "actor.I")


@pytest.mark.parametrize("who, out, state", [("actor", "out", "h0"), ("actor", "cell", "c0"), ("critic", "h_prev", "h0"), ("critic", "gates", "c0")])
def test_forward_refuses_an_output_that_overlaps_an_initial_state(who, out, state):
    """Other workgroups of the first launch still read h0 / c0.  Overlap, not equality: h0 in the MIDDLE of the output, and the other
    network's state as well."""
    base = 1 if who == "actor" else 20
    h0 = addr(base + NET_FIELDS.index(out)) + 4 * (E * H + 64)  # inside step 1 of the output array
    refused("lt_memory_seq_forward", forward_args(**{who: {state: h0}}), f"{who}.{out}")
    other = "critic" if who == "actor" else "actor"
    refused("lt_memory_seq_forward", forward_args(**{other: {state: h0}}), f"{who}.{out}")


BACKWARD_REFUSALS = SIZE_REFUSALS + [(f"{who}.{f}", {who: {f: bad}}) for who, base in (("actor", 1), ("critic", 20))
                                     for f in GRAD_FIELDS for bad in (None, addr(base + GRAD_FIELDS.index(f)) + 8)]


@pytest.mark.parametrize("field, kw", BACKWARD_REFUSALS, ids=str)
def test_backward_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_memory_seq_backward", backward_args(**kw), field)


def test_null_networks_are_refused_and_null_dones_pass_the_validation_stage():
    for name, make in (("lt_memory_seq_forward", forward_args), ("lt_memory_seq_backward", backward_args)):
        args = make()
        args[1] = None
        refused(name, args, "critic")
        refused(name, make(dones=None, dones_stride=0, H=96), "H")  # dones may be NULL (no reset anywhere): refused for H alone


def test_backward_units_is_a_value_query_over_the_supported_sizes():
    """64, 32 or 16 output units per workgroup (the backward kernel's variant), 0 where lt_memory_seq_backward would refuse E or H; never
    a panel that does not fit the 160 KiB of LDS: [units][4H + 8] floats."""
    lib = _abi.load()
    with pytest.raises(TypeError, match="returns a value"):
        _abi.call("lt_memory_seq_backward_units", 64, 128)
    for e, h in ((0, 128), (16 * 65535 + 1, 128), (64, 96), (64, 576), (64, 0)):
        assert lib.lt_memory_seq_backward_units(e, h) == 0, (e, h)
    for h in range(64, 513, 64):
        for e in (1, 17, 1024, 4096, 16 * 65535):
            u = lib.lt_memory_seq_backward_units(e, h)
            assert u in (16, 32, 64) and u * (4 * h + 8) * 4 <= 160 * 1024 and h % u == 0, (e, h, u)
