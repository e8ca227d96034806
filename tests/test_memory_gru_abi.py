"""include/lt_memory_gru.h: a header of its own, bound by locotouch_amd/_abi.py from the header itself, and the argument validation of
its four launching entry points and its value query.  No device is touched: every call below is decided on the host before anything is
launched (the pointers are made-up addresses that are never dereferenced) - the GRU counterpart of tests/test_memory_abi.py and
tests/test_memory_seq_abi.py."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
_vp, _int, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
A0 = 1 << 30  # made-up, 16-byte aligned addresses, 16 MiB apart (the largest array below, gates, is 4 * 64 * 4 * 128 * 4 B = 512 KiB)
STEP_FIELDS = ("x", "I", "w_ih", "w_hh", "b_ih", "b_hh", "h_in", "h_out", "saved_h")
NET_FIELDS = ("x", "x_stride", "I", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "out", "gates", "h_prev")
GRAD_FIELDS = ("dout", "w_hh", "gates", "h_prev", "dig", "dhg", "dh_carry")
T, E, H = 4, 64, 128
NAMES = {"lt_memory_gru_step", "lt_memory_gru_finish", "lt_memory_gru_seq_forward", "lt_memory_gru_seq_backward",
         "lt_memory_gru_seq_backward_units"}


def addr(k):
    return A0 + (k << 24)


def make(struct, fields, base, **kw):
    a = {f: addr(base + k) for k, f in enumerate(fields)}
    if "I" in a:
        a["I"] = 270
    if "x_stride" in a:
        a["x_stride"] = 100 * kw.get("I", 270)  # a block of a storage of 100 envs
    assert set(kw) <= set(a)
    a.update(kw)
    return struct(**a)


def step_args(actor=None, critic=None, **kw):
    a = dict(actor=make(_abi.LtMemoryGruNet, STEP_FIELDS, 1, **(actor or {})),
             critic=make(_abi.LtMemoryGruNet, STEP_FIELDS, 20, **{"I": 301, **(critic or {})}), dones=addr(40), N=E, H=H, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def finish_args(**kw):
    a = dict(h_a=addr(1), h_c=addr(2), dones=addr(40), N=E, H=H, out_h_a=addr(3), out_h_c=addr(4), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def forward_args(actor=None, critic=None, **kw):
    a = dict(actor=make(_abi.LtMemoryGruSeqNet, NET_FIELDS, 1, **(actor or {})),
             critic=make(_abi.LtMemoryGruSeqNet, NET_FIELDS, 20, **{"I": 301, **(critic or {})}), dones=addr(40), dones_stride=100, T=T, E=E,
             H=H, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def backward_args(actor=None, critic=None, **kw):
    a = dict(actor=make(_abi.LtMemoryGruSeqGrad, GRAD_FIELDS, 1, **(actor or {})),
             critic=make(_abi.LtMemoryGruSeqGrad, GRAD_FIELDS, 20, **(critic or {})), dones=addr(40), dones_stride=100, T=T, E=E, H=H,
             stream=None)
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
    assert os.path.samefile(_abi.MEMORY_GRU_HEADER, os.path.join(_abi.REPO, "include", "lt_memory_gru.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.MEMORY_GRU_HEADER).read(), flags=re.S))
    assert set(re.findall(r"\b(lt_\w+)\s*\(", src)) == set(_abi.MEMORY_GRU_SIGNATURES) == NAMES
    assert "lt_memory_gru.h" not in open(_abi.HEADER).read()  # lt_env.h does not include it
    assert _abi.MEMORY_GRU_VALUE_QUERIES == {"lt_memory_gru_seq_backward_units"}
    assert _abi.MEMORY_GRU_SIGNATURES["lt_memory_gru_seq_backward_units"] == (_int, [_int, _int])
    step_p, net_p, grad_p = (ctypes.POINTER(s) for s in (_abi.LtMemoryGruNet, _abi.LtMemoryGruSeqNet, _abi.LtMemoryGruSeqGrad))
    # (actor, critic, dones, N, H, stream)
    assert _abi.MEMORY_GRU_SIGNATURES["lt_memory_gru_step"] == (_int, [step_p, step_p, _vp, _int, _int, _vp])
    # (h_a, h_c, dones, N, H, out_h_a, out_h_c, stream)
    assert _abi.MEMORY_GRU_SIGNATURES["lt_memory_gru_finish"] == (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp])
    # (actor, critic, dones, dones_stride, T, E, H, stream), both
    assert _abi.MEMORY_GRU_SIGNATURES["lt_memory_gru_seq_forward"] == (_int, [net_p, net_p, _vp, _i64, _int, _int, _int, _vp])
    assert _abi.MEMORY_GRU_SIGNATURES["lt_memory_gru_seq_backward"] == (_int, [grad_p, grad_p, _vp, _i64, _int, _int, _int, _vp])
    assert [(n, t) for n, t in _abi.LtMemoryGruNet._fields_] == [(f, _int if f == "I" else _vp) for f in STEP_FIELDS]
    assert [(n, t) for n, t in _abi.LtMemoryGruSeqNet._fields_] == [(f, _i64 if f == "x_stride" else _int if f == "I" else _vp) for f in NET_FIELDS]
    assert [(n, t) for n, t in _abi.LtMemoryGruSeqGrad._fields_] == [(f, _vp) for f in GRAD_FIELDS]
    others = (set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES) | set(_abi.COLLECT_SIGNATURES)
              | set(_abi.LEDGER_SIGNATURES) | set(_abi.CNN_TRAIN_SIGNATURES) | set(_abi.BC_SIGNATURES) | set(_abi.LSTM_SIGNATURES)
              | set(_abi.MEMORY_SIGNATURES) | set(_abi.MEMORY_SEQ_SIGNATURES))
    assert not set(_abi.MEMORY_GRU_SIGNATURES) & others
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67  # lt_env.h's own prototypes and the version are unchanged
    assert set(_abi.MEMORY_SIGNATURES) == {"lt_memory_step", "lt_memory_finish"}
    assert set(_abi.MEMORY_SEQ_SIGNATURES) == {"lt_memory_seq_forward", "lt_memory_seq_backward", "lt_memory_seq_backward_units"}
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name, (restype, argtypes) in _abi.MEMORY_GRU_SIGNATURES.items():
        fn = getattr(lib, name)  # exported ...
        assert list(fn.argtypes) == argtypes and fn.restype is restype
        assert (name in _abi._calls) != (name in _abi.MEMORY_GRU_VALUE_QUERIES)  # ... and launched through `_abi.call`, or a value query


def net_refusals(fields, first_16, rows):
    """H = 96, H = 576, rows = 0 and too many, I + H over the limit, and per network every pointer NULL and misaligned (by 2 bytes where
    4-byte alignment is asked - x, w_ih - and by 4 or 8 where 16-byte alignment is)."""
    out = [("H", {"H": 96}), ("H", {"H": 576}), ("H", {"H": 0}), (rows, {rows: 0}), (rows, {rows: 16 * 65535 + 1}),
           ("actor.I", dict(actor=dict(I=0))), ("critic.I", dict(critic=dict(I=1249 - H))), ("actor.I", dict(actor=dict(I=1249 - H)))]
    for who, base in (("actor", 1), ("critic", 20)):
        for f in ("x", "w_ih"):
            out += [(f"{who}.{f}", {who: {f: None}}), (f"{who}.{f}", {who: {f: addr(base + fields.index(f)) + 2}})]
        for f in fields[fields.index(first_16):]:
            out += [(f"{who}.{f}", {who: {f: None}}), (f"{who}.{f}", {who: {f: addr(base + fields.index(f)) + 4}}),
                    (f"{who}.{f}", {who: {f: addr(base + fields.index(f)) + 8}})]
    return out


@pytest.mark.parametrize("field, kw", net_refusals(STEP_FIELDS, "w_hh", "N") + [("actor.h_out", dict(actor=dict(h_out=addr(1 + 6))))], ids=str)
def test_step_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_memory_gru_step", step_args(**kw), field)


@pytest.mark.parametrize("field, kw", [("H", dict(H=96)), ("H", dict(H=576)), ("N", dict(N=0))]
                         + [(f, {f: bad}) for k, f in enumerate(("h_a", "h_c", "out_h_a", "out_h_c"), 1) for bad in (None, addr(k) + 4)], ids=str)
def test_finish_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_memory_gru_finish", finish_args(**kw), field)


SEQ_REFUSALS = [("T", dict(T=0)), ("T", dict(T=-1)), ("dones_stride", dict(dones_stride=E - 1))]


@pytest.mark.parametrize("field, kw", net_refusals(NET_FIELDS, "w_hh", "E") + SEQ_REFUSALS
                         + [("actor.x_stride", dict(actor=dict(x_stride=E * 270 - 1)))], ids=str)
def test_forward_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_memory_gru_seq_forward", forward_args(**kw), field)


def test_the_largest_panel_passes_the_validation_stage_and_one_float_more_does_not():
    """I + H = 1248 passes the validation stage (a call whose only other fault is T = 0 is refused for T); 1249 is refused for I."""
    refused("lt_memory_gru_seq_forward", forward_args(actor=dict(I=1248 - H), T=0), "T")
    refused("lt_memory_gru_seq_forward", forward_args(actor=dict(I=1249 - H)), "actor.I")
    refused("lt_memory_gru_step", step_args(actor=dict(I=1248 - H), critic=dict(w_hh=None)), "critic.w_hh")
    refused("lt_memory_gru_step", step_args(actor=dict(I=1249 - H), critic=dict(w_hh=None)), "actor.I")


@pytest.mark.parametrize("who, out", [("actor", "out"), ("critic", "h_prev"), ("critic", "gates")])
def test_forward_refuses_an_output_that_overlaps_an_initial_state(who, out):
    """Other workgroups of the first launch still read h0.  Overlap, not equality: h0 in the MIDDLE of the output, and the other
    network's state as well."""
    base = 1 if who == "actor" else 20
    h0 = addr(base + NET_FIELDS.index(out)) + 4 * (E * H + 64)  # inside step 1 of the output array
    refused("lt_memory_gru_seq_forward", forward_args(**{who: {"h0": h0}}), f"{who}.{out}")
    other = "critic" if who == "actor" else "actor"
    refused("lt_memory_gru_seq_forward", forward_args(**{other: {"h0": h0}}), f"{who}.{out}")


BACKWARD_REFUSALS = ([("H", dict(H=96)), ("H", dict(H=576)), ("E", dict(E=0)), ("E", dict(E=16 * 65535 + 1))] + SEQ_REFUSALS
                     + [(f"{who}.{f}", {who: {f: bad}}) for who, base in (("actor", 1), ("critic", 20))
                        for f in GRAD_FIELDS for bad in (None, addr(base + GRAD_FIELDS.index(f)) + 8)])


@pytest.mark.parametrize("field, kw", BACKWARD_REFUSALS, ids=str)
def test_backward_names_what_it_refuses_before_touching_a_device(field, kw):
    refused("lt_memory_gru_seq_backward", backward_args(**kw), field)


def test_null_networks_are_refused_and_null_dones_pass_the_validation_stage():
    for name, args_of in (("lt_memory_gru_step", step_args), ("lt_memory_gru_seq_forward", forward_args),
                          ("lt_memory_gru_seq_backward", backward_args)):
        args = args_of()
        args[1] = None
        refused(name, args, "critic")
        args = args_of()
        args[0] = None
        refused(name, args, "actor")
        extra = {} if name == "lt_memory_gru_step" else {"dones_stride": 0}
        refused(name, args_of(dones=None, H=96, **extra), "H")  # dones may be NULL (no reset): refused for H alone
    refused("lt_memory_gru_finish", finish_args(dones=None, H=96), "H")


def test_backward_units_is_a_value_query_over_the_supported_sizes():
    """64, 32 or 16 output units per workgroup (the backward kernel's variant), 0 where lt_memory_gru_seq_backward would refuse E or H;
    never a panel that does not fit the 160 KiB of LDS: [units][3H + 8] floats, so 64 units only up to H = 192 and 32 only up to 384."""
    lib = _abi.load()
    with pytest.raises(TypeError, match="returns a value"):
        _abi.call("lt_memory_gru_seq_backward_units", 64, 128)
    for e, h in ((0, 128), (16 * 65535 + 1, 128), (64, 96), (64, 576), (64, 0)):
        assert lib.lt_memory_gru_seq_backward_units(e, h) == 0, (e, h)
    for h in range(64, 513, 64):
        for e in (1, 17, 1024, 4096, 16 * 65535):
            u = lib.lt_memory_gru_seq_backward_units(e, h)
            assert u in (16, 32, 64) and u * (3 * h + 8) * 4 <= 160 * 1024 and h % u == 0, (e, h, u)
            assert u <= (64 if h <= 192 else 32 if h <= 384 else 16)
