"""include/lt_policy.h: a header of its own, bound by locotouch_amd/_abi.py from the header itself, and the argument validation of
`lt_policy_validate`, `lt_policy_step` and the value query `lt_policy_step_launches`.  No device is touched: every call below is decided
on the host before anything is launched (the pointers are made-up addresses that are never dereferenced), as in
tests/test_memory_gru_abi.py."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
_vp, _int, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
A0 = 1 << 30  # made-up, 16-byte aligned addresses, 16 MiB apart (the largest array below, obs, is 64 * 300 * 4 B)
NAMES = {"lt_policy_validate", "lt_policy_step", "lt_policy_step_launches"}
MEM_FIELDS = ("w_ih", "w_hh", "b_ih", "b_hh", "norm_mean", "norm_std", "norm_eps")
N, I, H = 64, 270, 128
LSTM, GRU = 0, 1


def addr(k):
    return A0 + (k << 24)


def desc(**kw):
    d = _abi.LtPolicyDesc()
    d.rnn_type, d.rnn_layers, d.rnn_hidden, d.obs_dim = kw.pop("rnn_type", LSTM), kw.pop("rnn_layers", 1), kw.pop("rnn_hidden", H), kw.pop("obs_dim", I)
    dims = kw.pop("dims", (d.rnn_hidden, 256, 128, 12))
    d.actor.num_layers = kw.pop("num_layers", len(dims) - 1)
    for k, v in enumerate(dims):
        d.actor.dims[k] = v
    d.actor.activation = C["LT_ACT_ELU"]
    d.actor.input_format = kw.pop("input_format", C["LT_ROWS_F32"])
    assert not kw
    return d


def memory(**kw):
    a = dict(w_ih=addr(1), w_hh=addr(2), b_ih=addr(3), b_hh=addr(4), norm_mean=addr(5), norm_std=addr(6), norm_eps=1e-2)
    assert set(kw) <= set(a)
    a.update(kw)
    return _abi.LtPolicyMemory(**a)


def step_args(rnn_type=LSTM, d=None, mem=None, **kw):
    lstm = rnn_type == LSTM
    a = dict(desc=d or desc(rnn_type=rnn_type), mem=memory(**(mem or {})), actor_packed=addr(7), obs=addr(8), obs_row_stride=300,
             done_mask=addr(9), h_in=addr(10), c_in=addr(11) if lstm else None, h_out=addr(12), c_out=addr(13) if lstm else None, n=N,
             actions_out=addr(14), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def last_error():
    return _abi.load().lt_last_error().decode()


def refused(name, args, field):
    """LT_EINVAL through the raw function and a RuntimeError through `_abi.call`, the text naming the function and the field."""
    _abi.load()
    fn, conv = _abi._calls[name]
    assert fn(*[a if c is None else c(a) for c, a in zip(conv, args, strict=True)]) == C["LT_EINVAL"], (name, field)
    msg = last_error()
    assert msg.startswith(name + ": invalid argument: ") and re.search(rf"(?<![\w.]){re.escape(field)} must be\b", msg), msg
    with pytest.raises(RuntimeError, match=name):
        _abi.call(name, *args)


def test_header_is_bound_from_itself_and_leaves_the_abi_pins_alone():
    assert os.path.samefile(_abi.POLICY_HEADER, os.path.join(_abi.REPO, "include", "lt_policy.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.POLICY_HEADER).read(), flags=re.S))
    assert set(re.findall(r"\b(lt_\w+)\s*\(", src)) == set(_abi.POLICY_SIGNATURES) == NAMES
    assert "lt_policy.h" not in open(_abi.HEADER).read()  # lt_env.h does not include it
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67  # lt_env.h's own prototypes and the version are unchanged
    assert _abi.POLICY_VALUE_QUERIES == {"lt_policy_step_launches"}
    assert _abi.POLICY_CONSTS == {"LT_POLICY_RNN_LSTM": LSTM, "LT_POLICY_RNN_GRU": GRU}
    desc_p, mem_p = ctypes.POINTER(_abi.LtPolicyDesc), ctypes.POINTER(_abi.LtPolicyMemory)
    assert _abi.POLICY_SIGNATURES["lt_policy_validate"] == (_int, [desc_p])
    assert _abi.POLICY_SIGNATURES["lt_policy_step_launches"] == (_int, [desc_p, _i64])
    # (desc, mem, actor_packed, obs, obs_row_stride, done_mask, h_in, c_in, h_out, c_out, n, actions_out, stream)
    assert _abi.POLICY_SIGNATURES["lt_policy_step"] == (_int, [desc_p, mem_p, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp])
    assert [(n, t) for n, t in _abi.LtPolicyDesc._fields_] == [("rnn_type", ctypes.c_int32), ("rnn_layers", ctypes.c_int32),
                                                               ("rnn_hidden", ctypes.c_int32), ("obs_dim", ctypes.c_int32),
                                                               ("actor", _abi.LtMlpDesc)]
    assert [(n, t) for n, t in _abi.LtPolicyMemory._fields_] == [(f, ctypes.c_float if f == "norm_eps" else _vp) for f in MEM_FIELDS]
    others = (set(_abi.SIGNATURES) | set(_abi.OBS_NORM_SIGNATURES) | set(_abi.STUDENT_SIGNATURES) | set(_abi.COLLECT_SIGNATURES)
              | set(_abi.LEDGER_SIGNATURES) | set(_abi.CNN_TRAIN_SIGNATURES) | set(_abi.BC_SIGNATURES) | set(_abi.LSTM_SIGNATURES)
              | set(_abi.MEMORY_SIGNATURES) | set(_abi.MEMORY_SEQ_SIGNATURES) | set(_abi.MEMORY_GRU_SIGNATURES))
    assert not set(_abi.POLICY_SIGNATURES) & others
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name, (restype, argtypes) in _abi.POLICY_SIGNATURES.items():
        fn = getattr(lib, name)  # exported ...
        assert list(fn.argtypes) == argtypes and fn.restype is restype
        assert (name in _abi._calls) != (name in _abi.POLICY_VALUE_QUERIES)  # ... and launched through `_abi.call`, or a value query


DESC_REFUSALS = [("rnn_type", dict(rnn_type=2)), ("rnn_layers", dict(rnn_layers=2)), ("rnn_hidden", dict(rnn_hidden=96)),
                 ("rnn_hidden", dict(rnn_hidden=576)), ("rnn_hidden", dict(rnn_hidden=0)), ("obs_dim", dict(obs_dim=0)),
                 ("obs_dim", dict(obs_dim=1249 - H)), ("actor.dims[0]", dict(dims=(H + 64, 256, 12))),
                 ("actor.input_format", dict(input_format=C["LT_ROWS_BF16"])), ("actor", dict(dims=(H, 513, 12))),
                 ("actor", dict(num_layers=0))]


@pytest.mark.parametrize("field, kw", DESC_REFUSALS, ids=str)
def test_validate_and_step_name_the_descriptor_field_they_refuse(field, kw):
    refused("lt_policy_validate", [desc(**kw)], field)
    refused("lt_policy_step", step_args(d=desc(**kw)), field)
    lib = _abi.load()
    assert lib.lt_policy_step_launches(ctypes.byref(desc(**kw)), N) == C["LT_EINVAL"]  # the value query: a negative code
    assert re.search(rf"(?<![\w.]){re.escape(field)} must be\b", last_error())


def test_the_served_descriptors_pass_and_a_null_one_does_not():
    lib = _abi.load()
    for rnn_type in (LSTM, GRU):
        for h in range(64, 513, 64):
            for i in (1, 270, 1248 - h):
                assert lib.lt_policy_validate(ctypes.byref(desc(rnn_type=rnn_type, rnn_hidden=h, obs_dim=i))) == 0, (rnn_type, h, i)
    refused("lt_policy_validate", [None], "desc")
    refused("lt_policy_step", step_args()[:0] + [None] + step_args()[1:], "desc")


def pointer_refusals():
    """n = 0 and too many rows, a row stride below I, every pointer NULL and misaligned (2 bytes off where 4-byte alignment is asked, 4
    and 8 off where 16-byte alignment is), the cell state of the wrong cell, half a normaliser, overlapping ping-pong buffers."""
    out = [(LSTM, "n", dict(n=0)), (LSTM, "n", dict(n=16 * 65535 + 1)), (GRU, "n", dict(n=-1)), (LSTM, "obs_row_stride", dict(obs_row_stride=I - 1))]
    four = {"obs": 8, "actions_out": 14}
    sixteen = {"actor_packed": 7, "h_in": 10, "h_out": 12}
    for rnn_type in (LSTM, GRU):
        for f, k in four.items():
            out += [(rnn_type, f, {f: None}), (rnn_type, f, {f: addr(k) + 2})]
        for f, k in sixteen.items():
            out += [(rnn_type, f, {f: None}), (rnn_type, f, {f: addr(k) + 4}), (rnn_type, f, {f: addr(k) + 8})]
        out += [(rnn_type, "mem.w_ih", dict(mem=dict(w_ih=None))), (rnn_type, "mem.w_ih", dict(mem=dict(w_ih=addr(1) + 2)))]
        for k, f in enumerate(("w_hh", "b_ih", "b_hh"), 2):
            out += [(rnn_type, f"mem.{f}", dict(mem={f: bad})) for bad in (None, addr(k) + 4, addr(k) + 8)]
        out += [(rnn_type, "mem.norm_mean / mem.norm_std", dict(mem=dict(norm_mean=None))),
                (rnn_type, "mem.norm_mean / mem.norm_std", dict(mem=dict(norm_std=None))),
                (rnn_type, "mem.norm_mean", dict(mem=dict(norm_mean=addr(5) + 2))), (rnn_type, "mem.norm_std", dict(mem=dict(norm_std=addr(6) + 2)))]
        out += [(rnn_type, "mem", dict(mem=None))]
    for f, k in (("c_in", 11), ("c_out", 13)):
        out += [(LSTM, f, {f: None}), (LSTM, f, {f: addr(k) + 4}), (LSTM, f, {f: addr(k) + 8}), (GRU, f, {f: addr(k)})]
    inside = 4 * (17 * H + 4)  # overlap, not equality: an output that starts in the middle of a state that is read
    out += [(LSTM, "h_out", dict(h_out=addr(10))), (GRU, "h_out", dict(h_out=addr(10) + inside)), (LSTM, "h_out", dict(h_out=addr(11) + inside)),
            (LSTM, "c_out", dict(c_out=addr(11))), (LSTM, "c_out", dict(c_out=addr(10) + inside)),
            (GRU, "h_out", dict(h_in=addr(12) + inside))]
    return out


@pytest.mark.parametrize("rnn_type, field, kw", pointer_refusals(), ids=str)
def test_step_names_what_it_refuses_before_touching_a_device(rnn_type, field, kw):
    args = step_args(rnn_type, **{k: v for k, v in kw.items() if k != "mem"}, **({"mem": kw["mem"]} if kw.get("mem") else {}))
    if "mem" in kw and kw["mem"] is None:
        args[1] = None
    refused("lt_policy_step", args, field)


def test_null_mask_and_null_normaliser_pass_the_validation_stage():
    """Both are optional: a call whose only other fault is n = 0 is refused for n.  So does the largest row (I + H = 1248) and a row
    stride of exactly I."""
    for rnn_type in (LSTM, GRU):
        refused("lt_policy_step", step_args(rnn_type, done_mask=None, mem=dict(norm_mean=None, norm_std=None), n=0,
                                            d=desc(rnn_type=rnn_type, obs_dim=1248 - H), obs_row_stride=1248 - H), "n")


def test_step_launches_is_a_value_query():
    lib = _abi.load()
    with pytest.raises(TypeError, match="returns a value"):
        _abi.call("lt_policy_step_launches", desc(), N)
    for rnn_type in (LSTM, GRU):
        for n in (1, 50, 4096, 16 * 65535):
            assert lib.lt_policy_step_launches(ctypes.byref(desc(rnn_type=rnn_type)), n) == 2
    assert lib.lt_policy_step_launches(ctypes.byref(desc()), 0) == C["LT_EINVAL"]
    assert lib.lt_policy_step_launches(None, N) == C["LT_EINVAL"]
