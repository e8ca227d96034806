"""include/lt_rnn_encoder.h: a unit of the C ABI with a header of its own, bound by one row of `_abi.HEADERS`, and the host-side
validation of its entry points.  No device is touched: every call below is decided on the host before anything is launched (the
pointers are made-up addresses that are never dereferenced)."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
A0 = 1 << 30  # made-up, 16-byte aligned addresses


def addr(k):
    return A0 + (k << 24)


def refusal(rc):
    assert rc == C["LT_EINVAL"], rc
    return _abi.load().lt_last_error().decode()


def names(msg, fn, field):
    assert msg.startswith(fn + ": invalid argument:") and re.search(rf"(?<![\w.]){re.escape(field)} must be\b", msg), msg


def refused(fn_name, args, field):
    _abi.load()
    fn, conv = _abi._calls[fn_name]
    names(refusal(fn(*[a if c is None else c(a) for c, a in zip(conv, args, strict=True)])), fn_name, field)
    with pytest.raises(RuntimeError, match=fn_name):
        _abi.call(fn_name, *args)


def test_header_is_a_unit_of_its_own_bound_by_one_row():
    rows = [r for r in _abi.HEADERS if r[1] == "lt_rnn_encoder.h"]
    assert len(rows) == 1 and rows[0][0] == "RNN_ENCODER"
    assert os.path.samefile(_abi.RNN_ENCODER_HEADER, os.path.join(_abi.REPO, "include", "lt_rnn_encoder.h"))
    entries = {"lt_memory_step_strided", "lt_memory_gru_step_strided", "lt_rnn_encoder_forward", "lt_rnn_encoder_forward_launches"}
    assert set(_abi.RNN_ENCODER_SIGNATURES) == entries
    assert C["LT_ABI_VERSION"] == 21 and "lt_rnn_encoder.h" not in open(_abi.HEADER).read()  # lt_env.h and the version are unchanged
    assert _abi.RNN_ENCODER_CONSTS["LT_RNN_ENCODER_MAX_LAYERS"] == _abi.ENCODER_CONSTS["LT_ENCODER_MAX_LAYERS"]
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    mem_p, net_p = ctypes.POINTER(_abi.LtRnnEncoderMemory), ctypes.POINTER(_abi.LtRnnEncoderNet)
    step = (ctypes.c_int, [mem_p, mem_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p])
    assert _abi.RNN_ENCODER_SIGNATURES["lt_memory_step_strided"] == _abi.RNN_ENCODER_SIGNATURES["lt_memory_gru_step_strided"] == step
    assert _abi.RNN_ENCODER_SIGNATURES["lt_rnn_encoder_forward"] == (ctypes.c_int, [net_p, net_p, ctypes.c_int, ctypes.c_void_p])
    assert _abi.RNN_ENCODER_SIGNATURES["lt_rnn_encoder_forward_launches"] == (ctypes.c_int, [net_p, net_p])
    assert _abi.RNN_ENCODER_VALUE_QUERIES == {"lt_rnn_encoder_forward_launches"}
    for name, (restype, argtypes) in _abi.RNN_ENCODER_SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype
        assert (name in _abi._calls) == (name not in _abi.RNN_ENCODER_VALUE_QUERIES)
    # additions only: the structures of the headers these kernels come from keep their layout
    assert [f[0] for f in _abi.LtMemoryNet._fields_] == ["x", "I", "w_ih", "w_hh", "b_ih", "b_hh", "h_in", "c_in", "h_out", "c_out", "saved_h", "saved_c"]
    assert [f[0] for f in _abi.LtMemoryGruNet._fields_] == ["x", "I", "w_ih", "w_hh", "b_ih", "b_hh", "h_in", "h_out", "saved_h"]
    assert [f[0] for f in _abi.LtEncoderNet._fields_] == ["desc", "obs", "obs_stride", "weight", "bias", "out", "acts"]


# ---- a. the strided memory step ----
def memory(base, lstm, **kw):
    m = _abi.LtRnnEncoderMemory()
    m.x, m.x_stride, m.I = addr(base) + 4 * 270, 348, 78  # the tail at column 270 of a 348-wide row: 8-byte aligned
    m.w_ih, m.w_hh, m.b_ih, m.b_hh = addr(base + 1), addr(base + 2), addr(base + 3), addr(base + 4)
    m.h_in, m.h_out, m.saved_h = addr(base + 5), addr(base + 6), addr(base + 7)
    if lstm:
        m.c_in, m.c_out, m.saved_c = addr(base + 8), addr(base + 9), addr(base + 10)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


STEP_REFUSALS = [("N", lambda L: [memory(1, L), memory(20, L), None, 0, 256, None]),
                 ("N", lambda L: [memory(1, L), memory(20, L), None, 16 * 65535 + 1, 256, None]),
                 ("H", lambda L: [memory(1, L), memory(20, L), None, 64, 96, None]),
                 ("H", lambda L: [memory(1, L), memory(20, L), None, 64, 576, None]),
                 ("actor", lambda L: [None, memory(20, L), None, 64, 256, None]),
                 ("critic", lambda L: [memory(1, L), None, None, 64, 256, None]),
                 ("actor.I", lambda L: [memory(1, L, I=0), memory(20, L), None, 64, 256, None]),
                 ("critic.I", lambda L: [memory(1, L), memory(20, L, I=1248 - 256 + 1, x_stride=2000), None, 64, 256, None]),
                 ("actor.x_stride", lambda L: [memory(1, L, x_stride=77), memory(20, L), None, 64, 256, None]),
                 ("critic.x_stride", lambda L: [memory(1, L), memory(20, L, x_stride=0), None, 64, 256, None]),
                 ("actor.x", lambda L: [memory(1, L, x=None), memory(20, L), None, 64, 256, None]),
                 ("actor.x", lambda L: [memory(1, L, x=addr(1) + 2), memory(20, L), None, 64, 256, None]),
                 ("critic.w_ih", lambda L: [memory(1, L), memory(20, L, w_ih=None), None, 64, 256, None]),
                 ("actor.w_hh", lambda L: [memory(1, L, w_hh=addr(2) + 4), memory(20, L), None, 64, 256, None]),
                 ("actor.b_hh", lambda L: [memory(1, L, b_hh=None), memory(20, L), None, 64, 256, None]),
                 ("actor.h_in", lambda L: [memory(1, L, h_in=addr(5) + 8), memory(20, L), None, 64, 256, None]),
                 ("critic.saved_h", lambda L: [memory(1, L), memory(20, L, saved_h=None), None, 64, 256, None]),
                 ("actor.h_out", lambda L: [memory(1, L, h_out=addr(6)), memory(20, L), None, 64, 256, None])]  # no ping-pong


@pytest.mark.parametrize("fn, lstm", [("lt_memory_step_strided", True), ("lt_memory_gru_step_strided", False)])
@pytest.mark.parametrize("field, make", STEP_REFUSALS, ids=[f"{i}-{f}" for i, (f, _) in enumerate(STEP_REFUSALS)])
def test_strided_step_names_what_it_refuses_before_touching_a_device(fn, lstm, field, make):
    if field == "actor.h_out" and lstm:
        field = "actor.h_out / .c_out"
    refused(fn, make(lstm), field)


def test_each_cell_asks_for_its_own_state_arrays():
    refused("lt_memory_step_strided", [memory(1, True, c_in=None), memory(20, True), None, 64, 256, None], "actor.c_in")
    refused("lt_memory_step_strided", [memory(1, True), memory(20, True, saved_c=addr(30) + 4), None, 64, 256, None], "critic.saved_c")
    refused("lt_memory_gru_step_strided", [memory(1, False), memory(20, True), None, 64, 256, None], "critic.c_in / .c_out / .saved_c")


# ---- b. the encoder on a second array ----
def net(base, **kw):
    """The teacher shape of the reference's cfg: rows of 348 columns, head 270; the GRU's 256 columns -> 256 -> 128 -> 64 -> 64, ELU, tanh."""
    n = _abi.LtRnnEncoderNet()
    n.obs_dim, n.flat_dim, n.enc_in = 348, 270, 256
    dims = kw.pop("dims", [256, 128, 64, 64])
    n.num_layers = len(dims)
    for l, w in enumerate(dims[:_abi.RNN_ENCODER_CONSTS["LT_RNN_ENCODER_MAX_LAYERS"]]):
        n.dims[l] = w
    n.activation, n.final_activation = C["LT_ACT_ELU"], C["LT_ACT_TANH"]
    n.obs, n.obs_stride, n.h, n.h_stride, n.out = addr(base), 348, addr(base + 1), 256, addr(base + 2)
    for l in range(min(n.num_layers, 6)):
        n.weight[l], n.bias[l] = addr(base + 3 + l), addr(base + 9 + l)
    for k, v in kw.items():
        if isinstance(v, dict):
            for l, x in v.items():
                getattr(n, k)[l] = x
        else:
            setattr(n, k, v)
    return n


def test_forward_launches_is_one_or_the_refusal():
    lib = _abi.load()
    assert lib.lt_rnn_encoder_forward_launches(ctypes.byref(net(1)), None) == 1
    assert lib.lt_rnn_encoder_forward_launches(ctypes.byref(net(1)), ctypes.byref(net(20, dims=[16, 8], enc_in=64, flat_dim=0))) == 1
    assert lib.lt_rnn_encoder_forward_launches(ctypes.byref(net(1, enc_in=512, obs_dim=14, flat_dim=9)), None) == 1  # h is not bounded by the row
    names(refusal(lib.lt_rnn_encoder_forward_launches(ctypes.byref(net(1)), ctypes.byref(net(20, enc_in=0)))), "lt_rnn_encoder_forward_launches", "critic.enc_in")
    names(refusal(lib.lt_rnn_encoder_forward_launches(ctypes.byref(net(1, enc_in=513)), None)), "lt_rnn_encoder_forward_launches", "actor.enc_in")
    names(refusal(lib.lt_rnn_encoder_forward_launches(ctypes.byref(net(1, dims=[12])), None)), "lt_rnn_encoder_forward_launches", "actor.dims[0]")
    names(refusal(lib.lt_rnn_encoder_forward_launches(None, None)), "lt_rnn_encoder_forward_launches", "actor")
    with pytest.raises(TypeError, match="returns a value"):
        _abi.call("lt_rnn_encoder_forward_launches", net(1), None)


FORWARD_REFUSALS = [("n", lambda: [net(1), None, 0, None]),
                    ("n", lambda: [net(1), None, 16 * 65535 + 1, None]),
                    ("actor", lambda: [None, None, 64, None]),
                    ("actor.dims[1]", lambda: [net(1, dims=[256, 100, 64, 64]), None, 64, None]),
                    ("actor.dims[3]", lambda: [net(1, dims=[256, 128, 64, 6]), None, 64, None]),
                    ("actor.num_layers", lambda: [net(1, dims=[]), None, 64, None]),
                    ("actor.num_layers", lambda: [net(1, dims=[8] * 7), None, 64, None]),
                    ("critic.enc_in", lambda: [net(1), net(30, enc_in=520), 64, None]),
                    ("actor.flat_dim", lambda: [net(1, flat_dim=349), None, 64, None]),
                    ("actor.obs_dim", lambda: [net(1, obs_dim=0, flat_dim=0), None, 64, None]),
                    ("actor.activation", lambda: [net(1, activation=C["LT_ACT_NONE"]), None, 64, None]),
                    ("actor.final_activation", lambda: [net(1, final_activation=-1), None, 64, None]),
                    ("actor.obs", lambda: [net(1, obs=None), None, 64, None]),
                    ("actor.obs", lambda: [net(1, obs=addr(1) + 2), None, 64, None]),
                    ("actor.obs_stride", lambda: [net(1, obs_stride=347), None, 64, None]),
                    ("actor.h", lambda: [net(1, h=None), None, 64, None]),
                    ("actor.h", lambda: [net(1, h=addr(2) + 8), None, 64, None]),  # 16-byte aligned rows
                    ("critic.h_stride", lambda: [net(1), net(30, h_stride=255), 64, None]),
                    ("actor.h_stride", lambda: [net(1, h_stride=258), None, 64, None]),  # not a multiple of 4
                    ("actor.out", lambda: [net(1, out=None), None, 64, None]),
                    ("actor.out", lambda: [net(1, out=addr(1) + 4 * 348), None, 64, None]),  # inside the rows it reads
                    ("actor.out", lambda: [net(1, out=addr(2) + 4 * 256), None, 64, None]),  # inside the h rows
                    ("actor.weight[2]", lambda: [net(1, weight={2: None}), None, 64, None]),
                    ("critic.bias[0]", lambda: [net(1), net(30, bias={0: None}), 64, None]),
                    ("actor.acts[0]", lambda: [net(1, acts={0: addr(40)}), None, 64, None]),  # the inference form alone
                    ("critic.acts[3]", lambda: [net(1), net(30, acts={3: addr(40)}), 64, None])]


@pytest.mark.parametrize("field, make", FORWARD_REFUSALS, ids=[f"{i}-{f}" for i, (f, _) in enumerate(FORWARD_REFUSALS)])
def test_forward_names_what_it_refuses_before_touching_a_device(field, make):
    refused("lt_rnn_encoder_forward", make(), field)
