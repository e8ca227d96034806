"""include/lt_memory_dx.h: a header of its own, bound by one row of `_abi.HEADERS`, and the argument validation of its entry point and its
value query.  No device is touched: every call below is decided on the host before anything is launched (the pointers are made-up
addresses that are never dereferenced) - as tests/test_memory_seq_abi.py for the sequence passes this hop stands behind."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi

C = _abi.CONSTS
_vp, _int, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
A0 = 1 << 30  # made-up, 16-byte aligned addresses, 16 MiB apart (the largest array below, dg, is 70 * 4 * 128 * 4 B = 140 KiB)
FIELDS = ("dg", "w_ih", "I", "dx", "dx_stride")
N, H, GATES = 70, 128, 4
ENTRY, QUERY = "lt_memory_input_grad", "lt_memory_input_grad_launches"


def addr(k):
    return A0 + (k << 24)


def net(base, I=24, **kw):
    a = dict(dg=addr(base), w_ih=addr(base + 1), I=I, dx=addr(base + 2), dx_stride=I + 3)
    assert set(kw) <= set(a)
    a.update(kw)
    return _abi.LtMemoryDxNet(**a)


def args(actor=None, critic=None, **kw):
    a = dict(actor=net(1, **(actor or {})), critic=net(20, **{"I": 31, **(critic or {})}), n=N, H=H, gates=GATES, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def status(call_args):
    """(value of the query, its text, status of the entry point, its text).  The entry point is called ONLY where the query has refused
    the same arguments: the two share one validation, and a call that passed it would launch on the made-up addresses."""
    lib = _abi.load()
    q = getattr(lib, QUERY)(*[ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in call_args[:-1]])
    if q >= 0:
        return q, "", None, ""
    qmsg = lib.lt_last_error().decode()
    fn, conv = _abi._calls[ENTRY]
    rc = fn(*[a if c is None else c(a) for c, a in zip(conv, call_args, strict=True)])
    return q, qmsg, rc, lib.lt_last_error().decode()


def refused(call_args, field):
    """LT_EINVAL through the raw function and the query, a RuntimeError through `_abi.call`; both texts name their function and the field."""
    q, qmsg, rc, msg = status(call_args)
    assert rc == C["LT_EINVAL"] and q == C["LT_EINVAL"] < 0, (field, rc, q)
    for name, text in ((ENTRY, msg), (QUERY, qmsg)):
        assert text.startswith(name + ": invalid argument: ") and re.search(rf"(?<![\w.]){re.escape(field)} must be\b", text), text
    with pytest.raises(RuntimeError, match=ENTRY):
        _abi.call(ENTRY, *call_args)


def test_header_is_bound_by_its_row_and_leaves_the_abi_pins_alone():
    rows = [r for r in _abi.HEADERS if r[1] == "lt_memory_dx.h"]
    assert rows == [("MEMORY_DX", "lt_memory_dx.h", False, (QUERY,), ("lt_memory_dx_net",))]
    assert os.path.samefile(_abi.MEMORY_DX_HEADER, os.path.join(_abi.REPO, "include", "lt_memory_dx.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.MEMORY_DX_HEADER).read(), flags=re.S))
    assert set(re.findall(r"\b(lt_\w+)\s*\(", src)) == set(_abi.MEMORY_DX_SIGNATURES) == {ENTRY, QUERY}
    assert _abi.MEMORY_DX_VALUE_QUERIES == {QUERY}
    net_p = ctypes.POINTER(_abi.LtMemoryDxNet)
    assert _abi.MEMORY_DX_SIGNATURES[ENTRY] == (_int, [net_p, net_p, _i64, _int, _int, _vp])  # (actor, critic, n, H, gates, stream)
    assert _abi.MEMORY_DX_SIGNATURES[QUERY] == (_int, [net_p, net_p, _i64, _int, _int])
    assert [(n, t) for n, t in _abi.LtMemoryDxNet._fields_] == [(f, _int if f == "I" else _i64 if f == "dx_stride" else _vp) for f in FIELDS]
    assert C["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67  # lt_env.h's own prototypes and the version are unchanged
    assert set(_abi.MEMORY_SEQ_SIGNATURES) == {"lt_memory_seq_forward", "lt_memory_seq_backward", "lt_memory_seq_backward_units"}
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    for name, (restype, argtypes) in _abi.MEMORY_DX_SIGNATURES.items():
        fn = getattr(lib, name)  # exported ...
        assert list(fn.argtypes) == argtypes and fn.restype is restype
        assert (name in _abi._calls) != (name in _abi.MEMORY_DX_VALUE_QUERIES)  # ... and launched through `_abi.call`, or a value query
    with pytest.raises(TypeError, match="returns a value"):
        _abi.call(QUERY, *args()[:-1])


REFUSALS = [
    ("gates", dict(gates=2)), ("gates", dict(gates=5)), ("gates", dict(gates=0)),
    ("H", dict(H=96)), ("H", dict(H=576)), ("H", dict(H=0)),
    ("n", dict(n=0)), ("n", dict(n=-1)), ("n", dict(n=16 * 65535 + 1)), ("n", dict(n=(1 << 32) + 5)),
    ("actor.I", dict(actor=dict(I=0))), ("critic.I", dict(critic=dict(I=0))),
    ("actor.I", dict(actor=dict(I=513, dx_stride=600), H=64)), ("critic.I", dict(critic=dict(I=513, dx_stride=600), H=64)),
    # I + H = 1249: with H <= 512 that is an I above 512 as well, refused for the same field
    ("actor.I", dict(actor=dict(I=1249 - 512, dx_stride=800), H=512)), ("critic.I", dict(critic=dict(I=1249 - H, dx_stride=1200))),
    ("actor.dx_stride", dict(actor=dict(dx_stride=23))), ("critic.dx_stride", dict(critic=dict(dx_stride=0))),
    ("actor.dg", dict(actor=dict(dg=None))), ("actor.dg", dict(actor=dict(dg=addr(1) + 4))), ("critic.dg", dict(critic=dict(dg=addr(20) + 8))),
    ("actor.w_ih", dict(actor=dict(w_ih=None))), ("critic.w_ih", dict(critic=dict(w_ih=addr(21) + 2))),
    ("actor.dx", dict(actor=dict(dx=None))), ("critic.dx", dict(critic=dict(dx=addr(22) + 1))),
]


@pytest.mark.parametrize("field, kw", REFUSALS, ids=str)
def test_names_what_it_refuses_before_touching_a_device(field, kw):
    refused(args(**kw), field)


def test_the_widest_row_passes_and_one_float_more_is_refused():
    """I = 512 passes the width check (a call whose only other fault is its stride is refused for the stride); 513 is refused for I."""
    assert status(args(actor=dict(I=512, dx_stride=512), H=64))[0] == 1
    assert status(args(actor=dict(I=512, dx_stride=512), H=512, gates=3))[0] == 1
    refused(args(actor=dict(I=512, dx_stride=511), H=64), "actor.dx_stride")
    refused(args(actor=dict(I=513, dx_stride=513), H=64), "actor.I")


@pytest.mark.parametrize("who, base", [("actor", 1), ("critic", 20)])
def test_refuses_an_output_that_overlaps_an_input(who, base):
    """Overlap, not equality: dx in the MIDDLE of dg, dx ending inside w_ih, and the other network's inputs as well."""
    other, obase = ("critic", 20) if who == "actor" else ("actor", 1)
    inside_dg = addr(base) + 4 * (N * GATES * H // 2)
    refused(args(**{who: dict(dx=inside_dg)}), f"{who}.dx")
    I = 24 if who == "actor" else 31
    ends_in_w = addr(base + 1) - 4 * ((N - 1) * (I + 3) + I) + 4  # its last float is w_ih's first
    refused(args(**{who: dict(dx=ends_in_w)}), f"{who}.dx")
    refused(args(**{who: dict(dx=addr(obase) + 16)}), f"{who}.dx")
    refused(args(**{who: dict(dx=addr(obase + 1) + 4)}), f"{who}.dx")
    # one float in front of w_ih is no overlap: the query says one launch
    assert status(args(**{who: dict(dx=ends_in_w - 4)}))[0] == 1


def test_the_query_answers_one_launch_for_one_network_and_for_two():
    lib = _abi.load()
    q = getattr(lib, QUERY)
    a = args()
    assert q(ctypes.byref(a[0]), ctypes.byref(a[1]), N, H, GATES) == 1
    assert q(ctypes.byref(a[0]), None, N, H, GATES) == 1  # critic = NULL passes the validation
    assert q(ctypes.byref(a[0]), None, N, H, 3) == 1
    assert q(None, ctypes.byref(a[1]), N, H, GATES) == C["LT_EINVAL"]
    assert re.search(r"(?<![\w.])actor must be\b", lib.lt_last_error().decode())
    for h in range(64, 513, 64):
        for g in (3, 4):
            for n in (1, 17, 16 * 65535):
                wide = net(1, I=min(512, 1248 - h), w_ih=1 << 28, dg=1 << 40, dx=1 << 44)  # (n * K floats of dg: far apart)
                assert q(ctypes.byref(wide), None, n, h, g) == 1, (h, g, n)
    # a critic that is refused when given is not looked at when it is NULL
    fn, conv = _abi._calls[ENTRY]
    bad = args(critic=dict(I=0))
    assert fn(*[x if c is None else c(x) for c, x in zip(conv, bad, strict=True)]) == C["LT_EINVAL"]
    bad[1] = None
    assert q(ctypes.byref(bad[0]), None, N, H, GATES) == 1
