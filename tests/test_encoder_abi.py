"""include/lt_encoder.h: a unit of the C ABI with a header of its own, bound by one row of `_abi.HEADERS`, and the host-side validation
of its entry points.  No device is touched: every call below is decided on the host before anything is launched (the pointers of
the forward's refusals are made-up addresses that are never dereferenced)."""
import ctypes
import os
import re

import pytest

from locotouch_amd import _abi
from locotouch_amd.rl import encoder

C = _abi.CONSTS
EC = _abi.ENCODER_CONSTS
A0 = 1 << 30  # made-up, 16-byte aligned addresses


def addr(k):
    return A0 + (k << 24)


def reference_desc(**kw):
    """The teacher shape of the reference's cfg: rows of 348 columns, head 270, tail 78 -> 256 -> 128 -> 64 -> 64, ELU, tanh behind it."""
    a = dict(obs_dim=348, flat_dim=270, enc_in=78, dims=[256, 128, 64, 64], activation=C["LT_ACT_ELU"], final_activation=C["LT_ACT_TANH"])
    assert set(kw) <= set(a)
    a.update(kw)
    return encoder.make_desc(**a)


def net(base, desc=None, **kw):
    n = _abi.LtEncoderNet()
    n.desc = reference_desc() if desc is None else desc
    n.obs, n.obs_stride, n.out = addr(base), n.desc.obs_dim, addr(base + 1)
    for l in range(n.desc.num_layers):
        n.weight[l], n.bias[l] = addr(base + 2 + l), addr(base + 8 + l)
    for k, v in kw.items():
        if isinstance(v, dict):
            for l, x in v.items():
                getattr(n, k)[l] = x
        else:
            setattr(n, k, v)
    return n


def refusal(rc):
    assert rc == C["LT_EINVAL"], rc
    return _abi.load().lt_last_error().decode()


def names(msg, fn, field):
    assert msg.startswith(fn + ":") and re.search(rf"(?<![\w.]){re.escape(field)} must be\b", msg), msg


def test_header_is_a_unit_of_its_own_bound_by_one_row():
    rows = [r for r in _abi.HEADERS if r[1] == "lt_encoder.h"]
    assert len(rows) == 1 and rows[0][0] == "ENCODER"
    assert os.path.samefile(_abi.ENCODER_HEADER, os.path.join(_abi.REPO, "include", "lt_encoder.h"))
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.ENCODER_HEADER).read(), flags=re.S))
    declared = set(re.findall(r"\b(lt_\w+)\s*\(", src))
    assert declared == set(_abi.ENCODER_SIGNATURES) == {"lt_encoder_validate", "lt_encoder_forward", "lt_encoder_forward_launches"}
    assert C["LT_ABI_VERSION"] == 21 and "lt_encoder.h" not in open(_abi.HEADER).read()  # lt_env.h and the version are unchanged
    assert EC["LT_ENCODER_MAX_LAYERS"] == C["LT_MLP_MAX_LAYERS"] and EC["LT_ENCODER_MAX_WIDTH"] == 512
    lib = _abi.load()
    assert lib.lt_abi_version() == 21
    net_p, desc_p = ctypes.POINTER(_abi.LtEncoderNet), ctypes.POINTER(_abi.LtEncoderDesc)
    assert _abi.ENCODER_SIGNATURES["lt_encoder_forward"] == (ctypes.c_int, [net_p, net_p, ctypes.c_int, ctypes.c_void_p])
    assert _abi.ENCODER_SIGNATURES["lt_encoder_validate"] == (ctypes.c_int, [desc_p])
    assert _abi.ENCODER_SIGNATURES["lt_encoder_forward_launches"] == (ctypes.c_int, [desc_p, desc_p])
    assert _abi.ENCODER_VALUE_QUERIES == {"lt_encoder_forward_launches"}
    for name, (restype, argtypes) in _abi.ENCODER_SIGNATURES.items():
        fn = getattr(lib, name)  # exported, with the header's types ...
        assert list(fn.argtypes) == argtypes and fn.restype is restype
        assert (name in _abi._calls) == (name not in _abi.ENCODER_VALUE_QUERIES)  # ... and the status-returning ones go through `_abi.call`
    others = set()
    for prefix, *_ in _abi.HEADERS:
        if prefix != "ENCODER":
            others |= set(getattr(_abi, (prefix + "_" if prefix else "") + "SIGNATURES"))
    assert not declared & others


def test_validate_accepts_the_reference_shape_and_the_smallest_ones():
    lib = _abi.load()
    assert lib.lt_encoder_validate(ctypes.byref(reference_desc())) == 0
    assert encoder.validate(reference_desc()) is None
    assert encoder.validate(reference_desc(obs_dim=14, flat_dim=9, enc_in=5, dims=[16, 8, 8], final_activation=C["LT_ACT_NONE"])) is None
    assert encoder.validate(reference_desc(obs_dim=1, flat_dim=0, enc_in=1, dims=[8], final_activation=C["LT_ACT_ELU"])) is None
    assert encoder.validate(reference_desc(dims=[512] * 6, enc_in=348, flat_dim=348)) is None


REFUSALS = [("desc.dims[1]", dict(dims=[256, 100, 64, 64])),            # a width that is not a multiple of 8
            ("desc.dims[3]", dict(dims=[256, 128, 64, 6])),              # ... the embedding's
            ("desc.dims[0]", dict(dims=[520, 128, 64, 64])),             # a width above 512
            ("desc.dims[2]", dict(dims=[256, 128, 0, 64])),
            ("desc.num_layers", dict(dims=[])),                          # zero layers
            ("desc.num_layers", dict(dims=[8] * 7)),                     # more than LT_ENCODER_MAX_LAYERS
            ("desc.activation", dict(activation=7)),                     # a bad activation
            ("desc.activation", dict(activation=C["LT_ACT_NONE"])),      # (none between the layers is no MLP)
            ("desc.final_activation", dict(final_activation=-1)),
            ("desc.enc_in", dict(enc_in=0)),                             # enc_in < 1
            ("desc.enc_in", dict(enc_in=-3)),
            ("desc.enc_in", dict(enc_in=349)),                           # more columns than the row has
            ("desc.flat_dim", dict(flat_dim=349)),
            ("desc.flat_dim", dict(flat_dim=-1)),
            ("desc.obs_dim", dict(obs_dim=0))]


@pytest.mark.parametrize("field, kw", REFUSALS, ids=str)
def test_validate_names_the_field_it_refuses(field, kw):
    d = reference_desc(**kw)  # (seven widths: make_desc fills the six the struct holds and says 7)
    names(refusal(_abi.load().lt_encoder_validate(ctypes.byref(d))), "lt_encoder_validate", field)
    assert field in encoder.validate(d)


def test_validate_refuses_a_null_descriptor():
    names(refusal(_abi.load().lt_encoder_validate(None)), "lt_encoder_validate", "desc")


def test_forward_launches_is_one_or_the_refusal():
    lib = _abi.load()
    small = reference_desc(obs_dim=14, flat_dim=9, enc_in=5, dims=[16, 8], final_activation=C["LT_ACT_NONE"])
    assert lib.lt_encoder_forward_launches(ctypes.byref(reference_desc()), None) == 1
    assert lib.lt_encoder_forward_launches(ctypes.byref(reference_desc()), ctypes.byref(small)) == 1
    names(refusal(lib.lt_encoder_forward_launches(ctypes.byref(reference_desc()), ctypes.byref(reference_desc(enc_in=0)))),
          "lt_encoder_forward_launches", "critic.enc_in")
    names(refusal(lib.lt_encoder_forward_launches(ctypes.byref(reference_desc(dims=[12])), None)), "lt_encoder_forward_launches", "actor.dims[0]")
    with pytest.raises(TypeError, match="returns a value"):
        _abi.call("lt_encoder_forward_launches", reference_desc(), None)


def forward_refused(args, field):
    _abi.load()
    fn, conv = _abi._calls["lt_encoder_forward"]
    names(refusal(fn(*[a if c is None else c(a) for c, a in zip(conv, args, strict=True)])), "lt_encoder_forward", field)
    with pytest.raises(RuntimeError, match="lt_encoder_forward"):
        _abi.call("lt_encoder_forward", *args)


FORWARD_REFUSALS = [("n", lambda: [net(1), None, 0, None]),
                    ("n", lambda: [net(1), None, 16 * 65535 + 1, None]),
                    ("actor", lambda: [None, None, 64, None]),
                    ("actor.desc.dims[1]", lambda: [net(1, reference_desc(dims=[256, 100, 64, 64])), None, 64, None]),
                    ("critic.desc.enc_in", lambda: [net(1), net(30, reference_desc(enc_in=0)), 64, None]),
                    ("actor.obs", lambda: [net(1, obs=None), None, 64, None]),
                    ("actor.obs", lambda: [net(1, obs=addr(1) + 2), None, 64, None]),
                    ("actor.out", lambda: [net(1, out=None), None, 64, None]),
                    ("actor.out", lambda: [net(1, out=addr(1) + 4 * 348), None, 64, None]),  # inside the rows it reads
                    ("actor.obs_stride", lambda: [net(1, obs_stride=347), None, 64, None]),
                    ("actor.weight[2]", lambda: [net(1, weight={2: None}), None, 64, None]),
                    ("critic.bias[0]", lambda: [net(1), net(30, bias={0: None}), 64, None]),
                    ("actor.acts[1]", lambda: [net(1, acts={0: addr(20), 2: addr(22), 3: addr(23)}), None, 64, None]),  # a hidden buffer missing
                    ("actor.acts[3]", lambda: [net(1, acts={0: addr(20), 1: addr(21), 2: addr(22)}), None, 64, None]),  # tanh: the pre-activation too
                    ("actor.acts[4]", lambda: [net(1, acts={0: addr(20), 1: addr(21), 2: addr(22), 3: addr(23), 4: addr(24)}), None, 64, None])]


@pytest.mark.parametrize("field, make", FORWARD_REFUSALS, ids=[f"{i}-{f}" for i, (f, _) in enumerate(FORWARD_REFUSALS)])
def test_forward_names_what_it_refuses_before_touching_a_device(field, make):
    forward_refused(make(), field)


def test_describe_reads_the_reference_encoder_from_its_module():
    import torch

    from locotouch_amd.rl.models import MLP

    desc, linears = encoder.describe(MLP(78, [256, 128, 64], 64, activation="elu", final_layer_activation="tanh"), 348, 270)
    assert (desc.obs_dim, desc.flat_dim, desc.enc_in, desc.num_layers) == (348, 270, 78, 4)
    assert list(desc.dims)[:4] == [256, 128, 64, 64] and len(linears) == 4
    assert (desc.activation, desc.final_activation) == (C["LT_ACT_ELU"], C["LT_ACT_TANH"])
    desc, _ = encoder.describe(MLP(5, [], 8, activation="relu"), 14, 9)
    assert (desc.num_layers, desc.final_activation) == (1, C["LT_ACT_NONE"])
    with pytest.raises(ValueError, match=r"dims\[2\] must be"):
        encoder.describe(MLP(5, [16, 8], 6), 14, 9)
    with pytest.raises(ValueError, match="SELU"):
        encoder.describe(MLP(5, [16], 8, activation="selu"), 14, 9)
    with pytest.raises(ValueError, match="Linear"):
        encoder.describe(torch.nn.Sequential(torch.nn.ELU()), 14, 9)
