"""`PPO(direct_recurrent_update=True)` (rl/ppo.py `_direct_recurrent_update`) and its C entry lt_mlp_backward_pair_dx (include/lt_mlp_dx.h),
what holds without a GPU: the key refuses by name what it does not serve, the row index of an env block is the reference's dealing,
the header is bound through `_abi.HEADERS`, and the entry refuses bad arguments by their field's name before anything is launched."""
import ctypes

import pytest
import torch

from locotouch_amd import _abi
from locotouch_amd.rl import PPO
from locotouch_amd.rl.modules import ActorCriticRecurrent

from .test_recurrent_update_form import ACT, COBS, H, OBS


def _policy(**kw):
    return ActorCriticRecurrent(OBS, COBS, ACT, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_type="lstm", rnn_hidden_size=H, **kw)


def test_the_key_refuses_the_cpu_and_a_missing_whole_rollout_update_by_name():
    with pytest.raises(ValueError, match=r"^direct_recurrent_update: .*GPU"):
        PPO(_policy(), device="cpu", fused_recurrent_update=True, direct_recurrent_update=True)
    with pytest.raises(ValueError, match=r"^direct_recurrent_update: .*fused_recurrent_update"):
        PPO(_policy(), device="cpu", direct_recurrent_update=True)
    with pytest.raises(ValueError, match=r"^direct_recurrent_update: .*fused_recurrent_update"):
        PPO(_policy(), device="cpu", fused_recurrent_update=False, direct_recurrent_update=True)
    # off (the default, or spelled out) the key changes nothing: the whole-rollout update is built as before
    alg = PPO(_policy(), device="cpu", fused_recurrent_update=True, direct_recurrent_update=False)
    assert alg.fused_recurrent_update and not alg.direct_recurrent_update
    assert not PPO(_policy(), device="cpu").direct_recurrent_update


@pytest.mark.parametrize("nmb", [2, 3])
def test_the_block_row_index_is_the_reference_dealing(nmb):
    T, N = 6, 8
    per = N // nmb  # 3 minibatches of 8 envs: 2 envs each, envs 6 and 7 are dropped
    idx = PPO._block_row_index(T, N, nmb)
    assert idx.dtype == torch.int64 and idx.shape == (nmb, T * per) and idx.is_contiguous()
    rows = torch.arange(T * N).view(T, N)
    for i in range(nmb):
        assert torch.equal(idx[i], rows[:, i * per:(i + 1) * per].reshape(-1))
        for t in range(T):
            for j in range(per):
                assert int(idx[i, t * per + j]) == t * N + i * per + j
    if nmb == 3:
        assert not set(idx.reshape(-1).tolist()) & {t * N + e for t in range(T) for e in (6, 7)}


def test_the_header_is_bound_through_the_table():
    row = [r for r in _abi.HEADERS if r[1] == "lt_mlp_dx.h"]
    assert len(row) == 1 and row[0][0] == "MLP_DX" and row[0][2]  # (it uses lt_env.h's lt_mlp_desc)
    assert set(_abi.MLP_DX_SIGNATURES) == {"lt_mlp_backward_dx_packed_floats", "lt_mlp_pack_training_dx", "lt_mlp_backward_pair_dx"}
    assert "lt_mlp_dx.h" not in open(_abi.HEADER).read() and _abi.CONSTS["LT_ABI_VERSION"] == 21
    old, new = _abi.SIGNATURES["lt_mlp_backward_pair"][1], _abi.MLP_DX_SIGNATURES["lt_mlp_backward_pair_dx"][1]
    assert new == old[:-1] + [ctypes.c_void_p, ctypes.c_void_p] + old[-1:]  # lt_mlp_backward_pair's arguments plus dx0, dx1 in front of the stream
    _abi.load()
    assert all(name in _abi._calls for name in _abi.MLP_DX_SIGNATURES)


def _desc(dims, activation="LT_ACT_ELU"):
    d = _abi.LtMlpDesc()
    d.num_layers = len(dims) - 1
    for i, w in enumerate(dims):
        d.dims[i] = w
    d.activation = _abi.CONSTS[activation]
    return d


def _args(d0, d1, **replace):
    """A full argument list of lt_mlp_backward_pair_dx over host memory (nothing is dereferenced before the checks have passed)."""
    buf = torch.zeros(64)  # 16-byte aligned host floats stand in for every device buffer
    assert buf.data_ptr() % 16 == 0
    layers = _abi.ptr_array([buf] * 6)
    a = dict(fwd0=d0, bpacked0=buf, dy0=buf, acts0=layers, dz0=layers, amax0=layers, fwd1=d1, bpacked1=buf, dy1=buf, acts1=layers, dz1=layers,
             amax1=layers, m=48, acts_split=1, in_amax0=None, in_amax1=None, dz_split=0, scales_out=buf, sat_count=None, dx0=buf, dx1=buf, stream=None)
    assert not set(replace) - set(a)
    a.update(replace)
    return list(a.values()), buf


def _refusal(args):
    lib = _abi.load()
    fn, conv = _abi._calls["lt_mlp_backward_pair_dx"]
    rc = fn(*[x if c is None else c(x) for c, x in zip(conv, args, strict=True)])
    return rc, (lib.lt_last_error() or b"").decode()


def test_the_entry_refuses_by_field_name_before_any_launch():
    good = _desc([64, 32, 16, 5])
    E = _abi.CONSTS["LT_EINVAL"]
    cases = [
        (dict(fwd0=_desc([64, 32, 16, 5], "LT_ACT_TANH")), "network 0: fwd must be a network with a backward stream"),   # no ELU: no backward stream
        (dict(fwd1=_desc([64, 5])), "network 1: fwd must be a network with a backward stream"),                              # one layer
        (dict(fwd1=_desc([64, 36, 16, 1])), "network 1: fwd must be a network with a backward stream"),                      # hidden width not % 8
        (dict(fwd0=_desc([60, 32, 16, 5])), "network 0: fwd->dims[0] must be a multiple of 8 and <= 512"),
        (dict(fwd1=_desc([520, 32, 16, 1])), "network 1: fwd->dims[0] must be a multiple of 8 and <= 512"),
        (dict(fwd0=None), "network 0: fwd must be non-null"),
        (dict(bpacked0=None), "network 0: bpacked must be non-null"),
        (dict(dy1=None), "network 1: dy must be non-null"),
        (dict(acts0=None), "network 0: acts must be non-null"),
        (dict(dz1=None), "network 1: dz must be non-null"),
        (dict(amax0=None), "network 0: amax must be non-null"),
        (dict(dz0=_abi.ptr_array([None] * 6)), "network 0: dz[l] must be non-null"),
        (dict(m=0), "m must be positive"),
        (dict(dz_split=1), "in_amax0, in_amax1 and scales_out must be non-null where dz_split is set"),
    ]
    for replace, text in cases:
        args, _keep = _args(good, _desc([64, 32, 16, 1]), **replace)
        rc, msg = _refusal(args)
        assert rc == E and msg.startswith("lt_mlp_backward_pair_dx: invalid argument: ") and text in msg, (replace, rc, msg)
    # an input width the hop refuses is fine where that network's dx is NULL: the entry is then lt_mlp_backward_pair for it
    args, _keep = _args(_desc([60, 32, 16, 5]), _desc([64, 32, 16, 1]), dx0=None, bpacked1=None)
    rc, msg = _refusal(args)
    assert rc == E and "network 1: bpacked must be non-null" in msg, msg  # (the check went past network 0's width)


def test_the_size_query_covers_the_streams_and_w0():
    lib, d = _abi.load(), _desc([64, 32, 16, 5])
    base, full = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.lt_mlp_backward_packed_floats(ctypes.byref(d), ctypes.byref(base)) == 0
    assert lib.lt_mlp_backward_dx_packed_floats(ctypes.byref(d), ctypes.byref(full)) == 0
    assert full.value == base.value + 32 * 64 and base.value % 4 == 0  # W_0 [32][64] behind the streams, 16-byte aligned
    bad = _desc([60, 32, 16, 5])
    assert lib.lt_mlp_backward_dx_packed_floats(ctypes.byref(bad), ctypes.byref(full)) == _abi.CONSTS["LT_EINVAL"]
    assert b"lt_mlp_backward_dx_packed_floats: invalid argument: fwd must be" in lib.lt_last_error()
