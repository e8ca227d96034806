"""The host side of csrc/lt_wgrad.hip: what `lt_wgrad` and `lt_split_rows` refuse, and the values of `lt_wgrad_splits` /
`lt_wgrad_ws_floats`.  No device is touched: every call below is decided on the host before anything is launched (the pointers are
made-up addresses that are never dereferenced), as in tests/test_memory_seq_abi.py."""
import pytest

from locotouch_amd import _abi
from tests import wgrad_ref as R

C = _abi.CONSTS
A0 = 1 << 30  # made-up, 16-byte aligned addresses


def addr(k):
    return A0 + (k << 24)


def wgrad_args(**kw):
    a = dict(dz=addr(1), dz_split=0, dz_scale=None, x=addr(2), x_split=0, M=257, N=132, K=68, amax_blocks=addr(3), nblk_amax=6, slabs=addr(4),
             db_slabs=addr(5), stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def refused(name, args):
    """LT_EINVAL through the raw function and a RuntimeError through `_abi.call`, lt_last_error() naming the function"""
    _abi.load()
    fn, conv = _abi._calls[name]
    assert fn(*[a if c is None else c(a) for c, a in zip(conv, args, strict=True)]) == C["LT_EINVAL"] != 0, (name, args)
    assert _abi.load().lt_last_error().decode().startswith(name + ":"), _abi.load().lt_last_error()
    with pytest.raises(RuntimeError, match=name + " failed.*" + name + ":"):
        _abi.call(name, *args)


WGRAD_REFUSALS = [dict(dz=None), dict(x=None), dict(slabs=None), dict(M=0), dict(M=-1),
                  *[{d: v} for d in ("N", "K") for v in (0, 2, 6, -4)],
                  dict(nblk_amax=0), dict(nblk_amax=-1), dict(dz_split=1), dict(dz_split=1, x_split=1),
                  dict(M=1 << 21, N=4, K=512), dict(M=1 << 21, N=512, K=4), dict(M=1 << 30, N=4, K=4)]  # an operand of exactly 4 GiB


@pytest.mark.parametrize("kw", WGRAD_REFUSALS, ids=str)
def test_wgrad_refuses_before_touching_a_device(kw):
    refused("lt_wgrad", wgrad_args(**kw))


@pytest.mark.parametrize("kw", [dict(count=0), dict(count=2), dict(count=6), dict(count=-4), dict(x=None), dict(out=None)], ids=str)
def test_split_rows_refuses_before_touching_a_device(kw):
    a = dict(x=addr(1), out=addr(2), count=1032, stream=None)
    a.update(kw)
    refused("lt_split_rows", list(a.values()))


SPLITS_TABLE = {  # every shape of tests/test_hip_wgrad_f64.py, the layers of the LocoTouch networks, and the steps at which a slice is added
    (1, 4, 4): 1, (31, 68, 60): 1, (32, 64, 64): 1, (33, 64, 64): 1, (255, 12, 132): 1, (257, 132, 68): 1, (480, 64, 64): 1, (481, 64, 64): 2,
    (511, 64, 64): 2, (512, 64, 64): 2, (513, 64, 64): 2, (4100, 64, 64): 16, (2049, 132, 348): 8, ((1 << 21) - 1, 4, 512): 64,
    (24576, 512, 348): 10, (24576, 256, 512): 16, (24576, 128, 256): 64, (6144, 512, 348): 10, (1 << 20, 4, 4): 512, (1 << 20, 68, 4): 256,
    (255, 64, 64): 1, (256, 64, 64): 1, (257, 64, 64): 1, (736, 64, 64): 2, (737, 64, 64): 3,
}


def test_splits_and_workspace_are_the_stated_functions_of_the_shape():
    """lt_wgrad_splits == max(1, min(512 // tiles, ceil(M / 32) // 8)) with 64 x 64 tiles, lt_wgrad_ws_floats == splits * N * K: over the
    table (a shape must not drift to another slice count unnoticed) and over a sweep."""
    lib = _abi.load()
    assert set(R.SHAPES) <= set(SPLITS_TABLE)
    for (m, n, k), sp in SPLITS_TABLE.items():
        assert lib.lt_wgrad_splits(m, n, k) == sp == R.splits_of(m, n, k), (m, n, k, lib.lt_wgrad_splits(m, n, k), R.splits_of(m, n, k))
        assert lib.lt_wgrad_ws_floats(m, n, k) == sp * n * k
    for m in (1, 255, 256, 257, 479, 480, 481, 1000, 4096, 24576, 100000):
        for n in (4, 60, 64, 68, 512, 1024):
            for k in (4, 64, 348, 512):
                tiles = -(-n // 64) * -(-k // 64)
                want = max(1, min(512 // tiles, -(-m // 32) // 8))
                assert lib.lt_wgrad_splits(m, n, k) == want and lib.lt_wgrad_ws_floats(m, n, k) == want * n * k, (m, n, k)
