"""lt_mlp_backward_pair_dx (include/lt_mlp_dx.h, csrc/lt_mlp_dx.hip): the gradient with respect to the INPUT ROWS of the actor and critic
stacks - what a recurrent policy's memories take as `dout` - behind the chain of lt_mlp_backward_pair, and `PackedPair.backward_raw(dx_out=...)`
on both of its paths.  dx against the same chain in float64, with torch's own f32 chain on the same inputs as the yardstick (the bound of
tests/test_hip_mlp_backward.py for gradients these kernels produce); every other output of the entry against lt_mlp_backward_pair's, bit
for bit."""
import ctypes

import pytest

from tests.mlp_ref import linears, ref_chain

pytestmark = pytest.mark.gpu

# (input width H, hidden widths, rows): 30 and 199 leave partial row tiles in the chain (16) and in the dx kernel (128); 199 rows of 256
# columns take two column blocks and two row blocks of it, 512 hidden features sixteen panels
CASES = [(64, (32, 16), 5, 48), (64, (32, 16), 5, 30), (256, (512, 256, 128), 12, 199)]
IDS = ["H64-m48", "H64-m30", "H256-m199"]


def _setup(H, hidden, out0, m):
    import torch
    import torch.nn as nn

    from locotouch_amd.rl import mlp as M

    torch.manual_seed(H + m)

    def stack(out):
        mods, prev = [], H
        for h in hidden:
            mods += [nn.Linear(prev, h), nn.ELU()]
            prev = h
        return nn.Sequential(*mods, nn.Linear(prev, out)).cuda()

    actor, critic = stack(out0), stack(1)
    g = torch.Generator(device="cuda").manual_seed(m)
    xs = [torch.tanh(torch.randn(m, H, device="cuda", generator=g)) for _ in range(2)]  # a memory's outputs lie in (-1, 1)
    dy0 = torch.randn(m, out0, device="cuda", generator=g) * 1e-3
    dy0[::7] *= 200.0  # heavy-tailed rows, as PPO's are
    dy0[5] = 0.0
    dys = [dy0, torch.randn(m, 1, device="cuda", generator=g) * 1e-3]
    return M, M.PackedPair(actor, critic), (actor, critic), xs, dys


_REF = {}


def _reference(case, nets, xs, dys):
    """(dx in float64, max |torch's f32 chain - it|) per network: computed once per case, shared, left unchanged."""
    import torch

    if case not in _REF:
        out = []
        for net, x, dy in zip(nets, xs, dys):
            with torch.no_grad():
                dz, _, _ = ref_chain(net, x, dy)
                dx64 = dz[0] @ linears(net)[0].weight.double()
            x32 = x.clone().requires_grad_(True)
            net(x32).backward(dy)
            out.append((dx64, float((x32.grad.double() - dx64).abs().max())))
            net.zero_grad()
        _REF[case] = out
    return _REF[case]


def _check_dx(tag, dx, ref):
    import torch

    for k, (got, (dx64, eu)) in enumerate(zip(dx, ref)):
        assert bool(torch.isfinite(got).all()), (tag, k, "an element of dx was not written")
        e, top = float((got.double() - dx64).abs().max()), float(dx64.abs().max())
        print(f"\n[mlp dx] {tag} net {k}: max |dx - dx64| {e:.3e}   torch f32 chain {eu:.3e}   max |dx64| {top:.3e}")
        assert e <= max(4.0 * eu, 1e-5 * top), (tag, k, e, eu, top)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("path", ["fused", "fused-split", "fused-library-gemm", "library"])
def test_dx_of_backward_raw_matches_float64(case, path, monkeypatch):
    """`PackedPair.backward_raw(dx_out=...)`: the chain kernel with the dx hop behind it (per-workgroup scales; ONE scale and split dz),
    the chain kernel with the library GEMM on the unsplit dz_0, and the library path - which one ran is asserted."""
    import torch

    M, pair, nets, xs, dys = _setup(*CASES[case])
    ref = _reference(case, nets, xs, dys)
    monkeypatch.setattr(M, "USE_FUSED_BACKWARD", path != "library")
    monkeypatch.setattr(M, "USE_DX_KERNEL", path != "fused-library-gemm")
    grads = {p: torch.full_like(p, float("nan")) for net in nets for p in net.parameters()}
    without = {p: torch.full_like(p, float("nan")) for p in grads}
    dx = tuple(torch.full_like(x, float("nan")) for x in xs)
    amax = (dys[0].abs().max().reshape(1), dys[1].abs().max().reshape(1)) if path == "fused-split" else None
    _, acts = pair.forward_raw(*xs, with_dx=True)
    pair.backward_raw(*xs, acts, *dys, grads, dy_amax=amax, dx_out=dx)
    assert pair.last_backward == ("library" if path == "library" else "fused")
    assert pair._dx_kernel_ok() == (path != "fused-library-gemm") and pair.acts_split == (path != "library")
    _, acts = pair.forward_raw(*xs)
    pair.backward_raw(*xs, acts, *dys, without, dy_amax=amax)  # dx_out None: as it was
    torch.cuda.synchronize()
    _check_dx(f"{IDS[case]} {path}", dx, ref)
    for p in grads:  # asking for dx changes no parameter gradient
        assert torch.equal(grads[p], without[p])
    if path != "library":
        assert float(pair.saturated()) == 0.0


def _chain(pair, entry, acts, dys, amax, dx=None):
    """One call of lt_mlp_backward_pair / lt_mlp_backward_pair_dx into NaN-filled outputs: (dz, amax, scales_out, sat_count)."""
    import torch

    from locotouch_amd import _abi

    m, nets = dys[0].shape[0], (pair.a, pair.b)
    nblk = _abi.load().lt_mlp_backward_blocks(ctypes.byref(nets[0].desc), ctypes.byref(nets[1].desc), m)
    nan = float("nan")
    dzs = [[torch.full_like(a, nan) for a in acts[k]] for k in range(2)]
    amaxs = [torch.full((len(acts[k]), nblk), nan, device="cuda") for k in range(2)]
    scales, sat = torch.full((2,), nan, device="cuda"), torch.zeros(1, device="cuda")
    args = []
    for k in range(2):
        args += [nets[k].desc, nets[k].bpacked, dys[k], _abi.ptr_array(acts[k]), _abi.ptr_array(dzs[k]), _abi.ptr_array(list(amaxs[k]))]
    args += [m, int(pair.acts_split), *(amax or (None, None)), int(amax is not None), scales, sat]
    if entry == "lt_mlp_backward_pair_dx":
        args += list(dx or (None, None))
    _abi.call(entry, *args, _abi.stream())
    torch.cuda.synchronize()
    return dzs, amaxs, scales, sat


def _same_bits(a, b):
    import torch

    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("split", [False, True], ids=["per-workgroup-scales", "one-scale-split-dz"])
def test_the_entry_leaves_every_other_output_as_lt_mlp_backward_pair_does(case, split):
    """dz, amax, scales_out and sat_count of the new entry - with dx and with both dx NULL - are the old entry's bits, in both scale modes;
    dx itself holds to float64, every element written, and two runs give the same bits."""
    import torch

    M, pair, nets, xs, dys = _setup(*CASES[case])
    ref = _reference(case, nets, xs, dys)
    _, acts = pair.forward_raw(*xs, with_dx=True)
    assert pair.acts_split and pair._dx_fresh and pair.a.bpacked_dx and pair.b.bpacked_dx
    amax = (dys[0].abs().max().reshape(1), dys[1].abs().max().reshape(1)) if split else None
    old = _chain(pair, "lt_mlp_backward_pair", acts, dys, amax)
    null = _chain(pair, "lt_mlp_backward_pair_dx", acts, dys, amax)
    assert _same_bits(old, null)
    runs = []
    for _ in range(2):
        dx = tuple(torch.full_like(x, float("nan")) for x in xs)
        assert _same_bits(old, _chain(pair, "lt_mlp_backward_pair_dx", acts, dys, amax, dx))
        runs.append(dx)
    assert _same_bits(runs[0], runs[1])
    _check_dx(f"{IDS[case]} entry split={split}", runs[0], ref)
    # one network's hop alone: the other's dx stays untouched
    only = (torch.full_like(xs[0], float("nan")), None)
    assert _same_bits(old, _chain(pair, "lt_mlp_backward_pair_dx", acts, dys, amax, only))
    assert _same_bits(only[0], runs[0][0])
    assert bool(torch.isfinite(old[2]).all()) and float(old[3]) == 0.0
