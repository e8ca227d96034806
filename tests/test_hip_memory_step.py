"""csrc/lt_memory.hip (`lt_memory_step`, `lt_memory_finish`): one rollout step of the actor's and the critic's LSTM memory in one launch,
against a float64 `nn.LSTM` cell written here, and against the eager composition the kernel replaces (the library GEMM for the input
gates + `lt_lstm_forward(L = 1)`) on the same inputs.

Tolerance: none fixed in advance.  The kernel sums the same exact f32 products as the eager composition in another order, so its
largest error against f64 may be at most TWICE the composition's on the same inputs, per shape; both figures are printed."""
import pytest

pytestmark = pytest.mark.gpu

# N, I (the critic reads I + 7 columns), H
SHAPES = [(1, 5, 64),       # smallest
          (17, 270, 128),   # ragged row tile; row width not a multiple of 4
          (80, 64, 256),    # more than one row block
          (48, 33, 512),    # largest H
          (20, 150, 512)]   # I + H past what 64 gate rows leave room for in LDS: the 8-unit form of the kernel
STEPS = 4  # dones in front of step t: NULL, all zero, mixed, all one; the finish takes a mixed row again


def cell64(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """nn.LSTM's cell (gate order i, f, g, o) in float64."""
    import torch

    a = x.double() @ w_ih.double().t() + b_ih.double() + h.double() @ w_hh.double().t() + b_hh.double()
    i, f, g, o = a.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c.double() + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def make_case(n, i, h, seed):
    import torch

    gen = torch.Generator(device="cpu").manual_seed(seed)
    dev = "cuda:0"
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(dev)  # noqa: E731
    nets = []
    for width in (i, i + 7):  # actor, critic: different widths and weights, so that a swapped pointer shows
        k = 1.0 / h ** 0.5
        nets.append(dict(I=width, x=[r(n, width) for _ in range(STEPS)], w_ih=r(4 * h, width, scale=2 * k), w_hh=r(4 * h, h, scale=2 * k),
                         b_ih=r(4 * h, scale=0.3), b_hh=r(4 * h, scale=0.3), h0=torch.tanh(r(n, h)), c0=r(n, h)))
    mixed = (torch.rand(n, generator=gen) < 0.4).to(torch.uint8)
    if n > 1:
        mixed[0], mixed[-1] = 1, 0
    dones = [None, torch.zeros(n, dtype=torch.uint8), mixed, torch.ones(n, dtype=torch.uint8)]
    return nets, [d if d is None else d.to(dev) for d in dones], mixed.flip(0).contiguous().to(dev)


def run_chain(n, h, nets, dones, last_dones):
    """STEPS launches of lt_memory_step through ping-pong buffers + lt_memory_finish; every output starts as NaN."""
    import torch
    from locotouch_amd import _abi

    dev = "cuda:0"
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    stream = _abi.stream(torch.device(dev))
    out = [dict(saved_h=nan(STEPS, 1, n, h), saved_c=nan(STEPS, 1, n, h), raw_h=[], raw_c=[], fin_h=nan(1, n, h), fin_c=nan(1, n, h))
           for _ in nets]
    src = [(p["h0"], p["c0"]) for p in nets]
    for t in range(STEPS):
        dst = [(nan(n, h), nan(n, h)) for _ in nets]  # fresh buffers: the ping-pong rule (never the ones being read) holds trivially
        structs = [_abi.LtMemoryNet(p["x"][t].data_ptr(), p["I"], p["w_ih"].data_ptr(), p["w_hh"].data_ptr(), p["b_ih"].data_ptr(),
                                    p["b_hh"].data_ptr(), s[0].data_ptr(), s[1].data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                                    o["saved_h"][t].data_ptr(), o["saved_c"][t].data_ptr())
                   for p, s, d, o in zip(nets, src, dst, out)]
        _abi.call("lt_memory_step", structs[0], structs[1], dones[t], n, h, stream)
        for o, d in zip(out, dst):
            o["raw_h"].append(d[0])
            o["raw_c"].append(d[1])
        src = dst
    _abi.call("lt_memory_finish", src[0][0], src[0][1], src[1][0], src[1][1], last_dones, n, h, out[0]["fin_h"], out[0]["fin_c"],
              out[1]["fin_h"], out[1]["fin_c"], stream)
    torch.cuda.synchronize()
    return out


def eager_step(p, x, h, c):
    """What the parent's rollout runs per memory and step: the library GEMM for the input gates, then lt_lstm_forward with L = 1."""
    import torch
    from locotouch_amd import _abi

    n, hid = h.shape
    ig = (x @ p["w_ih"].t()).contiguous()
    out, cell, ws = torch.empty(1, n, hid, device=x.device), torch.empty(1, n, hid, device=x.device), torch.empty(1, n, 4 * hid, device=x.device)
    _abi.call("lt_lstm_forward", ig, h.contiguous(), c.contiguous(), p["w_hh"], p["b_ih"], p["b_hh"], 1, n, hid, out, cell, ws,
              _abi.stream(x.device))
    return out[0], cell[0]


@pytest.mark.parametrize("n, i, h", SHAPES, ids=lambda v: str(v))
def test_step_chain_matches_float64_cell_as_closely_as_the_eager_composition(n, i, h):
    import torch

    nets, dones, last_dones = make_case(n, i, h, seed=100 + n)
    out = run_chain(n, h, nets, dones, last_dones)
    err_kernel = err_eager = 0.0
    for name, p, o in zip(("actor", "critic"), nets, out):
        state = (p["h0"], p["c0"])  # the RAW f32 state the kernel's step t reads: the inputs of every reference below
        for t in range(STEPS):
            keep = torch.ones(n, 1, device="cuda:0", dtype=torch.bool) if dones[t] is None else (dones[t] == 0).unsqueeze(1)
            hm, cm = (torch.where(keep, s, torch.zeros_like(s)) for s in state)
            # the slot holds the masked pre-step state, every element of it, exactly (a copy)
            assert torch.equal(o["saved_h"][t, 0], hm) and torch.equal(o["saved_c"][t, 0], cm), (name, t)
            h64, c64 = cell64(p["x"][t], hm, cm, p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"])
            he, ce = eager_step(p, p["x"][t], hm, cm)
            kh, kc = o["raw_h"][t], o["raw_c"][t]
            assert not torch.isnan(kh).any() and not torch.isnan(kc).any(), (name, t, "an element of the new state was not written")
            err_kernel = max(err_kernel, float((kh.double() - h64).abs().max()), float((kc.double() - c64).abs().max()))
            err_eager = max(err_eager, float((he.double() - h64).abs().max()), float((ce.double() - c64).abs().max()))
            state = (kh, kc)
        keep = (last_dones == 0).unsqueeze(1)
        for fin, s in ((o["fin_h"], state[0]), (o["fin_c"], state[1])):
            assert torch.equal(fin[0], torch.where(keep, s, torch.zeros_like(s))), name
    print(f"\nlt_memory_step N={n} I={i}/{i + 7} H={h}: max |err| vs f64  kernel {err_kernel:.3e}  eager composition {err_eager:.3e}")
    assert err_eager > 0.0
    assert err_kernel <= 2.0 * err_eager, (err_kernel, err_eager)


@pytest.mark.parametrize("n, i, h", SHAPES, ids=lambda v: str(v))
def test_two_runs_give_the_same_bits(n, i, h):
    import torch

    nets, dones, last_dones = make_case(n, i, h, seed=7)
    a, b = run_chain(n, h, nets, dones, last_dones), run_chain(n, h, nets, dones, last_dones)
    for oa, ob in zip(a, b):
        for key in ("saved_h", "saved_c", "fin_h", "fin_c"):
            assert torch.equal(oa[key], ob[key]), key
        for key in ("raw_h", "raw_c"):
            assert all(torch.equal(x, y) for x, y in zip(oa[key], ob[key])), key
