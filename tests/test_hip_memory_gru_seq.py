"""csrc/lt_memory_gru.hip `lt_memory_gru_seq_forward` / `lt_memory_gru_seq_backward` (include/lt_memory_gru.h) through rl/memory_seq.py,
beside the float64 PyTorch-op form on the CPU.  The bound is the project's rule (tests/test_hip_memory_seq.py): per shape, the HIP
form's largest error against float64, relative to max(scale, 1), is at most 2 x that of the existing eager composition on the same
inputs - padded trajectories through `PolicyMemory` (`nn.GRU`), f32, on the GPU; the margin of 2 covers a different but fixed summation
order."""
import pytest

pytestmark = pytest.mark.gpu

# (T, E, I actor, H); the critic reads I + 7 columns.  17 rows: a ragged 16-row tile and rows that are not 16-byte aligned in x
# (I = 270); H = 512 with I = 150: the forward kernel's UT = 8 panel; T = 1: the backward pass is its opening launch alone.
# The backward kernel's W_hh column panel is [units][3H + 8] floats of 160 KiB of LDS (K = 3H): H = 256 -> 3104 B per unit, 64 units
# (194 KiB) do not fit, 32 (97 KiB) do; H = 128 -> 1568 B per unit, 64 units are 98 KiB.  A wider panel is taken only where the grid
# still has half a workgroup per CU (256 CUs on the MI355X): H = 256 with 32 units is 2 x 8 unit tiles, so 8 row blocks of 64 rows (E
# = 500, not a multiple of 16); H = 128 with 64 units is 2 x 2 unit tiles, so 32 row blocks (E = 2040, not a multiple of 16).  The
# first five take 16.  UNITS pins the choice: a shape must not drift to another variant unnoticed.
SHAPES = [(1, 1, 5, 64), (4, 17, 270, 128), (5, 80, 64, 256), (3, 48, 33, 512), (3, 20, 150, 512), (2, 500, 24, 256), (2, 2040, 24, 128)]
UNITS = {(1, 64): 16, (17, 128): 16, (80, 256): 16, (48, 512): 16, (20, 512): 16, (500, 256): 32, (2040, 128): 64}
PATTERNS = ("none", "zero", "mixed", "one")
GRADS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
PLANES = ("r", "z", "n", "hn")
_cache = {}


def make_case(T, E, I, H):
    """Inputs on the CPU in f32 (shared by every test of a shape, never modified): x as a block [:, e0:e1] of a wider storage."""
    import torch
    from locotouch_amd.rl.modules import PolicyMemory

    key = (T, E, I, H)
    if key in _cache:
        return _cache[key]
    gen = torch.Generator().manual_seed(1000 + 7 * T + E + H)
    torch.manual_seed(17 + H + E)
    e0, wide = 3, E + 5
    case = dict(e0=e0, mems=[PolicyMemory(w, type="gru", hidden_size=H) for w in (I, I + 7)],
                x=[torch.randn(T, wide, w, generator=gen) for w in (I, I + 7)],
                h0=[torch.tanh(torch.randn(E, H, generator=gen)) for _ in range(2)],
                dout=[torch.randn(T, E, H, generator=gen) for _ in range(2)])
    with torch.no_grad():  # biases of order 0.3: b_hn inside r * (...) is not a rounding matter
        for m in case["mems"]:
            m.rnn.bias_ih_l0.copy_(0.3 * torch.randn(3 * H, generator=gen))
            m.rnn.bias_hh_l0.copy_(0.3 * torch.randn(3 * H, generator=gen))
    mixed = torch.rand(T, wide, generator=gen) < 0.35
    mixed[0, e0], mixed[T - 1, e0] = True, True  # a done at t = 0 and one at t = T - 1 inside the block
    if E > 1:
        mixed[:, e0 + 1] = False
    case["dones"] = dict(none=None, zero=torch.zeros(T, wide, dtype=torch.uint8), mixed=mixed.to(torch.uint8), one=torch.ones(T, wide, dtype=torch.uint8))
    _cache[key] = case
    return case


def reference64(case, pattern, E):
    """float64 PyTorch-op form on the CPU, computed once per (shape, pattern)."""
    import copy

    from locotouch_amd.rl import memory_seq

    key = ("ref", pattern)
    if key in case:
        return case[key]
    e0 = case["e0"]
    mems = [copy.deepcopy(m).double() for m in case["mems"]]
    d = case["dones"][pattern]
    d = None if d is None else d[:, e0:e0 + E]
    params = [p.detach() for m in mems for p in memory_seq._params(m)]  # (the op form's loops run outside autograd here)
    x = [v[:, e0:e0 + E].double() for v in case["x"]]
    done_rows = None if d is None else (d != 0).unsqueeze(-1)
    res = {}
    for k in range(2):
        out, gates, h_prev = memory_seq._gru_forward_ops(x[k], done_rows, case["h0"][k].double(), *params[4 * k:4 * k + 4])
        dig, dhg = memory_seq._gru_backward_ops(case["dout"][k].double(), done_rows, params[4 * k + 1], gates, h_prev)
        grads = memory_seq._gru_finish(x[k], dig, dhg, h_prev)
        res[k] = dict(out=out, h_prev=h_prev, **dict(zip(PLANES, gates.split(out.shape[2], dim=2))), **dict(zip(GRADS, grads)))
    case[key] = res
    return res


def run_hip(case, pattern, E, dev="cuda:0"):
    import copy

    import torch
    from locotouch_amd.rl import memory_seq

    e0 = case["e0"]
    mems = [copy.deepcopy(m).to(dev) for m in case["mems"]]
    d = case["dones"][pattern]
    d = None if d is None else d.to(dev)[:, e0:e0 + E]  # a view: the step stride of the wider tensor
    x = [v.to(dev)[:, e0:e0 + E] for v in case["x"]]
    assert x[0].stride(0) > E * x[0].shape[2] and memory_seq.serves(mems[0], mems[1], x[0], gru_memories=True)  # read in place
    assert not memory_seq.serves(mems[0], mems[1], x[0])  # the key is what opens the path
    h0 = [case["h0"][k].to(dev) for k in range(2)]
    params = [p for m in mems for p in memory_seq._params(m)]
    recs = memory_seq.gru_hip_forward(x[0], x[1], d, h0[0], h0[1], params)  # the forward record itself
    outs = memory_seq.memory_rollout_sequence(mems[0], mems[1], x[0], x[1], d, h0[0], h0[1], gru_memories=True)  # the public function
    (outs[0] * case["dout"][0].to(dev)).sum().add((outs[1] * case["dout"][1].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    res = {}
    for k in range(2):
        assert torch.equal(outs[k], recs[k]["out"])
        H = recs[k]["out"].shape[2]
        res[k] = dict(out=recs[k]["out"], h_prev=recs[k]["h_prev"], **dict(zip(PLANES, recs[k]["gates"].split(H, dim=2))),
                      **{g: getattr(mems[k].rnn, g).grad for g in GRADS})
    return res, d


def run_eager(case, pattern, E, dev="cuda:0"):
    """The existing composition: padded trajectories from their saved first states through `PolicyMemory` (batch mode, nn.GRU), f32, GPU."""
    import copy

    import torch
    from locotouch_amd.rl.trajectories import split_and_pad_trajectories

    e0, T = case["e0"], case["dout"][0].shape[0]
    d = case["dones"][pattern]
    d = (torch.zeros(T, E, dtype=torch.uint8) if d is None else d[:, e0:e0 + E]).to(dev).unsqueeze(-1)
    starts = torch.ones(T, E, dtype=torch.bool, device=dev)
    starts[1:] = d[:-1, :, 0] != 0
    res = {}
    for k in range(2):
        mem = copy.deepcopy(case["mems"][k]).to(dev)
        x = case["x"][k].to(dev)[:, e0:e0 + E].contiguous()
        padded, masks = split_and_pad_trajectories(x, d)
        saved = torch.zeros(T, E, case["h0"][k].shape[1], device=dev)  # `reset(dones)`: zeros behind every done
        saved[0] = case["h0"][k].to(dev)
        out = mem(padded, masks, saved.permute(1, 0, 2)[starts.t()].unsqueeze(0).contiguous())
        (out * case["dout"][k].to(dev)).sum().backward()
        res[k] = dict(out=out.detach(), **{g: getattr(mem.rnn, g).grad for g in GRADS})
    torch.cuda.synchronize()
    return res


def rel_err(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1.0)


@pytest.mark.parametrize("T, E, I, H", SHAPES, ids=lambda v: str(v))
def test_forward_and_gradients_match_float64_as_closely_as_the_eager_composition(T, E, I, H):
    import torch

    from locotouch_amd import _abi

    assert _abi.load().lt_memory_gru_seq_backward_units(E, H) == UNITS[(E, H)]  # the backward kernel variant this shape is here for
    case = make_case(T, E, I, H)
    err_hip = err_eager = 0.0
    for pattern in PATTERNS:
        ref = reference64(case, pattern, E)
        hip, d = run_hip(case, pattern, E)
        eager = run_eager(case, pattern, E)
        worst, worst_eager = {}, {}
        for k in range(2):
            # the masked pre-step state: exact zeros at masked rows, exact copies of the previous step's out elsewhere
            assert torch.equal(hip[k]["h_prev"][0], case["h0"][k].to("cuda:0")), (pattern, k)
            for t in range(1, T):
                keep = torch.ones(E, 1, dtype=torch.bool, device="cuda:0") if d is None else (d[t - 1] == 0).unsqueeze(1)
                prev = hip[k]["out"][t - 1]
                assert torch.equal(hip[k]["h_prev"][t], torch.where(keep, prev, torch.zeros_like(prev))), (pattern, k, t)
                if d is not None and bool((~keep).any()):
                    assert torch.count_nonzero(hip[k]["h_prev"][t][~keep[:, 0]]) == 0
            for q, r in ref[k].items():
                assert not torch.isnan(hip[k][q]).any(), (pattern, k, q, "an element was not written")
                e = rel_err(hip[k][q], r)
                worst[q] = max(worst.get(q, 0.0), e)
                err_hip = max(err_hip, e)
                if q in eager[k]:
                    ee = rel_err(eager[k][q], r)
                    worst_eager[q] = max(worst_eager.get(q, 0.0), ee)
                    err_eager = max(err_eager, ee)
        print(f"\nlt_memory_gru_seq T={T} E={E} I={I}/{I + 7} H={H} dones={pattern}: HIP " + " ".join(f"{q} {e:.2e}" for q, e in worst.items())
              + " | eager " + " ".join(f"{q} {e:.2e}" for q, e in worst_eager.items()))
    print(f"lt_memory_gru_seq T={T} E={E} I={I}/{I + 7} H={H}: max rel err vs f64  HIP form {err_hip:.3e}  eager composition {err_eager:.3e}")
    assert err_eager > 0.0
    assert err_hip <= 2.0 * err_eager, (err_hip, err_eager)


@pytest.mark.parametrize("T, E, I, H", SHAPES, ids=lambda v: str(v))
def test_two_runs_give_the_same_bits(T, E, I, H):
    import torch

    case = make_case(T, E, I, H)
    a, _ = run_hip(case, "mixed", E)
    b, _ = run_hip(case, "mixed", E)
    for k in range(2):
        for q in a[k]:
            assert torch.equal(a[k][q], b[k][q]), (k, q)
