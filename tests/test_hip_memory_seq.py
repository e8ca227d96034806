"""The sequence kernels of both memory cells through rl/memory_seq.py, beside the float64 PyTorch-op form on the CPU: csrc/lt_memory.hip
`lt_memory_seq_forward` / `lt_memory_seq_backward` (include/lt_memory_seq.h) and csrc/lt_memory_gru.hip `lt_memory_gru_seq_forward` /
`lt_memory_gru_seq_backward` (include/lt_memory_gru.h).  The bound is the project's rule (tests/test_hip_memory_step.py): per shape, the
HIP form's largest error against float64, relative to max(scale, 1), is at most 2 x that of the existing eager composition on the same
inputs - padded trajectories through `PolicyMemory` (`lstm_sequence`, csrc/lt_lstm.hip; for the GRU `nn.GRU`), f32, on the GPU; the margin
of 2 covers a different but fixed summation order."""
import pytest

pytestmark = pytest.mark.gpu

# (T, E, I actor, H); the critic reads I + 7 columns.  17 rows: a ragged 16-row tile and rows that are not 16-byte aligned in x
# (I = 270); H = 512 with I = 150: the forward kernel's UT = 8 panel; T = 1: the backward pass is its opening launch alone
# The last two are the backward kernel's wider panels, per cell; the first five take 16 output units per workgroup.  UNITS pins the choice
# (it depends on the device's CU count; 256 on the MI355X): a shape must not drift to another variant unnoticed.
FIRST_FIVE = [(1, 1, 5, 64), (4, 17, 270, 128), (5, 80, 64, 256), (3, 48, 33, 512), (3, 20, 150, 512)]
# LSTM: 32 output units per workgroup at H = 256 (E = 512: the variant of the shape the feature exists for, H = 256 with 1024 envs per
# minibatch) and 64 at H = 128 (E = 2048).
# GRU: the backward kernel's W_hh column panel is [units][3H + 8] floats of 160 KiB of LDS (K = 3H): H = 256 -> 3104 B per unit, 64 units
# (194 KiB) do not fit, 32 (97 KiB) do; H = 128 -> 1568 B per unit, 64 units are 98 KiB.  A wider panel is taken only where the grid
# still has half a workgroup per CU (256 CUs on the MI355X): H = 256 with 32 units is 2 x 8 unit tiles, so 8 row blocks of 64 rows (E
# = 500, not a multiple of 16); H = 128 with 64 units is 2 x 2 unit tiles, so 32 row blocks (E = 2040, not a multiple of 16).
SHAPES = {"lstm": FIRST_FIVE + [(2, 512, 24, 256), (2, 2048, 24, 128)], "gru": FIRST_FIVE + [(2, 500, 24, 256), (2, 2040, 24, 128)]}
UNITS = {"lstm": {(1, 64): 16, (17, 128): 16, (80, 256): 16, (48, 512): 16, (20, 512): 16, (512, 256): 32, (2048, 128): 64},
         "gru": {(1, 64): 16, (17, 128): 16, (80, 256): 16, (48, 512): 16, (20, 512): 16, (500, 256): 32, (2040, 128): 64}}
# the recorded arrays held to float64 beside `out` and `h_prev`: the LSTM's cell states, the four planes of the GRU's `gates`
RECORDED = {"lstm": ("cell", "c_prev"), "gru": ("r", "z", "n", "hn")}
# ids: the shape, and `gru-` in front of a GRU case
CASES = [pytest.param(kind, *shape, id=("" if kind == "lstm" else "gru-") + "-".join(map(str, shape))) for kind in SHAPES for shape in SHAPES[kind]]
PATTERNS = ("none", "zero", "mixed", "one")
GRADS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
_cache = {}


def the_cell(kind):
    from locotouch_amd.rl import memory_seq

    return {"lstm": memory_seq.LSTM, "gru": memory_seq.GRU}[kind]


def planes(kind, rec):
    """The recorded arrays of one network by the names of RECORDED."""
    if kind == "lstm":
        return {q: rec[q] for q in RECORDED[kind]}
    return dict(zip(RECORDED[kind], rec["gates"].split(rec["out"].shape[2], dim=2)))


def make_case(kind, T, E, I, H):
    """Inputs on the CPU in f32 (shared by every test of a shape, never modified): x as a block [:, e0:e1] of a wider storage.  `state`:
    per network, the cell's initial state tensors (h0 first)."""
    import torch
    from locotouch_amd.rl.modules import PolicyMemory

    key = (kind, T, E, I, H)
    if key in _cache:
        return _cache[key]
    gen = torch.Generator().manual_seed(1000 + 7 * T + E + H)
    torch.manual_seed(17 + H + E)
    e0, wide = 3, E + 5
    case = dict(kind=kind, e0=e0, mems=[PolicyMemory(w, type=kind, hidden_size=H) for w in (I, I + 7)],
                x=[torch.randn(T, wide, w, generator=gen) for w in (I, I + 7)])
    h0 = [torch.tanh(torch.randn(E, H, generator=gen)) for _ in range(2)]
    c0 = [torch.randn(E, H, generator=gen) for _ in range(2)] if kind == "lstm" else None  # (the draws keep the order they had per cell)
    case["state"] = [(h0[k],) if c0 is None else (h0[k], c0[k]) for k in range(2)]
    case["dout"] = [torch.randn(T, E, H, generator=gen) for _ in range(2)]
    if kind == "gru":
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

    import torch
    from locotouch_amd.rl import memory_seq

    key = ("ref", pattern)
    if key in case:
        return case[key]
    e0, cell = case["e0"], the_cell(case["kind"])
    mems = [copy.deepcopy(m).double() for m in case["mems"]]
    d = case["dones"][pattern]
    d = None if d is None else d[:, e0:e0 + E]
    params = [p.detach() for m in mems for p in memory_seq._params(m)]  # (the op form's loops run outside autograd here)
    x = [v[:, e0:e0 + E].double() for v in case["x"]]
    done_rows = None if d is None else (d != 0).unsqueeze(-1)
    res = {}
    for k in range(2):
        rec = dict(zip((q for q, _ in cell.record), cell.forward_ops(x[k], done_rows, *(s.double() for s in case["state"][k]), *params[4 * k:4 * k + 4])))
        dgs = cell.backward_ops(case["dout"][k].double(), done_rows, params[4 * k + 1], *(rec[q] for q in cell.reads))
        grads = memory_seq._finish(cell, x[k], dict(zip((q for q, _ in cell.dgates), dgs)), rec["h_prev"])
        res[k] = dict(out=rec["out"], h_prev=rec["h_prev"], **planes(case["kind"], rec), **dict(zip(GRADS, grads)))
    case[key] = res
    return res


def run_hip(case, pattern, E, dev="cuda:0"):
    import copy

    import torch
    from locotouch_amd.rl import memory_seq

    e0, kind = case["e0"], case["kind"]
    gru = kind == "gru"
    mems = [copy.deepcopy(m).to(dev) for m in case["mems"]]
    d = case["dones"][pattern]
    d = None if d is None else d.to(dev)[:, e0:e0 + E]  # a view: the step stride of the wider tensor
    x = [v.to(dev)[:, e0:e0 + E] for v in case["x"]]
    assert x[0].stride(0) > E * x[0].shape[2] and memory_seq.serves(mems[0], mems[1], x[0], gru_memories=gru)  # read in place, through the step stride
    if gru:
        assert not memory_seq.serves(mems[0], mems[1], x[0])  # the key is what opens the path
    hc = [tuple(s.to(dev) for s in case["state"][k]) for k in range(2)]
    params = [p for m in mems for p in memory_seq._params(m)]
    recs = memory_seq.hip_forward(the_cell(kind), x[0], x[1], d, hc[0] + hc[1], params)  # the forward record itself
    # the public function, with autograd (a GRU's state as the bare tensor)
    outs = memory_seq.memory_rollout_sequence(mems[0], mems[1], x[0], x[1], d, *((hc[0][0], hc[1][0]) if gru else hc), gru_memories=gru)
    (outs[0] * case["dout"][0].to(dev)).sum().add((outs[1] * case["dout"][1].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    res = {}
    for k in range(2):
        assert torch.equal(outs[k], recs[k]["out"])
        res[k] = dict(out=recs[k]["out"], h_prev=recs[k]["h_prev"], **planes(kind, recs[k]), **{g: getattr(mems[k].rnn, g).grad for g in GRADS})
    return res, d


def run_eager(case, pattern, E, dev="cuda:0"):
    """The existing composition: padded trajectories from their saved first states through `PolicyMemory` (batch mode; a GRU memory's
    is nn.GRU), f32, GPU."""
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
        hid = []
        for s0 in case["state"][k]:
            saved = torch.zeros(T, E, s0.shape[1], device=dev)  # `reset(dones)`: zeros behind every done
            saved[0] = s0.to(dev)
            hid.append(saved.permute(1, 0, 2)[starts.t()].unsqueeze(0).contiguous())
        out = mem(padded, masks, tuple(hid) if len(hid) > 1 else hid[0])
        (out * case["dout"][k].to(dev)).sum().backward()
        res[k] = dict(out=out.detach(), **{g: getattr(mem.rnn, g).grad for g in GRADS})
    torch.cuda.synchronize()
    return res


def rel_err(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1.0)


@pytest.mark.parametrize("kind, T, E, I, H", CASES)
def test_forward_and_gradients_match_float64_as_closely_as_the_eager_composition(kind, T, E, I, H):
    import torch

    from locotouch_amd import _abi

    assert getattr(_abi.load(), the_cell(kind).backward_units)(E, H) == UNITS[kind][(E, H)]  # the backward kernel variant this shape is here for
    case = make_case(kind, T, E, I, H)
    name = the_cell(kind).seq_forward[:-len("_forward")]
    err_hip = err_eager = 0.0
    for pattern in PATTERNS:
        ref = reference64(case, pattern, E)
        hip, d = run_hip(case, pattern, E)
        eager = run_eager(case, pattern, E)
        worst, worst_eager = {}, {}
        for k in range(2):
            # the masked pre-step state: exact zeros at masked rows, exact copies of the previous step's out (and cell) elsewhere
            for prev, new, first in zip(("h_prev", "c_prev"), ("out", "cell"), case["state"][k]):
                assert torch.equal(hip[k][prev][0], first.to("cuda:0")), (pattern, k, prev)
                for t in range(1, T):
                    keep = torch.ones(E, 1, dtype=torch.bool, device="cuda:0") if d is None else (d[t - 1] == 0).unsqueeze(1)
                    assert torch.equal(hip[k][prev][t], torch.where(keep, hip[k][new][t - 1], torch.zeros_like(hip[k][new][t - 1]))), (pattern, k, prev, t)
                    if d is not None and bool((~keep).any()):
                        assert torch.count_nonzero(hip[k][prev][t][~keep[:, 0]]) == 0
            for q, r in ref[k].items():
                assert not torch.isnan(hip[k][q]).any(), (pattern, k, q, "an element was not written")
                e = rel_err(hip[k][q], r)
                worst[q] = max(worst.get(q, 0.0), e)
                err_hip = max(err_hip, e)
                if q in eager[k]:
                    ee = rel_err(eager[k][q], r)
                    worst_eager[q] = max(worst_eager.get(q, 0.0), ee)
                    err_eager = max(err_eager, ee)
        print(f"\n{name} T={T} E={E} I={I}/{I + 7} H={H} dones={pattern}: HIP " + " ".join(f"{q} {e:.2e}" for q, e in worst.items())
              + " | eager " + " ".join(f"{q} {e:.2e}" for q, e in worst_eager.items()))
    print(f"{name} T={T} E={E} I={I}/{I + 7} H={H}: max rel err vs f64  HIP form {err_hip:.3e}  eager composition {err_eager:.3e}")
    assert err_eager > 0.0
    assert err_hip <= 2.0 * err_eager, (err_hip, err_eager)


@pytest.mark.parametrize("kind, T, E, I, H", CASES)
def test_two_runs_give_the_same_bits(kind, T, E, I, H):
    import torch

    case = make_case(kind, T, E, I, H)
    a, _ = run_hip(case, "mixed", E)
    b, _ = run_hip(case, "mixed", E)
    for k in range(2):
        for q in a[k]:
            assert torch.equal(a[k][q], b[k][q]), (k, q)
