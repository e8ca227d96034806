"""lt_memory_input_grad (include/lt_memory_dx.h, csrc/lt_memory_dx.hip) on the device: dx = dg W_ih held to float64 by the project's
bound (tests/test_hip_rnn_encoder_backward.py `held_to_float64`), written in place between guard words, with bits that depend on the
row and on W_ih alone - and what stands on it in rl/memory_seq.py: `memory_rollout_sequence` on rows that require a gradient,
`direct_backward(dx_out=...)`, and a layer in front of the memories that now trains.  The CPU counterparts are
tests/test_memory_dx_abi.py and tests/test_memory_seq_input_grad_cpu.py."""
import functools

import pytest

pytestmark = pytest.mark.gpu

PAD = 3  # dx_stride = I + PAD: one padding column in front of a row's I floats (so dx is 4-byte aligned only), two behind


@functools.lru_cache(maxsize=None)
def operands(gates, H, I, seed):
    """(dg [70][K], W_ih [K][I] as a 4-byte aligned view of a flat bucket, the float64 product, the f32 torch product) - made once per
    shape, shared by every test, never written."""
    import torch

    from tests.guarded import DEV

    K = gates * H
    g = torch.Generator().manual_seed(1000 * seed + 7 * K + I)
    dg = torch.randn(70, K, generator=g).to(DEV)
    bucket = torch.randn(K * I + 5, generator=g).mul_(I ** -0.5).to(DEV)
    w = bucket[1:1 + K * I].view(K, I)
    assert w.data_ptr() % 16 == 4
    return dg, w, dg.double() @ w.double(), dg @ w


def launch(nets, n, H, gates):
    """One launch for one or two networks, each (dg [n][K], w [K][I]).  Every dx is a strided view in a guarded, NaN-filled buffer
    [n][I + PAD]: checks that every element of the I columns was written and no padding column or guard word was -> the dx views."""
    import torch

    from locotouch_amd import _abi
    from tests.guarded import NAN_BITS, guard_problem, guarded

    structs, held_bufs = [], []
    for dg, w in nets:
        I = w.shape[1]
        assert dg.shape == (n, gates * H) and dg.is_contiguous() and w.is_contiguous()
        buf, view = guarded((n, I + PAD))
        dx = view[:, 1:1 + I]
        structs.append(_abi.LtMemoryDxNet(dg=dg.data_ptr(), w_ih=w.data_ptr(), I=I, dx=dx.data_ptr(), dx_stride=I + PAD))
        held_bufs.append((buf, view, dx))
    assert _abi.load().lt_memory_input_grad_launches(structs[0], structs[1] if len(structs) > 1 else None, n, H, gates) == 1
    _abi.call("lt_memory_input_grad", structs[0], structs[1] if len(structs) > 1 else None, n, H, gates, _abi.stream(torch.device("cuda:0")))
    torch.cuda.synchronize()
    outs = []
    for k, (buf, view, dx) in enumerate(held_bufs):
        I = dx.shape[1]
        assert guard_problem(f"dx[{k}]", buf, view) is None
        bits = view.view(torch.int32)
        assert bool((bits[:, 0] == NAN_BITS).all()) and bool((bits[:, 1 + I:] == NAN_BITS).all()), f"a padding column of dx[{k}] was written"
        assert not bool(torch.isnan(dx).any()), f"an element of dx[{k}] was left unwritten"
        outs.append(dx)
    return outs


def check(tag, gates, H, I_a, I_c, n):
    from tests.memory_dx_ref import held

    ops = [operands(gates, H, I_a, 1), operands(gates, H, I_c, 2)]
    outs = launch([(dg[:n], w) for dg, w, _, _ in ops], n, H, gates)
    for k, (dx, (_, _, ref, chain)) in enumerate(zip(outs, ops)):
        held(f"{tag} gates={gates} H={H} I={dx.shape[1]} n={n} net {k}", dx, ref[:n], chain[:n])
    return outs


# ---- a. held to float64 ----
@pytest.mark.parametrize("I", [1, 5, 24, 64, 100])
@pytest.mark.parametrize("gates", [3, 4])
def test_held_to_float64(gates, I):
    """K = 192 and 256; every n in {1, 17, 70}; the critic of each launch has another width than the actor (the widths, rotated)."""
    other = {1: 100, 5: 1, 24: 5, 64: 24, 100: 64}[I]
    for n in (1, 17, 70):
        check("kernel", gates, 64, I, other, n)


def test_held_to_float64_on_the_narrow_panel():
    """K = 2048: 16 columns of W_ih fill the LDS, I = 64 takes four column tiles."""
    check("narrow panel", 4, 512, 64, 24, 70)


def test_widest_row():
    """I = 512, the limit, at the GRU's K = 768 (32-column panels, 16 column tiles) beside a one-column critic."""
    check("widest", 3, 256, 512, 1, 17)


# ---- b. bits ----
def test_bits_depend_on_the_row_and_the_weight_alone():
    import torch

    gates, H, I_a, I_c = 4, 64, 24, 100
    first = check("bits", gates, H, I_a, I_c, 70)
    again = check("bits", gates, H, I_a, I_c, 70)
    for k in (0, 1):
        assert torch.equal(first[k], again[k]), f"net {k}: a second run differs"
    part = check("bits", gates, H, I_a, I_c, 37)
    for k in (0, 1):
        assert torch.equal(part[k], first[k][:37]), f"net {k}: the rows n = 37 and n = 70 share differ"
    dg, w, _, _ = operands(gates, H, I_a, 1)
    alone, = launch([(dg, w)], 70, H, gates)
    assert torch.equal(alone, first[0]), "the actor's rows differ without a critic"
    dg_c, w_c, _, _ = operands(gates, H, I_c, 2)
    swapped = launch([(dg_c, w_c), (dg, w)], 70, H, gates)  # the networks in the other order: other column tiles per grid slot
    assert torch.equal(swapped[1], first[0]) and torch.equal(swapped[0], first[1])


@pytest.mark.parametrize("gates, H, I", [(4, 64, 64), (3, 64, 24), (4, 256, 40)])
def test_a_rows_bits_do_not_depend_on_its_place_or_the_tile_shapes(gates, H, I):
    """n = 10 007: the 70 rows repeated.  More than one row block, row blocks that end inside a 16-row sub-tile, and - with enough rows to
    cover the chip - a wider column panel than n = 70 takes."""
    import torch

    n = 10007
    ops = [operands(gates, H, I, 1), operands(gates, H, 5, 2)]
    small = launch([(dg, w) for dg, w, _, _ in ops], 70, H, gates)
    idx = torch.arange(n, device=small[0].device) % 70
    big = launch([(dg[idx].contiguous(), w) for dg, w, _, _ in ops], n, H, gates)
    for k in (0, 1):
        assert torch.equal(big[k], small[k][idx]), f"net {k}"


# ---- c. through autograd ----
@functools.lru_cache(maxsize=None)
def case_and_loop(kind, T, E, I_a, I_c, H, x_width=None):
    import torch

    from tests.memory_dx_ref import Case

    c = Case(kind, T, E, I_a, I_c, H, seed=3, x_width=x_width)
    return c, (c.loop(torch.float64) if x_width is None else None)


def ops_form(monkeypatch, fn):
    """`fn()` with `memory_rollout_sequence` on its PyTorch-op time loop"""
    from locotouch_amd.rl import memory_seq

    with monkeypatch.context() as m:
        m.setattr(memory_seq, "use_hip_kernels", False)
        return fn()


@pytest.mark.parametrize("T, E, I_a, I_c", [(5, 7, 5, 9), (3, 19, 24, 24)])
@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_row_gradients_through_autograd(monkeypatch, kind, T, E, I_a, I_c):
    import torch

    from locotouch_amd.rl import memory_seq
    from tests.guarded import DEV
    from tests.memory_dx_ref import held

    c, (ref_dx, _) = case_and_loop(kind, T, E, I_a, I_c, 64)
    mems = c.memories(torch.float32, DEV)
    assert memory_seq.serves(mems[0], mems[1], *c.rows(torch.float32, DEV, True), gru_memories=kind == "gru")
    calls = []
    real = memory_seq.input_grad
    monkeypatch.setattr(memory_seq, "input_grad", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    dx, params, _, _ = c.run(torch.float32, DEV, requires_grad=True)
    assert calls == [1]  # the HIP form, one launch
    _, plain, _, _ = c.run(torch.float32, DEV, requires_grad=False)
    assert calls == [1]  # rows that ask for nothing launch nothing
    chain, _, _, _ = ops_form(monkeypatch, lambda: c.run(torch.float32, DEV, requires_grad=True))
    assert calls == [1]
    for k, name in enumerate(("obs.grad", "critic_obs.grad")):
        assert dx[k] is not None and dx[k].shape == (T, E, (I_a, I_c)[k]) and dx[k].dtype == torch.float32
        held(f"autograd {kind} T={T} E={E} {name}", dx[k], ref_dx[k], chain[k])
    for k, (a, b) in enumerate(zip(params, plain)):
        assert torch.equal(a, b), f"parameter gradient {k} depends on whether the rows ask"
    for k in (0, 1):  # one network asking alone: the same bits
        rows = c.rows(torch.float32, DEV, False)
        rows[k].requires_grad_(True)
        one, _, _, _ = c.run(torch.float32, DEV, rows=rows)
        assert one[1 - k] is None and torch.equal(one[k], dx[k]), k


# ---- d. without the autograd Function ----
@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_direct_backward_writes_the_input_gradients_in_place(kind):
    import torch

    from locotouch_amd.rl import memory_seq
    from tests.guarded import DEV
    from tests.memory_dx_ref import held

    T, E, I_a, I_c, H = 3, 19, 24, 9, 64
    c, _ = case_and_loop(kind, T, E, I_a, I_c, H)
    cell = memory_seq.GRU if kind == "gru" else memory_seq.LSTM
    mems = c.memories(torch.float32, DEV)
    to = lambda t: t.to(device=DEV, dtype=torch.float32).contiguous()
    x = [to(v) for v in c.x]
    dones = memory_seq._dones_bytes(c.dones.to(DEV))
    hc = [tuple(to(s) for s in st) for st in c.state]
    douts = tuple(to(d) for d in c.dout)
    recs = memory_seq.direct_forward(cell, mems[0], mems[1], x[0], x[1], dones, hc[0], hc[1])

    def run(dx_out):
        grad_of = {p: torch.full_like(p, float("nan")) for m in mems for p in memory_seq._params(m)}
        memory_seq.direct_backward(cell, mems[0], mems[1], x[0], x[1], dones, recs, douts, grad_of, **({} if dx_out is None else {"dx_out": dx_out}))
        return [grad_of[p] for m in mems for p in memory_seq._params(m)]

    plain = run(None)
    wide = [torch.full((T, E, I + 4), float("nan"), device=DEV) for I in (I_a, I_c)]  # the tail columns of a wider gradient row
    with_dx = run(tuple(w[..., 4:] for w in wide))
    for k, (a, b) in enumerate(zip(with_dx, plain)):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b), f"bucket view {k}"
    dgs = memory_seq.hip_backward(cell, douts, dones, tuple(memory_seq._params(m)[1] for m in mems), recs)
    want = memory_seq.input_grad(cell, dgs, tuple(memory_seq._params(m)[0] for m in mems))
    for k, (w, ref) in enumerate(zip(wide, want)):
        assert bool(torch.isnan(w[..., :4]).all()) and torch.equal(w[..., 4:], ref), k
        d_ih, w_ih = dgs[k][cell.d_ih].view(T * E, -1), memory_seq._params(mems[k])[0].detach()
        held(f"direct {kind} net {k}", ref.view(T * E, -1), d_ih.double() @ w_ih.double(), d_ih @ w_ih)


# ---- e. the trap: a layer in front of the memories ----
@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_a_layer_in_front_of_the_memories_trains(monkeypatch, kind):
    import torch

    from tests.guarded import DEV
    from tests.memory_dx_ref import held

    T, E, H = 3, 19, 64
    c, _ = case_and_loop(kind, T, E, 24, 24, H, x_width=31)
    torch.manual_seed(11)
    front64 = torch.nn.Linear(31, 24).double()
    c.loop(torch.float64, front=front64)
    ref = front64.weight.grad
    assert ref is not None and float(ref.abs().max()) > 0

    def through_the_memories():
        front = torch.nn.Linear(31, 24).to(DEV)
        front.load_state_dict({k: v.float() for k, v in front64.state_dict().items()})
        rows = [front(x) for x in c.rows(torch.float32, DEV, False)]
        c.run(torch.float32, DEV, rows=rows)
        return front.weight.grad, front.bias.grad

    got, got_b = through_the_memories()
    chain, chain_b = ops_form(monkeypatch, through_the_memories)
    assert got is not None, "the layer in front of the memories got no gradient: it trains as if frozen"
    assert float(got.abs().max()) > 0
    held(f"front layer {kind} weight", got, ref, chain)
    held(f"front layer {kind} bias", got_b, front64.bias.grad, chain_b)
