"""rl/lstm.py against nn.LSTM (same parameters): outputs, both final states and every gradient; the call sites in `Memory` and
`PolicyMemory`.  The GPU tests force `use_hip_kernels` on, so they do not depend on its default."""
import copy

import pytest
import torch
import torch.nn as nn

import locotouch_amd.rl.lstm as LS
from locotouch_amd.rl.lstm import lstm_sequence

NAMES = ["out", "h_n", "c_n", "dx", "dh0", "dc0", "dW_ih", "dW_hh", "db_ih", "db_hh"]


@pytest.fixture
def hip_on():
    old, LS.use_hip_kernels = LS.use_hip_kernels, True
    yield
    LS.use_hip_kernels = old


@pytest.fixture
def hip_calls(monkeypatch, hip_on):
    """Counts the applications of the HIP `Function` (the switch is on)."""
    calls, real = [], LS._LSTMSequenceHip.apply
    monkeypatch.setattr(LS._LSTMSequenceHip, "apply", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def _problem(device, L, B, I, H, seed=0):
    torch.manual_seed(seed)
    lstm = nn.LSTM(I, H).to(device)
    x = torch.randn(L, B, I, device=device)
    h0, c0 = 0.3 * torch.randn(1, B, H, device=device), 0.3 * torch.randn(1, B, H, device=device)
    g = [torch.randn(L, B, H, device=device), torch.randn(1, B, H, device=device), torch.randn(1, B, H, device=device)]
    return lstm, x, h0, c0, g


def _run(lstm, fn, x, h0, c0, g, states=True):
    """[out, h_n, c_n, dx, dh0, dc0, dW_ih, dW_hh, db_ih, db_hh] of `fn` under a loss over out, h_n and c_n (`states` False: out only)."""
    lstm.zero_grad()
    xa, ha, ca = (t.clone().requires_grad_(True) for t in (x, h0, c0))
    out, (hn, cn) = fn(xa, (ha, ca))
    loss = (out * g[0]).sum()
    if states:
        loss = loss + (hn * g[1]).sum() + (cn * g[2]).sum()
    loss.backward()
    return [out.detach(), hn.detach(), cn.detach(), xa.grad, ha.grad, ca.grad] + [p.grad.clone() for p in lstm.parameters()], out.grad_fn


def _close(res_a, res_b, tol):
    for n, a, b in zip(NAMES, res_a, res_b, strict=True):
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= tol * max(scale, 1.0), (n, float((a - b).abs().max()), scale)


def _check(device, L, B, I, H, tol, states=True, function=None):
    lstm, x, h0, c0, g = _problem(device, L, B, I, H)
    ref, _ = _run(lstm, lambda a, hc: lstm(a, hc), x, h0, c0, g, states)
    got, grad_fn = _run(lstm, lambda a, hc: lstm_sequence(lstm, a, hc), x, h0, c0, g, states)
    if function is not None:
        assert type(grad_fn).__name__ == function.__name__ + "Backward", grad_fn
    _close(ref, got, tol)
    return lstm, x, h0, c0, g, ref, got


def test_lstm_sequence_matches_nn_lstm_cpu():
    _check("cpu", 9, 5, 7, 12, 2e-5, function=LS._LSTMSequence)
    _check("cpu", 40, 3, 64, 32, 5e-5, function=LS._LSTMSequence)


def test_lstm_sequence_with_a_loss_over_out_only_cpu():
    """Neither final state enters the loss: both carries reach backward as None."""
    _check("cpu", 9, 5, 7, 12, 2e-5, states=False)
    lstm, x, _, _, g = _problem("cpu", 9, 5, 7, 12)
    out, (hn, cn) = lstm_sequence(lstm, x)  # no initial state: zeros
    ref, (rh, rc) = lstm(x)
    assert torch.allclose(out, ref, atol=2e-5) and torch.allclose(hn, rh, atol=2e-5) and torch.allclose(cn, rc, atol=2e-5)
    (hn * g[1]).sum().backward()  # ... and a loss over h_n only: `dout` is the one that is None
    got = [p.grad.clone() for p in lstm.parameters()]
    lstm.zero_grad()
    (rh * g[1]).sum().backward()
    for a, p in zip(got, lstm.parameters()):
        assert float((a - p.grad).abs().max()) <= 2e-5 * max(float(p.grad.abs().max()), 1.0)


def _f64_errors(lstm, x, h0, c0, g, states, results):
    """Per quantity, max |result - float64 nn.LSTM on the CPU| / max(scale, 1) for each of `results`."""
    l64 = copy.deepcopy(lstm).double().cpu()
    ref, _ = _run(l64, lambda a, hc: l64(a, hc), x.double().cpu(), h0.double().cpu(), c0.double().cpu(), [t.double().cpu() for t in g], states)
    return [{n: float((r.double().cpu() - e).abs().max()) / max(float(e.abs().max()), 1.0) for n, r, e in zip(NAMES, res, ref, strict=True)}
            for res in results]


RAGGED = [(1, 3, 8, 256), (2, 16, 8, 512), (7, 1, 5, 64), (20, 37, 64, 512), (33, 101, 64, 128), (3, 200, 16, 192)]


@pytest.mark.gpu
@pytest.mark.parametrize("L,B,I,H", RAGGED)
def test_hip_lstm_kernels_on_ragged_shapes(L, B, I, H, hip_on):
    """Row counts that are not multiples of the 16-row tile, a single row, every compile-time hidden size and the generic form (192), and
    the one- and two-step sequences where the backward recursion opens and closes at once (lt_seq_step_bwd_open ->
    lt_seq_step_bwd_fused, csrc/lt_seq_tile.h).  Bound: 2e-4 of max(scale, 1) against nn.LSTM on the GPU, the bound of tests/test_rl_gru.py for the same
    kernel plan on the same shapes.  The errors of both forms against a float64 nn.LSTM on the CPU are printed (DESIGN.md section 4
    records them)."""
    lstm, x, h0, c0, g, ref, got = _check("cuda:0", L, B, I, H, 2e-4, function=LS._LSTMSequenceHip)
    e_ref, e_hip = _f64_errors(lstm, x, h0, c0, g, True, [ref, got])
    print(f"\nF64ERR shape=({L},{B},{I},{H}) worst nn.LSTM={max(e_ref.values()):.3e} hip={max(e_hip.values()):.3e} | "
          + " ".join(f"{n}:{e_ref[n]:.1e}/{e_hip[n]:.1e}" for n in NAMES))


@pytest.mark.gpu
def test_hip_lstm_with_a_loss_over_out_only(hip_on):
    """dhn and dcn reach lt_lstm_backward as NULL."""
    _check("cuda:0", 7, 37, 16, 128, 2e-4, states=False, function=LS._LSTMSequenceHip)


@pytest.mark.gpu
def test_hip_lstm_gives_the_same_bits_twice(hip_on):
    lstm, x, h0, c0, g = _problem("cuda:0", 20, 37, 64, 512)
    a, fn_a = _run(lstm, lambda v, hc: lstm_sequence(lstm, v, hc), x, h0, c0, g)
    b, _ = _run(lstm, lambda v, hc: lstm_sequence(lstm, v, hc), x, h0, c0, g)
    assert type(fn_a).__name__ == "_LSTMSequenceHipBackward"
    for n, u, v in zip(NAMES, a, b, strict=True):
        assert torch.equal(u, v), n


@pytest.mark.gpu
def test_hidden_sizes_the_kernels_do_not_cover_take_the_torch_loop(hip_on):
    _check("cuda:0", 6, 9, 8, 48, 2e-4, function=LS._LSTMSequence)  # H = 48: not a multiple of 64 -> PyTorch-op time loop


@pytest.mark.gpu
def test_memory_steps_and_sequences_through_the_hip_form(hip_calls):
    """`Memory("lstm")`: 6 single steps at 37 rows with `reset(dones)` between them against nn.LSTM driven step by step with the same
    masking of (h, c); the same trajectory without resets as ONE [6, 37, 64] call."""
    from locotouch_amd.rl.models import Memory

    torch.manual_seed(3)
    dev = "cuda:0"
    mem = Memory("lstm", 64, 128, 1).to(dev)
    x = torch.randn(6, 37, 64, device=dev)
    dones = (torch.rand(6, 37, device=dev) < 0.3).long()
    assert int(dones.sum()) > 0

    def close(a, b):
        assert float((a - b).abs().max()) <= 2e-4 * max(float(b.abs().max()), 1.0)

    with torch.no_grad():
        for resets in (True, False):
            mem.reset()
            hc, outs = None, []
            for t in range(6):
                y = mem(x[t])
                ref, hc = mem.rnn(x[t].unsqueeze(0), hc)
                close(y, ref[0])
                close(mem.hidden_states[0], hc[0])
                close(mem.hidden_states[1], hc[1])
                outs.append(y)
                if resets:
                    mem.reset(dones[t])
                    keep = (dones[t] == 0).float()[None, :, None]
                    hc = (hc[0] * keep, hc[1] * keep)
                    assert float(mem.hidden_states[1][0][dones[t] != 0].abs().max()) == 0.0
        assert len(hip_calls) == 12
        close(mem(x), torch.stack(outs))  # no resets occurred in the second pass
        close(mem(x), mem.rnn(x)[0])
        assert len(hip_calls) == 14
        mem.use_miopen_sequence = True
        mem(x)
        assert len(hip_calls) == 14


@pytest.mark.gpu
def test_policy_memory_batch_and_inference_modes_through_the_hip_form(hip_calls):
    """`PolicyMemory(type="lstm")` in batch mode on padded trajectories of lengths {5, 3, 1} cut from a 5-step rollout of 3 envs, from
    saved first hidden states: outputs and parameter gradients against `self.rnn` followed by `unpad_trajectories`; inference mode
    against `self.rnn` step by step."""
    from locotouch_amd.rl.modules import PolicyMemory
    from locotouch_amd.rl.trajectories import split_and_pad_trajectories, unpad_trajectories

    torch.manual_seed(4)
    dev = "cuda:0"
    pm = PolicyMemory(11, type="lstm", hidden_size=64).to(dev)
    obs = torch.randn(5, 3, 11, device=dev)
    dones = torch.zeros(5, 3, dtype=torch.bool, device=dev)
    dones[2, 1] = dones[3, 1] = dones[0, 2] = dones[3, 2] = True  # pieces, env-major: 5 | 3, 1, 1 | 1, 3, 1
    padded, masks = split_and_pad_trajectories(obs, dones)
    assert masks.sum(0).tolist() == [5, 3, 1, 1, 1, 3, 1]
    hs = (0.3 * torch.randn(1, 7, 64, device=dev), 0.3 * torch.randn(1, 7, 64, device=dev))
    g = torch.randn(5, 3, 64, device=dev)

    pm.zero_grad()
    got = pm(padded, masks, hs)
    assert len(hip_calls) == 1 and got.shape == (5, 3, 64)
    (got * g).sum().backward()
    got = got.detach()
    got_grads = [p.grad.clone() for p in pm.parameters()]
    pm.zero_grad()
    ref = unpad_trajectories(pm.rnn(padded, hs)[0], masks)
    (ref * g).sum().backward()
    ref = ref.detach()
    assert float((got - ref).abs().max()) <= 2e-4 * max(float(ref.abs().max()), 1.0)
    for a, p in zip(got_grads, pm.parameters(), strict=True):
        assert float((a - p.grad).abs().max()) <= 2e-4 * max(float(p.grad.abs().max()), 1.0)

    with torch.no_grad():
        hc = None
        for t in range(3):
            y = pm(obs[t])
            r, hc = pm.rnn(obs[t].unsqueeze(0), hc)
            assert y.shape == r.shape and float((y - r).abs().max()) <= 2e-4
            pm.reset(dones[t].long())
            keep = (~dones[t]).float()[None, :, None]
            hc = (hc[0] * keep, hc[1] * keep)
    assert len(hip_calls) == 4
