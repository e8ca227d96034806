"""rl/gru.py against nn.GRU (same parameters): outputs, final state and every gradient."""
import pytest
import torch
import torch.nn as nn

from locotouch_amd.rl.gru import gru_sequence


NAMES = ["out", "h_n", "dx", "dh0", "dW_ih", "dW_hh", "db_ih", "db_hh"]


def _problem(device, L, B, I, H):
    torch.manual_seed(0)
    gru = nn.GRU(I, H).to(device)
    x = torch.randn(L, B, I, device=device)
    h0 = 0.3 * torch.randn(1, B, H, device=device)
    return gru, x, h0, (torch.randn(L, B, H, device=device), torch.randn(1, B, H, device=device))


def _run(gru, fn, x, h0, g):
    """[out, h_n, dx, dh0, dW_ih, dW_hh, db_ih, db_hh] of `fn` under a loss over out and h_n"""
    gru.zero_grad()
    xa, ha = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    out, hn = fn(xa, ha)
    ((out * g[0]).sum() + (hn * g[1]).sum()).backward()
    return [out.detach(), hn.detach(), xa.grad, ha.grad] + [p.grad.clone() for p in gru.parameters()]


def _check(device, L, B, I, H, tol):
    gru, x, h0, g = _problem(device, L, B, I, H)
    res = [_run(gru, fn, x, h0, g) for fn in (lambda a, b: gru(a, b), lambda a, b: gru_sequence(gru, a, b))]
    for n, a, b in zip(NAMES, *res, strict=True):
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= tol * max(scale, 1.0), (n, float((a - b).abs().max()), scale)


def test_gru_sequence_matches_nn_gru_cpu():
    _check("cpu", 9, 5, 7, 12, 2e-5)
    _check("cpu", 40, 3, 64, 32, 5e-5)


@pytest.mark.gpu
def test_gru_sequence_matches_nn_gru_on_distillation_shape():
    _check("cuda:0", 500, 48, 64, 512, 3e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("L,B,I,H", [(20, 37, 64, 512), (7, 1, 5, 64), (33, 101, 64, 128), (3, 200, 16, 192), (2, 16, 8, 512), (1, 3, 8, 256)])
def test_hip_gru_kernels_on_ragged_shapes(L, B, I, H):
    """Row counts that are not multiples of the 16-row tile, a single row, other hidden sizes (multiples of 64), and the one- and
    two-step sequences where the backward recursion opens and closes at once (lt_seq_step_bwd_open -> lt_seq_step_bwd_fused,
    csrc/lt_seq_tile.h).  The backward pass runs with a scratch buffer of [B][H]."""
    import locotouch_amd.rl.gru as G

    assert G.use_hip_kernels
    _check("cuda:0", L, B, I, H, 2e-4)


@pytest.mark.gpu
def test_hip_gru_gives_the_same_bits_twice():
    import locotouch_amd.rl.gru as G

    assert G.use_hip_kernels
    gru, x, h0, g = _problem("cuda:0", 20, 37, 64, 512)
    a = _run(gru, lambda v, h: gru_sequence(gru, v, h), x, h0, g)
    b = _run(gru, lambda v, h: gru_sequence(gru, v, h), x, h0, g)
    for n, u, v in zip(NAMES, a, b, strict=True):
        assert torch.equal(u, v), n


@pytest.mark.gpu
@pytest.mark.parametrize("L,B,H", [(3, 17, 64), (2, 17, 128)])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_null_carries_equal_zero_carries_bit_for_bit(cell, L, B, H):
    """dhn (and the LSTM's dcn) NULL against a buffer of zeros, straight through the C ABI (autograd never sends NULL for the GRU): the
    generic and a compile-time kernel form, a partial row tile, and sequences short enough that the opening and the closing launch
    meet.  Outputs start as NaN, so one that a call leaves unwritten compares unequal."""
    from locotouch_amd import _abi

    torch.manual_seed(1)
    dev, ng = "cuda:0", {"gru": 3, "lstm": 4}[cell]
    rnd = lambda *shape: torch.randn(*shape, device=dev)  # noqa: E731
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)  # noqa: E731
    ig, w_hh, b_ih, b_hh = rnd(L, B, ng * H), rnd(ng * H, H) / H ** 0.5, rnd(ng * H), rnd(ng * H)
    h0, c0, dout, zeros = 0.3 * rnd(B, H), 0.3 * rnd(B, H), rnd(L, B, H), torch.zeros(B, H, device=dev)
    out, cellseq, ws, st = nan(L, B, H), nan(L, B, H), nan(L, B, 4 * H), _abi.stream(dev)
    if cell == "gru":
        _abi.call("lt_gru_forward", ig, h0, w_hh, b_ih, b_hh, L, B, H, out, ws, st)
        carries = [(None,), (zeros,)]
    else:
        _abi.call("lt_lstm_forward", ig, h0, c0, w_hh, b_ih, b_hh, L, B, H, out, cellseq, ws, st)
        carries = [(None, None), (zeros, None), (None, zeros), (zeros, zeros)]
    results = []
    for carry in carries:
        if cell == "gru":
            res = dict(dig=nan(L, B, 3 * H), dhg=nan(L, B, 3 * H), dh0=nan(B, H))
            _abi.call("lt_gru_backward", dout, *carry, out, ws, h0, w_hh, L, B, H, res["dig"], res["dhg"], nan(B, H), res["dh0"], st)
        else:
            res = dict(dgates=nan(L, B, 4 * H), dh0=nan(B, H), dc0=nan(B, H))
            _abi.call("lt_lstm_backward", dout, *carry, out, cellseq, ws, h0, c0, w_hh, L, B, H, res["dgates"], nan(B, H), res["dh0"], res["dc0"], st)
        results.append(res)
    for carry, res in zip(carries[1:], results[1:], strict=True):
        for n in res:
            assert torch.equal(results[0][n], res[n]), (n, [c is not None for c in carry])


@pytest.mark.gpu
def test_hidden_sizes_the_kernels_do_not_cover_take_the_torch_loop():
    _check("cuda:0", 6, 9, 8, 48, 2e-4)  # H = 48: not a multiple of 64 -> PyTorch-op time loop

