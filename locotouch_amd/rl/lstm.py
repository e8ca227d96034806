"""Single-layer LSTM over a padded batch of whole trajectories: the LSTM counterpart of rl/gru.py, for `Memory` and `PolicyMemory`.

The recurrence is one [B, H] x [H, 4H] GEMM and one pointwise gate formula per step; everything else is NOT sequential and is hoisted
out of the loop here, as one GEMM each:

  forward    igates = X W_ih^T for ALL steps; per step: the recurrent GEMM + the gates (i, f, g, o), c' = f c + i g, h' = o tanh(c')
  backward   per step: the gate gradients and dh_prev = dgates W_hh; after the loop dW_hh = dgates^T H_prev and dW_ih = dgates^T X
             (sums over all L * B rows, split-K), dX = dgates W_ih, db_ih = db_hh = the column sums of dgates

Unlike a GRU's, an LSTM's gate gradients are the same on the input side and on the hidden side: there is ONE `dgates` array.  Two forms
of the time loop: plain PyTorch ops (the CPU, hidden sizes the kernels do not cover, and `use_hip_kernels` off) and csrc/lt_lstm.hip
(`lt_lstm_forward` / `lt_lstm_backward`: one launch per step, issued from C).  Results equal `nn.LSTM` to fp32 rounding
(tests/test_rl_lstm.py).  Parameters are the `nn.LSTM` module's own (`weight_ih_l0`, ...): checkpoints are unaffected.
"""
from __future__ import annotations

import torch

from .gru import _wgrad


def _finish_backward(ctx, x, h0, w_ih, out, dgates, dh0, dc0):
    """Everything of the backward pass that is not sequential: one GEMM each."""
    L, B, _ = x.shape
    H = out.shape[2]
    dg2 = dgates.view(L * B, 4 * H)
    h_prev = torch.cat([h0.unsqueeze(0), out[:-1]], dim=0).view(L * B, H)
    dw_hh = _wgrad(dg2, h_prev)
    dw_ih = _wgrad(dg2, x.reshape(L * B, -1))
    dx = (dg2 @ w_ih).view_as(x) if ctx.needs_input_grad[0] else None
    db = dg2.sum(0)
    return dx, dh0, dc0, dw_ih, dw_hh, db, db.clone()


class _LSTMSequence(torch.autograd.Function):
    """Time loop in PyTorch ops (the CPU, and the GPU when the HIP kernels do not apply)."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh):
        L, B, _ = x.shape
        H = w_hh.shape[1]
        ig = (x.reshape(L * B, -1) @ w_ih.t()).view(L, B, 4 * H)
        w_hh_t = w_hh.t().contiguous()
        bias = b_ih + b_hh
        out = x.new_empty(L, B, H)
        cell = x.new_empty(L, B, H)
        ws = x.new_empty(L, B, 4 * H)  # the activated gates i, f, g, o
        h, c = h0, c0
        for t in range(L):
            a = torch.addmm(ig[t] + bias, h, w_hh_t)
            torch.sigmoid(a[:, :2 * H], out=ws[t, :, :2 * H])
            torch.tanh(a[:, 2 * H:3 * H], out=ws[t, :, 2 * H:3 * H])
            torch.sigmoid(a[:, 3 * H:], out=ws[t, :, 3 * H:])
            i, f, g, o = ws[t].split(H, dim=1)
            c = f * c + i * g
            h = o * torch.tanh(c)
            out[t] = h
            cell[t] = c
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, h0, c0, w_ih, w_hh, out, cell, ws)
        return out, h, c

    @staticmethod
    def backward(ctx, dout, dhn, dcn):
        x, h0, c0, w_ih, w_hh, out, cell, ws = ctx.saved_tensors
        L, B, _ = x.shape
        H = w_hh.shape[1]
        dgates = x.new_empty(L, B, 4 * H)
        dh = dhn if dhn is not None else x.new_zeros(B, H)
        dc = dcn if dcn is not None else x.new_zeros(B, H)
        for t in range(L - 1, -1, -1):
            if dout is not None:
                dh = dh + dout[t]
            i, f, g, o = ws[t].split(H, dim=1)
            tc = torch.tanh(cell[t])
            dc = dc + dh * o * (1 - tc * tc)
            c_prev = cell[t - 1] if t > 0 else c0
            dgates[t] = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], dim=1)
            dh = dgates[t] @ w_hh
            dc = dc * f
        return _finish_backward(ctx, x, h0, w_ih, out, dgates, dh, dc)


class _LSTMSequenceHip(torch.autograd.Function):
    """Time loop in csrc/lt_lstm.hip: one launch per step forward, one per step (+ the one that opens the recursion) backward."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh):
        from .. import _abi

        L, B, _ = x.shape
        H = w_hh.shape[1]
        ig = (x.reshape(L * B, -1) @ w_ih.t()).view(L, B, 4 * H)
        h0c, c0c, w_hh_c = h0.contiguous(), c0.contiguous(), w_hh.contiguous()
        out = x.new_empty(L, B, H)
        cell = x.new_empty(L, B, H)
        ws = x.new_empty(L, B, 4 * H)
        _abi.call("lt_lstm_forward", ig, h0c, c0c, w_hh_c, b_ih.contiguous(), b_hh.contiguous(), L, B, H, out, cell, ws, _abi.stream(x.device))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, h0c, c0c, w_ih, w_hh_c, out, cell, ws)
        return out, out[-1].clone(), cell[-1].clone()  # copies, as nn.LSTM's: `reset()` of the callers rewrites the carried state in place

    @staticmethod
    def backward(ctx, dout, dhn, dcn):
        from .. import _abi

        x, h0, c0, w_ih, w_hh, out, cell, ws = ctx.saved_tensors
        L, B, _ = x.shape
        H = w_hh.shape[1]
        dout = dout.contiguous() if dout is not None else x.new_zeros(L, B, H)
        dhn = dhn.contiguous() if dhn is not None else None
        dcn = dcn.contiguous() if dcn is not None else None
        dgates = x.new_empty(L, B, 4 * H)
        scratch = x.new_empty(B, H)
        dh0 = x.new_empty(B, H)
        dc0 = x.new_empty(B, H)
        _abi.call("lt_lstm_backward", dout, dhn, dcn, out, cell, ws, h0, c0, w_hh, L, B, H, dgates, scratch, dh0, dc0, _abi.stream(x.device))
        return _finish_backward(ctx, x, h0, w_ih, out, dgates, dh0, dc0)


def lstm_sequence(lstm: torch.nn.LSTM, x: torch.Tensor, hc0: tuple[torch.Tensor, torch.Tensor] | None = None):
    """`lstm(x, (h0, c0))` for a single-layer, unidirectional, time-major `nn.LSTM`: (output [L, B, H], (h_n, c_n) [1, B, H] each)."""
    assert lstm.num_layers == 1 and not lstm.bidirectional and not lstm.batch_first and lstm.bias and lstm.proj_size == 0
    if hc0 is not None:
        h, c = hc0[0][0], hc0[1][0]
    else:
        h = c = x.new_zeros(x.shape[1], lstm.hidden_size)
    fn = _LSTMSequenceHip if (x.is_cuda and x.dtype == torch.float32 and lstm.hidden_size % 64 == 0 and use_hip_kernels) else _LSTMSequence
    out, hn, cn = fn.apply(x.contiguous(), h, c, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)
    return out, (hn.unsqueeze(0), cn.unsqueeze(0))


def serves(rnn: torch.nn.Module, x: torch.Tensor) -> bool:
    """Whether `Memory` / `PolicyMemory` send (rnn, x) through `lstm_sequence`'s HIP form: a CUDA, f32, single-layer, unidirectional
    `nn.LSTM` with biases, no projection and a hidden size the kernels cover."""
    return (isinstance(rnn, torch.nn.LSTM) and x.is_cuda and x.dtype == torch.float32 and rnn.num_layers == 1 and not rnn.bidirectional
            and not rnn.batch_first and rnn.bias and rnn.proj_size == 0 and rnn.hidden_size % 64 == 0 and use_hip_kernels)


# False: `Memory` / `PolicyMemory` keep nn.LSTM's own (MIOpen) path and `lstm_sequence` takes the PyTorch-op time loop on the GPU as well.
# On: tools/lstm_probe.py -> profiles/lstm_probe_{24000,50000}.json, the HIP form is 2.6x / 2.2x nn.LSTM at L = 500, B = 48 / 100.
use_hip_kernels = True
