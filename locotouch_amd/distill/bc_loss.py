"""The masked behaviour-cloning loss and its statistics in HIP kernels (include/lt_bc.h `lt_bc_loss_forward` / `lt_bc_loss_backward`).

`Student.batch_loss` is the definition: about twenty elementwise and reduction launches on [L][B][12] tensors going forward and autograd's
mirror of them going back.  `bc_loss` computes the same three scalars in two launches (workgroup partials, the finish) and the gradient
with respect to the loss pair in one; the incoming gradient and the mask count are read from device memory, so no host read sits
between them.  Opt-in (`Student.enable_fused_bc_step`); a non-CUDA tensor raises `ValueError` - nothing falls back.
"""
from __future__ import annotations

import ctypes

import torch

from .. import _abi


def _rows(x: torch.Tensor, what: str) -> torch.Tensor:
    if not x.is_cuda or x.dtype != torch.float32:
        raise ValueError(f"bc_loss: {what} must be a float32 CUDA tensor (there is no fall-back)")
    return x.detach().reshape(-1, x.shape[-1]).contiguous()


class _BcLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, sa, ta, mask, clip_range, action_scale):
        p, t = _rows(pred, "pred"), _rows(target, "target")
        if p.shape != t.shape:
            raise ValueError(f"bc_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
        m = mask.detach().reshape(-1).contiguous()
        if m.dtype not in (torch.bool, torch.uint8) or not m.is_cuda or m.numel() != p.shape[0]:
            raise ValueError("bc_loss: masks must be a bool CUDA tensor with one entry per row")
        a = b = None
        if sa is not None:
            a, b = _rows(sa, "student actions"), _rows(ta, "teacher actions")
            if a.shape != b.shape or a.shape[0] != p.shape[0]:
                raise ValueError("bc_loss: the action pair must have one row per row of the loss pair")
        R, W = p.shape
        size = ctypes.c_size_t()
        _abi.call("lt_bc_loss_ws_floats", R, ctypes.byref(size))
        ws = torch.empty(size.value, device=p.device)
        stats = torch.empty(_abi.BC_CONSTS["LT_BC_STATS_FIELDS"], device=p.device)
        _abi.call("lt_bc_loss_forward", p, t, W, a, b, 0 if a is None else a.shape[1], m, R, float(clip_range), float(action_scale), stats, ws,
                  _abi.stream(p.device))
        ctx.save_for_backward(p, t, m, stats)
        ctx.shape = pred.shape
        loss, mse, mae = stats[_abi.BC_CONSTS["LT_BC_LOSS"]], stats[_abi.BC_CONSTS["LT_BC_ACTION_MSE"]], stats[_abi.BC_CONSTS["LT_BC_ACTION_MAE"]]
        ctx.mark_non_differentiable(mse, mae)
        ctx.set_materialize_grads(False)  # (no zero tensors for the two statistics)
        return loss, mse, mae

    @staticmethod
    def backward(ctx, g, _g_mse, _g_mae):
        if g is None:
            return (None,) * 7
        p, t, m, stats = ctx.saved_tensors
        d_pred = torch.empty_like(p)
        g = g.to(torch.float32).contiguous()
        _abi.call("lt_bc_loss_backward", p, t, p.shape[1], m, p.shape[0], g, stats, d_pred, _abi.stream(p.device))
        return d_pred.view(ctx.shape), None, None, None, None, None, None


def bc_loss(pred, target, masks, student_actions=None, teacher_actions=None, clip_range: float = 0.0, action_scale: float = 1.0):
    """(loss, action_mse | None, action_mae) as device scalars, shaped as `Student.batch_loss` returns them.

    `pred`, `target` [..., W]: the loss pair, gradient flows to `pred` only; `masks` [...]: bool.  Monolithic distillation gives no action
    pair - the loss pair is the action pair and `action_mse` is None; RMA passes the embedding pair and the actions.
    `clip_range <= 0`: the actions are not clipped for `action_mae`."""
    if (student_actions is None) != (teacher_actions is None):
        raise ValueError("bc_loss: student_actions and teacher_actions are given together")
    loss, mse, mae = _BcLoss.apply(pred, target, student_actions, teacher_actions, masks, clip_range, action_scale)
    return loss, (None if student_actions is None else mse), mae
