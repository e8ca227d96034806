"""PPO minibatch loss through csrc/lt_ppo.hip: forward and gradients in ONE launch instead of ~105 small PyTorch launches.

`fused_ppo_loss(mu, std, value, batch..., cfg...)` returns (loss, surrogate, value_loss, entropy, kl) with autograd edges to
`mu`, `std` and `value`; the formulas are the reference's (loco_rl/loco_rl/algorithms/ppo.py:251-311), checked against the
PyTorch-op chain of `PPO._eager_update` in tests/test_hip_ppo_graph.py.  CUDA tensors, f32, state-independent std: the policy's `std`
parameter ("scalar" noise type) or, with `std_is_log=True`, its `log_std` ("log"), whose gradient the backward then returns.
"""
from __future__ import annotations

import math

import torch

from .. import _abi


class _FusedPPOLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, std, value, actions, old_logp, adv, returns, old_values, old_mu, old_sigma, clip, vcoef, ecoef, clipped, idx,
                std_is_log=False, adv_stats=None):
        m, a = mu.shape
        c = lambda t: t.detach().contiguous()  # noqa: E731
        mu_c, std_c, v_c = c(mu), c(std), c(value).view(-1)
        dmu = torch.empty_like(mu_c)
        dvalue = torch.empty(m, device=mu.device, dtype=torch.float32)
        acc = torch.empty(24, device=mu.device, dtype=torch.float32)
        args = [c(actions), c(old_logp).view(-1), c(adv).view(-1), c(returns).view(-1), c(old_values).view(-1), c(old_mu), c(old_sigma)]
        rows = args[0].shape[0]
        if (any(t.shape[0] != rows for t in args) or any(t.shape != (rows, a) for t in (args[0], args[5], args[6]))
                or (idx is None and rows != m) or (idx is not None and (idx.dtype != torch.int64 or idx.numel() != m))):
            raise ValueError("fused_ppo_loss: batch tensors do not match the minibatch / index")
        idx_c = None if idx is None else c(idx)
        out = torch.empty(24, device=mu.device, dtype=torch.float32)
        if std_is_log or adv_stats is not None:  # include/lt_ppo_opts.h
            if adv_stats is not None and (adv_stats.dtype != torch.float32 or adv_stats.numel() != 2 or not adv_stats.is_contiguous()
                                          or adv_stats.device != mu.device):
                raise ValueError("fused_ppo_loss: adv_stats must be two contiguous f32 values (mean, 1 / (std + 1e-8)) on the minibatch's device")
            _abi.call("lt_ppo_loss_opts", mu_c, std_c, v_c, *args, idx_c, m, a, float(clip), float(vcoef), float(ecoef), int(bool(clipped)),
                      int(bool(std_is_log)), adv_stats, dmu, dvalue, acc, out, _abi.stream(mu.device))
        else:
            _abi.call("lt_ppo_loss", mu_c, std_c, v_c, *args, idx_c, m, a, float(clip), float(vcoef), float(ecoef), int(bool(clipped)),
                      dmu, dvalue, acc, out, _abi.stream(mu.device))
        # out: the finished scalars, written by a one-wave launch behind the main kernel (a dozen 12-float tensor ops otherwise)
        ctx.save_for_backward(dmu, dvalue.view_as(value), out[8:8 + a])
        return out[0], out[1], out[2], out[3], out[4]

    @staticmethod
    def backward(ctx, g, *unused):
        dmu, dvalue, dstd = ctx.saved_tensors
        # (dstd: with respect to the tensor passed as `std` - sigma, or log sigma for a log-type policy)
        return g * dmu, g * dstd, g * dvalue, None, None, None, None, None, None, None, None, None, None, None, None, None, None


def fused_ppo_loss(mu, std, value, actions, old_logp, adv, returns, old_values, old_mu, old_sigma, clip_param, value_loss_coef,
                   entropy_coef, use_clipped_value_loss, idx=None, std_is_log=False, adv_stats=None):
    """`idx` (int64 [M], optional): the batch tensors `actions ... old_sigma` are then the WHOLE flattened rollout storage and
    minibatch row i is their row idx[i] - the kernel gathers while it loads, seven gather launches less per step.
    `std_is_log`: `std` is the `log_std` parameter of a `noise_std_type="log"` policy; sigma = exp(std) and the gradient that comes back
    is the one with respect to log sigma.  `adv_stats` (f32 [2], optional: mean and 1 / (std + 1e-8) of this minibatch's advantages, as
    `lt_adv_stats` writes them): the advantages enter as (adv - adv_stats[0]) * adv_stats[1] (`normalize_advantage_per_mini_batch`)."""
    return _FusedPPOLoss.apply(mu, std, value, actions, old_logp, adv, returns, old_values, old_mu, old_sigma, clip_param, value_loss_coef,
                               entropy_coef, use_clipped_value_loss, idx, std_is_log, adv_stats)


def std_param(ac):
    """(the state-independent std parameter of a plain ActorCritic, whether it holds log sigma): `std` or `log_std`"""
    if getattr(ac, "noise_std_type", "scalar") == "log":
        return ac.log_std, True
    return ac.std, False


def adv_stats(adv, idx, m, nmb):
    """f32 [nmb, 2]: (mean, 1 / (unbiased std + 1e-8)) of the advantages of each of `nmb` minibatches of `m` rows - rows
    idx[b m .. (b + 1) m) of the flattened storage `adv` (idx None: the rows themselves) - in ONE launch (`lt_adv_stats`)."""
    adv = adv.detach().contiguous().view(-1)
    if idx is not None and (idx.dtype != torch.int64 or idx.numel() < nmb * m or not idx.is_contiguous()):
        raise ValueError("adv_stats: idx must be a contiguous int64 index of at least nmb * m rows")
    if idx is None and adv.numel() < nmb * m:
        raise ValueError("adv_stats: fewer advantages than nmb * m")
    stats = torch.empty(nmb, 2, device=adv.device, dtype=torch.float32)
    _abi.call("lt_adv_stats", adv, idx, int(m), int(nmb), stats, _abi.stream(adv.device))
    return stats
