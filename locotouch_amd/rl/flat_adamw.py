"""`AdamW.step()` as one launch on flat buffers (csrc/lt_bc.hip `lt_adamw_step`).

The student's behaviour-cloning step ends with `torch.optim.AdamW.step()` over ~28 small tensors (locotouch_amd/distill/student.py;
reference locotouch/distill/student.py:60,150): multi-tensor launches, as the PPO step had before `FlatAdam`.  `FlatAdamW` is the
`FlatAdam` scheme for a single-group `torch.optim.AdamW`: the parameters with `requires_grad`, their gradients and both moments live in
four flat f32 buffers, the tensors the module and the optimizer hold become VIEWS of them (so `state_dict()` / `load_state_dict()` of
both keep torch's layout and checkpoints interchange), a re-bind is detected and re-adopted before the next step, and `step()` is one
kernel with AdamW's DECOUPLED weight decay (`lt_adam_clip_step` has Adam's coupled one) and no gradient clipping.

One rule differs from `FlatAdam` on purpose: a parameter whose `.grad` is None at `step()` raises.  Torch skips such a parameter, its
decay included; a fused step that counted the gradient as zero would still decay it, so it must not pass quietly.
"""
from __future__ import annotations

import torch

from .. import _abi
from .flat_adam import FlatAdam


class FlatAdamW(FlatAdam):
    def __init__(self, optimizer: torch.optim.AdamW):
        if type(optimizer) is not torch.optim.AdamW or len(optimizer.param_groups) != 1:
            raise TypeError("FlatAdamW wraps a single-group torch.optim.AdamW")
        g = optimizer.param_groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable"):
            raise TypeError("FlatAdamW: amsgrad / maximize / capturable / differentiable are not supported")
        self.optimizer = optimizer
        self.params = [p for p in g["params"] if p.requires_grad]
        if not self.params or any(p.dtype != torch.float32 or not p.is_cuda for p in self.params):
            raise ValueError("FlatAdamW needs f32 CUDA parameters (there is no fall-back)")
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += -(-p.numel() // self.ALIGN) * self.ALIGN
        self.n = off
        dev = self.params[0].device
        self.flat_p = torch.zeros(self.n, device=dev)
        self.flat_g = torch.zeros(self.n, device=dev)
        self.flat_m = torch.zeros(self.n, device=dev)
        self.flat_v = torch.zeros(self.n, device=dev)
        self._adopt()

    def _adopt(self) -> None:
        """`FlatAdam._adopt`, then a step tensor of its OWN per parameter: torch's AdamW increments every parameter's `step` in place, so
        a state dict whose entries share one tensor would count a step once per parameter in a plain `torch.optim.AdamW` it is loaded
        into."""
        super()._adopt()
        self._steps = [torch.tensor(float(self.step_count)) for _ in self.params]
        self._step_t = self._steps[0]  # (what `_bound` looks for)
        for p, t in zip(self.params, self._steps):
            self.optimizer.state[p]["step"] = t

    def gather_grads(self) -> torch.Tensor:
        """Pack the parameters' gradients into `flat_g` with one multi-tensor copy and re-point `.grad` at its views."""
        missing = [i for i, p in enumerate(self.params) if p.grad is None]
        if missing:
            raise RuntimeError(f"FlatAdamW.step: {len(missing)} parameter(s) have no gradient (first: index {missing[0]}, shape "
                               f"{tuple(self.params[missing[0]].shape)}); torch.optim.AdamW would skip them, decay included")
        have = [(v, p.grad) for p, v in zip(self.params, self._gviews) if p.grad.data_ptr() != v.data_ptr()]
        if have:
            torch._foreach_copy_([v for v, _ in have], [g for _, g in have])
        for p, v in zip(self.params, self._gviews):
            p.grad = v
        return self.flat_g

    def step_dev(self, max_norm, lr_dev) -> None:
        raise TypeError("FlatAdamW has no device-side learning rate")

    def step(self, gathered: bool = False) -> None:
        if not self._bound():
            self._adopt()
        if not gathered:
            self.gather_grads()
        g = self.optimizer.param_groups[0]
        self.step_count += 1
        b1, b2 = g["betas"]
        _abi.call("lt_adamw_step", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.n, float(g["lr"]), float(b1), float(b2),
                  float(g["eps"]), float(g["weight_decay"]), self.step_count, _abi.stream(self.flat_p.device))
        for t in self._steps:  # (host tensors)
            t.fill_(float(self.step_count))
