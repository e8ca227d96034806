"""Opt-in device form of the tactile delay line: `TactileRecorder` as a ring buffer behind the C ABI (include/lt_collect.h,
csrc/lt_collect.hip) - one HIP launch per call instead of the shift / fill / gather / mask passes over the whole register.

`DeviceTactileRecorder` has the constructor and the four methods of `TactileRecorder` (`reset`, `record_new_tactile_signals`,
`get_tactile_signals`, the attributes `delay_steps`, `min_delay`, `max_delay`) and returns the same bits: rows are only moved.  It
adds the fused forms the loops use: `push` (record + delayed rows to one or two destinations + a row copy, one launch) and
`after_step` (reward and done mask to their store slots + the reset of the finished envs, one launch behind the env step).

Delays are drawn exactly as the eager class draws them - one `torch.randint(low=min_delay, high=max_delay, size=(env_num,))` in the
constructor and one per `reset` / `after_step` call - so two runs from the same seed consume the generator identically.
A non-CUDA device raises `ValueError`: there is no fall-back to the eager class.
"""
from __future__ import annotations

import ctypes
import math

import torch

from .. import _abi


class DeviceTactileRecorder:
    def __init__(self, device, env_num: int, tactile_shape, min_delay: int = 3, max_delay: int = 7):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceTactileRecorder: the delay line runs in HIP kernels and needs a CUDA device, got {device!r} "
                             "(use TactileRecorder there)")
        if not 0 <= int(min_delay) < int(max_delay):
            raise ValueError("DeviceTactileRecorder: 0 <= min_delay < max_delay (delays are drawn from [min_delay, max_delay))")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.env_num = int(env_num)
        self.tactile_shape = (tactile_shape,) if isinstance(tactile_shape, int) else tuple(tactile_shape)
        self.min_delay, self.max_delay = int(min_delay), int(max_delay)
        self.dim, self.depth = math.prod(self.tactile_shape), self.max_delay  # every delay is < max_delay: the ring's depth
        size = ctypes.c_size_t()
        _abi.call("lt_delay_state_bytes", self.env_num, self.dim, self.depth, ctypes.byref(size))
        assert size.value % 4 == 0
        self._state = torch.zeros(size.value // 4, dtype=torch.int32, device=self.device)  # ring | head | count | delay (lt_collect.h)
        self._ints = self._state[size.value // 4 - 3 * self.env_num:].view(3, self.env_num)
        self._out = torch.zeros(self.env_num, self.dim, dtype=torch.float32, device=self.device)  # record_new_tactile_signals' destination
        self.reset()

    # ---- the eager class's surface ---------------------------------------------------------------------------------
    @property
    def delay_steps(self) -> torch.Tensor:
        """[env_num] int64, as `TactileRecorder.delay_steps` (a copy of the state's int32 column)."""
        return self._ints[2].to(torch.long)

    def _fresh(self) -> torch.Tensor:
        # torch.randint(low=min_delay, high=max_delay): the upper bound is exclusive (tactile_recorder.py:22), so every draw is < depth
        return torch.randint(low=self.min_delay, high=self.max_delay, size=(self.env_num,), device=self.device)

    def reset(self, env_idx=None):
        """`env_idx`: index tensor (reference call form), bool mask [env_num], or None = all."""
        mask = env_idx
        if env_idx is not None and env_idx.dtype != torch.bool:
            mask = torch.zeros(self.env_num, dtype=torch.bool, device=self.device)
            mask[env_idx] = True
        if mask is not None:
            if mask.shape != (self.env_num,) or mask.device != self.device:
                raise ValueError("DeviceTactileRecorder.reset: one mask entry per env, on the recorder's device")
            mask = mask.contiguous()
        fresh = self._fresh()
        with torch.cuda.device(self.device):
            _abi.call("lt_delay_reset", self._state, self.env_num, self.dim, self.depth, mask, fresh, _abi.stream(self.device))

    def record_new_tactile_signals(self, tactile_signals: torch.Tensor):
        self.push(tactile_signals, self._out)

    def get_tactile_signals(self) -> torch.Tensor:
        out = torch.empty(self.env_num, self.dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.call("lt_delay_read", self._state, self.env_num, self.dim, self.depth, out, out.stride(0), _abi.stream(self.device))
        return out.view(self.env_num, *self.tactile_shape)

    # ---- the fused forms ---------------------------------------------------------------------------------------------
    def _rows(self, name: str, x: torch.Tensor, width: int) -> torch.Tensor:
        """`x` as [env_num][width] float32 rows with unit column stride on the recorder's device (a view; anything else raises)."""
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != self.device:
            raise TypeError(f"DeviceTactileRecorder: {name} must be a float32 tensor on {self.device}")
        if x.dim() > 2:
            x = x.view(x.shape[0], -1)  # (raises for rows that are not contiguous inside)
        if x.dim() != 2 or x.shape != (self.env_num, width) or (width > 1 and x.stride(1) != 1):
            raise ValueError(f"DeviceTactileRecorder: {name} must be [{self.env_num}][{width}] with unit column stride, "
                             f"got {tuple(x.shape)} strides {x.stride()}")
        return x

    def push(self, rows: torch.Tensor, out: torch.Tensor, store: torch.Tensor | None = None, copy=None) -> torch.Tensor:
        """Record `rows` and write the delayed rows to `out` and, if given, to `store`; `copy = (src, dst)` copies equally shaped
        rows (the policy rows into their store slot) in the same launch.  Every operand may be a column slice of wider rows.
        Returns `out`."""
        rows, o0 = self._rows("rows", rows, self.dim), self._rows("out", out, self.dim)
        o1 = None if store is None else self._rows("store", store, self.dim)
        src = dst = None
        cd = 0
        if copy is not None:
            cd = copy[0].shape[-1] if isinstance(copy[0], torch.Tensor) and copy[0].dim() == 2 else 0
            src, dst = self._rows("copy source", copy[0], cd), self._rows("copy destination", copy[1], cd)
        with torch.cuda.device(self.device):
            _abi.call("lt_delay_push", self._state, self.env_num, self.dim, self.depth, rows, rows.stride(0), o0, o0.stride(0),
                      o1, 0 if o1 is None else o1.stride(0), src, 0 if src is None else src.stride(0), dst, 0 if dst is None else dst.stride(0),
                      cd, _abi.stream(self.device))
        self.last_delayed = o0
        return out

    last_delayed = None  # the delayed rows `push` wrote last (what the student read): a viewer's handle, no copy and no launch

    def after_step(self, reward: torch.Tensor, dones: torch.Tensor, reward_out: torch.Tensor, done_out: torch.Tensor) -> None:
        """Behind an env step: `reward_out = reward`, `done_out = dones != 0` (bool or uint8 [env_num]: what a student's `reset`
        takes as its pending mask) and the delay-line reset of the finished envs, with one fresh draw - one launch."""
        n = self.env_num
        for name, x, dtypes in (("reward", reward, (torch.float32,)), ("dones", dones, (torch.int64,)), ("reward_out", reward_out, (torch.float32,)),
                                ("done_out", done_out, (torch.bool, torch.uint8))):
            if not isinstance(x, torch.Tensor) or x.dtype not in dtypes or x.device != self.device or x.shape != (n,) or not x.is_contiguous():
                raise TypeError(f"DeviceTactileRecorder.after_step: {name} must be a contiguous [{n}] tensor of "
                                f"{' or '.join(str(t) for t in dtypes)} on {self.device}")
        fresh = self._fresh()
        with torch.cuda.device(self.device):
            _abi.call("lt_collect_after_step", self._state, n, self.dim, self.depth, reward, dones, fresh, reward_out, done_out,
                      _abi.stream(self.device))
