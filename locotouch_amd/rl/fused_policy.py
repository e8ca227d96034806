"""Opt-in inference front of a recurrent policy: one env step through `lt_policy_step` (include/lt_policy.h, csrc/lt_policy.hip) - the
memory step and the actor MLP as two HIP launches instead of the eager chain `PolicyMemory.forward` -> `lstm_sequence(L = 1)` or
`nn.GRU` -> torch MLP.

`FusedRecurrentPolicy.for_actor_critic(ac, normalizer=None)` reads `ac.memory_a.rnn` and `ac.actor` of an `ActorCriticRecurrent` (it
owns no parameters) and offers the call surface of the play loop: `__call__(obs)`, `reset(dones=None)`, `get_hidden_states()`,
`eval()` / `train()`.  `refresh()` re-packs the actor after the module changed.  What the kernels do not serve raises `ValueError` with
the validator's message - there is no fall-back to the eager path.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from .. import _abi
from .mlp import PackedMLP
from .modules import ActorCriticRecurrent
from .normalizer import EmpiricalNormalization


class FusedRecurrentPolicy:
    def __init__(self, actor_critic, normalizer=None):
        ac = actor_critic
        if type(ac) is not ActorCriticRecurrent:
            raise ValueError(f"FusedRecurrentPolicy: actor_critic must be a plain ActorCriticRecurrent, got {type(ac).__name__}")
        if normalizer is not None and not isinstance(normalizer, EmpiricalNormalization):
            raise ValueError(f"FusedRecurrentPolicy: normalizer must be an EmpiricalNormalization or None, got {type(normalizer).__name__}")
        self.actor_critic, self.normalizer = ac, normalizer
        rnn = ac.memory_a.rnn
        self.lstm = isinstance(rnn, nn.LSTM)
        try:
            self.mlp = PackedMLP(ac.actor)
        except ValueError as e:
            raise ValueError(f"FusedRecurrentPolicy: actor: {e}") from None
        d = _abi.LtPolicyDesc()
        d.rnn_type = _abi.LT_POLICY_RNN_LSTM if self.lstm else _abi.LT_POLICY_RNN_GRU
        d.rnn_layers, d.rnn_hidden, d.obs_dim = rnn.num_layers, rnn.hidden_size, rnn.input_size
        d.actor = self.mlp.desc
        self.desc = d
        lib = _abi.load()
        if lib.lt_policy_validate(ctypes.byref(d)) != 0:
            raise ValueError(f"FusedRecurrentPolicy: {lib.lt_last_error().decode()}")
        if not rnn.bias or rnn.bidirectional or getattr(rnn, "proj_size", 0) or rnn.dropout:
            raise ValueError("FusedRecurrentPolicy: the memory must be a unidirectional rnn with biases, without projection or dropout")
        self._params = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]
        if any(t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t in self._params):
            raise ValueError("FusedRecurrentPolicy: every parameter of the memory must be a contiguous float32 CUDA tensor")
        self.device = self._params[0].device
        self.hidden, self.obs_dim, self.actions_dim = d.rnn_hidden, d.obs_dim, self.mlp.out_features
        self.launches = lib.lt_policy_step_launches(ctypes.byref(d), 1)
        self._state = None      # two ping-pong sets of (h,) or (h, c), each [n][H]; `_cur` is the one the next step reads
        self._cur = 0
        self._dones = None      # the mask `reset(dones)` stored: applied by the next step, inside the memory launch
        self._fresh = True      # no state yet / reset(): the next step starts from zeros
        self.refresh()

    @classmethod
    def for_actor_critic(cls, actor_critic, normalizer=None) -> "FusedRecurrentPolicy":
        """The fused front of `actor_critic`; ValueError (the validator's message) for what the kernels do not serve."""
        return cls(actor_critic, normalizer)

    def refresh(self) -> None:
        """Re-pack the actor (stream-ordered, no host read) and re-read the normaliser's statistics: call after the module changed.
        The memory's own parameters are read in place by every step."""
        m = _abi.LtPolicyMemory()
        m.w_ih, m.w_hh, m.b_ih, m.b_hh = (t.data_ptr() for t in self._params)
        if self.normalizer is not None:
            nz = self.normalizer
            self._norm = (nz._mean.detach().reshape(-1).to(self.device, torch.float32).contiguous(),
                          nz._std.detach().reshape(-1).to(self.device, torch.float32).contiguous())
            if self._norm[0].numel() != self.obs_dim:
                raise ValueError(f"FusedRecurrentPolicy: the normaliser holds {self._norm[0].numel()} columns, the memory reads {self.obs_dim}")
            m.norm_mean, m.norm_std, m.norm_eps = self._norm[0].data_ptr(), self._norm[1].data_ptr(), float(nz.eps)
        self._mem = m
        with torch.cuda.device(self.device):
            self.mlp.pack()

    def _buffers(self, n: int) -> None:
        if self._state is None or self._state[0][0].shape[0] != n:
            self._state = [tuple(torch.zeros(n, self.hidden, dtype=torch.float32, device=self.device) for _ in range(2 if self.lstm else 1))
                           for _ in range(2)]
            self._cur, self._dones, self._fresh = 0, None, True

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        """Mean actions [n][num_actions] of one env step; the memory state advances.  `obs` may be a column slice of wider rows (unit
        column stride): read in place."""
        if not isinstance(obs, torch.Tensor) or obs.dtype != torch.float32 or not obs.is_cuda or obs.device != self.device:
            raise TypeError(f"FusedRecurrentPolicy: obs must be a float32 tensor on {self.device}")
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim or (obs.shape[1] > 1 and obs.stride(1) != 1) or (obs.shape[0] > 1 and obs.stride(0) < self.obs_dim):
            raise ValueError(f"FusedRecurrentPolicy: obs must be [n][{self.obs_dim}] with unit column stride, got {tuple(obs.shape)} strides {obs.stride()}")
        n = obs.shape[0]
        self._buffers(n)
        src, dst = self._state[self._cur], self._state[self._cur ^ 1]
        if self._fresh:
            for t in src:
                t.zero_()
            self._fresh = False
        actions = torch.empty(n, self.actions_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.call("lt_policy_step", self.desc, self._mem, self.mlp.packed, obs, max(obs.stride(0), self.obs_dim) if n > 1 else self.obs_dim,
                      self._dones, src[0], src[1] if self.lstm else None, dst[0], dst[1] if self.lstm else None, n, actions,
                      _abi.stream(self.device))
        self._cur ^= 1
        self._dones = None
        return actions

    def reset(self, dones=None) -> None:
        """`ActorCriticRecurrent.reset`: None forgets the state; a per-env mask is STORED and zeroes those rows inside the next step (no
        launch for a bool / uint8 mask; the tensor must stay unchanged until that step).  Two masks without a step between are OR-ed."""
        if dones is None:
            self._fresh, self._dones = True, None
            return
        if self._state is None or self._fresh:
            return
        d = dones.reshape(-1)
        if d.dtype not in (torch.bool, torch.uint8) or not d.is_contiguous():
            d = (d != 0).contiguous()
        if d.shape[0] != self._state[0][0].shape[0] or d.device != self.device:
            raise ValueError("FusedRecurrentPolicy.reset: one mask entry per env, on the policy's device")
        if self._dones is not None:
            d = d.to(torch.bool) | self._dones.to(torch.bool)
        self._dones = d

    def get_hidden_states(self):
        """What `ActorCriticRecurrent.get_hidden_states()[0]` would hold - (1, n, H) for a GRU, the pair (h, c) of them for an LSTM -
        with a pending reset applied; None before the first step."""
        if self._state is None or self._fresh:
            return None
        keep = None if self._dones is None else (self._dones == 0).to(torch.float32)[:, None]
        out = tuple((t if keep is None else t * keep).unsqueeze(0) for t in self._state[self._cur])
        return out if self.lstm else out[0]

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self
