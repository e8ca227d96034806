"""Opt-in inference fronts of the policy classes with a memory or an encoder: one env step on HIP launches instead of the eager chain.

`FusedRecurrentPolicy` - an `ActorCriticRecurrent` through `lt_policy_step` (include/lt_policy.h, csrc/lt_policy.hip): the memory step
and the actor MLP as two launches instead of `PolicyMemory.forward` -> `lstm_sequence(L = 1)` or `nn.GRU` -> torch MLP.

`FusedEncoderPolicy` - an `ActorCriticRNNEncoder` or an `ActorCriticEncoder` through `lt_policy_encoder_step`
(include/lt_policy_encoder.h, csrc/lt_policy_encoder.hip): the memory step on the tail columns, then ONE launch for the normalised head
columns, the encoder, the concatenation and the actor (the plain class: that launch alone) instead of the torch normaliser,
`PolicyMemory.forward`, the encoder's modules, `torch.cat` and the actor's modules.

`X.for_actor_critic(ac, normalizer=None)` reads the module's parameters (it owns none) and offers the call surface of the play loop:
`__call__(obs)`, `reset(dones=None)`, `get_hidden_states()`, `eval()` / `train()`, `launches`.  `refresh()` is to be called after the
module or the normaliser changed.  What the kernels do not serve raises `ValueError` with the validator's message - there is no
fall-back to the eager path.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from .. import _abi
from .mlp import PackedMLP
from .modules import ActorCriticEncoder, ActorCriticRecurrent, ActorCriticRNNEncoder
from .normalizer import EmpiricalNormalization


class _MemoryState:
    """The memory state of a front and its reset protocol: two ping-pong sets of (h,) or (h, c), each [n][H]; a mask `reset(dones)`
    stores is applied by the next step, inside the memory launch.  `hidden == 0`: a policy without a memory - no state, `reset` does
    nothing, `get_hidden_states()` is None."""

    hidden = 0
    lstm = False

    def _init_state(self) -> None:
        self._state = None      # two ping-pong sets of (h,) or (h, c), each [n][H]; `_cur` is the one the next step reads
        self._cur = 0
        self._dones = None      # the mask `reset(dones)` stored: applied by the next step, inside the memory launch
        self._fresh = True      # no state yet / reset(): the next step starts from zeros

    def _buffers(self, n: int) -> None:
        if self._state is None or self._state[0][0].shape[0] != n:
            self._state = [tuple(torch.zeros(n, self.hidden, dtype=torch.float32, device=self.device) for _ in range(2 if self.lstm else 1))
                           for _ in range(2)]
            self._cur, self._dones, self._fresh = 0, None, True

    def _step_buffers(self, n: int):
        """(the set the step reads, the set it writes), the first one zeroed behind `reset()`."""
        self._buffers(n)
        src, dst = self._state[self._cur], self._state[self._cur ^ 1]
        if self._fresh:
            for t in src:
                t.zero_()
            self._fresh = False
        return src, dst

    def _check_obs(self, obs) -> None:
        name = type(self).__name__
        if not isinstance(obs, torch.Tensor) or obs.dtype != torch.float32 or not obs.is_cuda or obs.device != self.device:
            raise TypeError(f"{name}: obs must be a float32 tensor on {self.device}")
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim or (obs.shape[1] > 1 and obs.stride(1) != 1) or (obs.shape[0] > 1 and obs.stride(0) < self.obs_dim):
            raise ValueError(f"{name}: obs must be [n][{self.obs_dim}] with unit column stride, got {tuple(obs.shape)} strides {obs.stride()}")

    def reset(self, dones=None) -> None:
        """The module's `reset`: None forgets the state; a per-env mask is STORED and zeroes those rows inside the next step (no launch
        for a bool / uint8 mask; the tensor must stay unchanged until that step).  Two masks without a step between are OR-ed."""
        if not self.hidden:
            return
        if dones is None:
            self._fresh, self._dones = True, None
            return
        if self._state is None or self._fresh:
            return
        d = dones.reshape(-1)
        if d.dtype not in (torch.bool, torch.uint8) or not d.is_contiguous():
            d = (d != 0).contiguous()
        if d.shape[0] != self._state[0][0].shape[0] or d.device != self.device:
            raise ValueError(f"{type(self).__name__}.reset: one mask entry per env, on the policy's device")
        if self._dones is not None:
            d = d.to(torch.bool) | self._dones.to(torch.bool)
        self._dones = d

    def get_hidden_states(self):
        """What the module's `get_hidden_states()[0]` would hold - (1, n, H) for a GRU, the pair (h, c) of them for an LSTM - with a
        pending reset applied; None before the first step (and for a policy without a memory)."""
        if not self.hidden or self._state is None or self._fresh:
            return None
        keep = None if self._dones is None else (self._dones == 0).to(torch.float32)[:, None]
        out = tuple((t if keep is None else t * keep).unsqueeze(0) for t in self._state[self._cur])
        return out if self.lstm else out[0]

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self


def _check_memory(name: str, rnn) -> list:
    """The four parameters of a memory the kernels serve, as the step reads them in place."""
    if not rnn.bias or rnn.bidirectional or getattr(rnn, "proj_size", 0) or rnn.dropout:
        raise ValueError(f"{name}: the memory must be a unidirectional rnn with biases, without projection or dropout")
    params = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]
    if any(t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t in params):
        raise ValueError(f"{name}: every parameter of the memory must be a contiguous float32 CUDA tensor")
    return params


class FusedRecurrentPolicy(_MemoryState):
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
        self._params = _check_memory("FusedRecurrentPolicy", rnn)
        self.device = self._params[0].device
        self.hidden, self.obs_dim, self.actions_dim = d.rnn_hidden, d.obs_dim, self.mlp.out_features
        self.launches = lib.lt_policy_step_launches(ctypes.byref(d), 1)
        self._init_state()
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

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        """Mean actions [n][num_actions] of one env step; the memory state advances.  `obs` may be a column slice of wider rows (unit
        column stride): read in place."""
        self._check_obs(obs)
        n = obs.shape[0]
        src, dst = self._step_buffers(n)
        actions = torch.empty(n, self.actions_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.call("lt_policy_step", self.desc, self._mem, self.mlp.packed, obs, max(obs.stride(0), self.obs_dim) if n > 1 else self.obs_dim,
                      self._dones, src[0], src[1] if self.lstm else None, dst[0], dst[1] if self.lstm else None, n, actions,
                      _abi.stream(self.device))
        self._cur ^= 1
        self._dones = None
        return actions


class FusedEncoderPolicy(_MemoryState):
    """One env step of an `ActorCriticRNNEncoder` (two launches) or an `ActorCriticEncoder` (one) through `lt_policy_encoder_step`.
    Every parameter is read in place, in torch's layout, by every step: nothing is packed.  The normaliser's statistics are a snapshot
    `refresh()` takes (a consistent pair, whatever a later update does to the module's own)."""

    def __init__(self, actor_critic, normalizer=None, obs_dim: int | None = None):
        from . import encoder

        ac, name = actor_critic, "FusedEncoderPolicy"
        if type(ac) not in (ActorCriticEncoder, ActorCriticRNNEncoder):
            raise ValueError(f"{name}: actor_critic must be an ActorCriticEncoder or an ActorCriticRNNEncoder, got {type(ac).__name__}")
        if normalizer is not None and not isinstance(normalizer, EmpiricalNormalization):
            raise ValueError(f"{name}: normalizer must be an EmpiricalNormalization or None, got {type(normalizer).__name__}")
        self.actor_critic, self.normalizer = ac, normalizer
        self.recurrent = type(ac) is ActorCriticRNNEncoder
        flat, tail = ac.actor_flatten_obs_dim, ac.actor_encoder_obs_dim
        if obs_dim is None and normalizer is not None:
            obs_dim = normalizer._mean.numel()
        self._obs_dim_known = obs_dim is not None  # else: the first rows tell (the module keeps the two widths, not the row's)
        self.obs_dim = int(obs_dim) if self._obs_dim_known else max(flat, tail)
        try:
            enc, self._enc_linears = encoder.describe(ac.actor_encoder, self.obs_dim, flat, tail=False)
        except ValueError as e:
            raise ValueError(f"{name}: actor_encoder: {e}") from None
        try:
            act, self._actor_linears = encoder.describe(ac.actor, flat + self._enc_linears[-1].out_features, 0, tail=False)
        except ValueError as e:
            raise ValueError(f"{name}: actor: {e}") from None
        if act.final_activation != _abi.CONSTS["LT_ACT_NONE"]:
            raise ValueError(f"{name}: actor: no activation may follow the last layer")
        if self._actor_linears[0].in_features != flat + self._enc_linears[-1].out_features:
            raise ValueError(f"{name}: the actor reads {self._actor_linears[0].in_features} columns, its encoder's rows have "
                             f"{flat + self._enc_linears[-1].out_features}")
        d = _abi.LtPolicyEncoderDesc()
        rnn = ac.memory_a.rnn if self.recurrent else None
        if rnn is not None:
            self.lstm = isinstance(rnn, nn.LSTM)
            d.rnn_type = _abi.LT_POLICY_RNN_LSTM if self.lstm else _abi.LT_POLICY_RNN_GRU
            d.rnn_layers, d.rnn_hidden = rnn.num_layers, rnn.hidden_size
            if rnn.input_size != tail or self._enc_linears[0].in_features != rnn.hidden_size:
                raise ValueError(f"{name}: the memory reads {rnn.input_size} of {tail} tail columns, the encoder {self._enc_linears[0].in_features} "
                                 f"of {rnn.hidden_size} hidden units")
        else:
            d.rnn_type, d.rnn_layers, d.rnn_hidden = _abi.LT_POLICY_ENCODER_NO_MEMORY, 0, 0
            if self._enc_linears[0].in_features != tail:
                raise ValueError(f"{name}: the encoder reads {self._enc_linears[0].in_features} of {tail} tail columns")
        d.obs_dim, d.flat_dim, d.tail_dim = self.obs_dim, flat, tail
        d.enc_layers, d.enc_activation, d.enc_final_activation = enc.num_layers, enc.activation, enc.final_activation
        d.actor_layers, d.actor_activation = act.num_layers, act.activation
        for l in range(enc.num_layers):
            d.enc_dims[l] = enc.dims[l]
        for l in range(act.num_layers):
            d.actor_dims[l] = act.dims[l]
        self.desc = d
        self._validate()
        self._mem_params = _check_memory(name, rnn) if rnn is not None else []
        linears = self._enc_linears + self._actor_linears
        if any(t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for m in linears for t in (m.weight, m.bias)):
            raise ValueError(f"{name}: every parameter of the encoder and the actor must be a contiguous float32 CUDA tensor")
        self.device = linears[0].weight.device
        self.hidden, self.embedding_dim, self.actions_dim = d.rnn_hidden, enc.dims[enc.num_layers - 1], act.dims[act.num_layers - 1]
        self._init_state()
        self.refresh()

    def _validate(self) -> None:
        lib = _abi.load()
        if lib.lt_policy_encoder_validate(ctypes.byref(self.desc)) != 0:
            raise ValueError(f"FusedEncoderPolicy: {lib.lt_last_error().decode()}")
        self.launches = lib.lt_policy_encoder_step_launches(ctypes.byref(self.desc), 1)

    @classmethod
    def for_actor_critic(cls, actor_critic, normalizer=None, obs_dim: int | None = None) -> "FusedEncoderPolicy":
        """The fused front of `actor_critic`; ValueError (the validator's message) for what the kernels do not serve.  `obs_dim`: the
        width of an observation row, where neither a normaliser nor the first rows are to tell it."""
        return cls(actor_critic, normalizer, obs_dim)

    def refresh(self) -> None:
        """Re-read where the parameters live and take a new snapshot of the normaliser's statistics: call after the module or the
        normaliser changed (stream-ordered, no host read).  In-place changes of a parameter need no call: every step reads them."""
        p = _abi.LtPolicyEncoderParams()
        if self._mem_params:
            p.w_ih, p.w_hh, p.b_ih, p.b_hh = (t.data_ptr() for t in self._mem_params)
        for l, m in enumerate(self._enc_linears):
            p.enc_weight[l], p.enc_bias[l] = m.weight.data_ptr(), m.bias.data_ptr()
        for l, m in enumerate(self._actor_linears):
            p.actor_weight[l], p.actor_bias[l] = m.weight.data_ptr(), m.bias.data_ptr()
        if self.normalizer is not None:
            nz = self.normalizer
            if nz._mean.numel() != self.obs_dim:
                raise ValueError(f"FusedEncoderPolicy: the normaliser holds {nz._mean.numel()} columns, the rows have {self.obs_dim}")
            self._norm = tuple(t.detach().reshape(-1).to(self.device, torch.float32, copy=True) for t in (nz._mean, nz._std))
            p.norm_mean, p.norm_std, p.norm_eps = self._norm[0].data_ptr(), self._norm[1].data_ptr(), float(self.normalizer.eps)
        self._params = p

    def __call__(self, obs: torch.Tensor, embedding_out: torch.Tensor | None = None) -> torch.Tensor:
        """Mean actions [n][num_actions] of one env step; the memory state (if any) advances.  `obs` may be a column slice of wider rows
        (unit column stride): read in place.  `embedding_out`: a contiguous f32 [n][embedding_dim] tensor that receives the embedding."""
        if not self._obs_dim_known and isinstance(obs, torch.Tensor) and obs.dim() == 2:
            self.obs_dim = self.desc.obs_dim = int(obs.shape[1])
            self._validate()
            self._obs_dim_known = True
        self._check_obs(obs)
        n = obs.shape[0]
        if embedding_out is not None and (embedding_out.dtype != torch.float32 or embedding_out.device != self.device
                                          or embedding_out.shape != (n, self.embedding_dim) or not embedding_out.is_contiguous()):
            raise ValueError(f"FusedEncoderPolicy: embedding_out must be a contiguous float32 [n][{self.embedding_dim}] tensor on {self.device}")
        src, dst = self._step_buffers(n) if self.hidden else ((None, None), (None, None))
        actions = torch.empty(n, self.actions_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.call("lt_policy_encoder_step", self.desc, self._params, obs, max(obs.stride(0), self.obs_dim) if n > 1 else self.obs_dim,
                      self._dones, src[0], src[1] if self.lstm else None, dst[0], dst[1] if self.lstm else None, n, actions, embedding_out,
                      _abi.stream(self.device))
        self._cur ^= 1
        self._dones = None
        return actions
