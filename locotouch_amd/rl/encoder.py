"""The encoder in front of an `ActorCriticEncoder`'s stacks on the HIP library (include/lt_encoder.h, csrc/lt_encoder.hip): one launch
writes `[ obs[:, :flat_dim] | enc(obs[:, -enc_in:]) ]` for the actor and, when it has an encoder, the critic.  The kernel reads the live
`nn.Linear` parameters: nothing is packed, so there is nothing to refresh after an optimizer step.

`EncoderPair` holds the descriptors of a policy's encoders; `forward(obs, critic_obs, out, critic_out, acts=...)` is the launch - the
rollout's form without `acts`, the update's with them (the activation behind every hidden layer and, with a final activation, the
pre-activation embedding: what `rl/mlp.py::backward_chain` and the final activation's derivative read).

`RnnEncoderPair` is the same for an `ActorCriticRNNEncoder`, whose encoders read the output rows of a memory (include/lt_rnn_encoder.h):
`forward` in the rollout, and for `PPO._direct_rnn_encoder_update` `forward_train` and `backward` (include/lt_rnn_encoder_train.h: one
launch from the gradient of the stacks' input rows to every layer's dz and the gradient of the memory's output).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _abi

_ACT_IDS = {nn.ELU: "LT_ACT_ELU", nn.ReLU: "LT_ACT_RELU", nn.Tanh: "LT_ACT_TANH"}


def make_desc(obs_dim: int, flat_dim: int, enc_in: int, dims, activation: int, final_activation: int):
    """LtEncoderDesc of an encoder with layer outputs `dims` (the last one is the embedding width); nothing is checked here."""
    d = _abi.LtEncoderDesc()
    d.obs_dim, d.flat_dim, d.enc_in, d.num_layers = int(obs_dim), int(flat_dim), int(enc_in), len(dims)
    for l, w in enumerate(list(dims)[:_abi.ENCODER_CONSTS["LT_ENCODER_MAX_LAYERS"]]):
        d.dims[l] = int(w)
    d.activation, d.final_activation = int(activation), int(final_activation)
    return d


def validate(desc) -> str | None:
    """None for a descriptor the kernel serves, else the library's refusal text (host only)."""
    import ctypes

    lib = _abi.load()
    if lib.lt_encoder_validate(ctypes.byref(desc)) == 0:
        return None
    return lib.lt_last_error().decode()


def make_net(desc, obs: torch.Tensor, weights, biases, out: torch.Tensor, acts=None, obs_stride: int | None = None):
    """LtEncoderNet of one network: `obs` rows read in place (`obs_stride` floats apart; default: the tensor's own row stride)."""
    net = _abi.LtEncoderNet()
    net.desc = desc
    net.obs = obs.data_ptr()
    net.obs_stride = int(obs.stride(0) if obs_stride is None else obs_stride)
    for l, (w, b) in enumerate(zip(weights, biases)):
        net.weight[l], net.bias[l] = w.data_ptr(), b.data_ptr()
    net.out = out.data_ptr()
    for l, a in enumerate(acts or ()):
        net.acts[l] = None if a is None else a.data_ptr()
    return net


def describe(enc: nn.Module, obs_dim: int, flat_dim: int, tail: bool = True):
    """(LtEncoderDesc, [Linear...]) of an `MLP` encoder module (rl/models.py) reading the last `in_features` of `obs_dim` columns;
    ValueError naming the reason for a module the kernel does not serve.  `tail=False`: the encoder reads another array than the row
    (`RnnEncoderPair`), so the library's check of the widths is the caller's to ask."""
    mods = list(enc.model) if hasattr(enc, "model") else list(enc)
    linears = [m for m in mods if isinstance(m, nn.Linear)]
    if not linears or any(m.bias is None or m.weight.dtype != torch.float32 or not m.weight.is_contiguous() for m in linears):
        raise ValueError("the encoder must be a stack of contiguous f32 Linear layers with biases")
    C = _abi.CONSTS
    acts, final, i = set(), C["LT_ACT_NONE"], 0
    for l, lin in enumerate(linears):  # Linear, activation, ..., Linear[, final activation]
        if i >= len(mods) or mods[i] is not lin:
            raise ValueError("the encoder must be Linear layers with one activation between them")
        i += 1
        last = l == len(linears) - 1
        if i < len(mods) and not isinstance(mods[i], nn.Linear):
            a = mods[i]
            if type(a) not in _ACT_IDS or (type(a) is nn.ELU and a.alpha != 1.0):
                raise ValueError(f"encoder activation {type(a).__name__} is not served (ELU with alpha 1, ReLU, Tanh)")
            if last:
                final = C[_ACT_IDS[type(a)]]
            else:
                acts.add(type(a))
            i += 1
        elif not last:
            raise ValueError("an activation must follow every hidden layer of the encoder")
    if i != len(mods) or len(acts) > 1:
        raise ValueError("the encoder must be Linear layers with one activation between them")
    if any(a.out_features != b.in_features for a, b in zip(linears[:-1], linears[1:])):
        raise ValueError("the encoder's layers do not chain")
    if len(linears) > _abi.ENCODER_CONSTS["LT_ENCODER_MAX_LAYERS"]:
        raise ValueError("the encoder has more than LT_ENCODER_MAX_LAYERS layers")
    act = C[_ACT_IDS[next(iter(acts))]] if acts else C["LT_ACT_ELU"]  # (a single Linear has no hidden activation: any served id)
    desc = make_desc(obs_dim, flat_dim, linears[0].in_features, [m.out_features for m in linears], act, final)
    why = validate(desc) if tail else None
    if why is not None:
        raise ValueError(why)
    return desc, linears


class EncoderPair:
    """The encoders of an `ActorCriticEncoder` as one launch: the actor's and, when `ac.critic_with_encoder`, the critic's."""

    def __init__(self, ac, obs_dim: int, critic_obs_dim: int):
        self.a_desc, self.a_linears = describe(ac.actor_encoder, obs_dim, ac.actor_flatten_obs_dim)
        self.a_width = ac.actor_flatten_obs_dim + self.a_linears[-1].out_features
        if self.a_width != ac.actor[0].in_features:
            raise ValueError(f"the actor reads {ac.actor[0].in_features} columns, its encoder's rows have {self.a_width}")
        self.c_desc = self.c_linears = None
        self.c_width = critic_obs_dim
        if ac.critic_with_encoder:
            self.c_desc, self.c_linears = describe(ac.critic_encoder, critic_obs_dim, ac.critic_flatten_obs_dim)
            self.c_width = ac.critic_flatten_obs_dim + self.c_linears[-1].out_features
            if self.c_width != ac.critic[0].in_features:
                raise ValueError(f"the critic reads {ac.critic[0].in_features} columns, its encoder's rows have {self.c_width}")

    @staticmethod
    def _acts(desc, n, device):
        """The training form's buffers of one network: hidden activations, then the pre-activation embedding if a final activation is set."""
        count = desc.num_layers if desc.final_activation != _abi.CONSTS["LT_ACT_NONE"] else desc.num_layers - 1
        return [torch.empty(n, desc.dims[l], device=device, dtype=torch.float32) for l in range(count)]

    def forward(self, obs, critic_obs, out, critic_out=None, train: bool = False):
        """One launch.  Returns (actor acts, critic acts) in the training form, else (None, None)."""
        n = obs.shape[0]
        for x in (obs, critic_obs if self.c_desc is not None else None):
            if x is not None and (x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1):
                raise ValueError("the encoder reads f32 rows with unit column stride")
        a_acts = self._acts(self.a_desc, n, obs.device) if train else None
        c_acts = self._acts(self.c_desc, n, obs.device) if train and self.c_desc is not None else None
        a = make_net(self.a_desc, obs, [m.weight for m in self.a_linears], [m.bias for m in self.a_linears], out, a_acts)
        c = None
        if self.c_desc is not None:
            c = make_net(self.c_desc, critic_obs, [m.weight for m in self.c_linears], [m.bias for m in self.c_linears], critic_out, c_acts)
        _abi.call("lt_encoder_forward", a, c, n, _abi.stream(obs.device))
        return a_acts, c_acts


class RnnEncoderPair:
    """The encoders of an `ActorCriticRNNEncoder` as one launch (include/lt_rnn_encoder.h): per network
    `[ obs[:, :flat_dim] | enc(h) ]` with `h` the output rows of the network's memory.  Both networks have an encoder."""

    def __init__(self, ac, obs_dim: int, critic_obs_dim: int):
        import ctypes

        if not ac.critic_with_encoder:
            raise ValueError("the critic has no encoder")
        self.nets = []
        for who, enc, mem, stack, dim, flat in (("actor", ac.actor_encoder, ac.memory_a, ac.actor, obs_dim, ac.actor_flatten_obs_dim),
                                                ("critic", ac.critic_encoder, ac.memory_c, ac.critic, critic_obs_dim, ac.critic_flatten_obs_dim)):
            try:
                desc, linears = describe(enc, dim, flat, tail=False)
            except ValueError as e:
                raise ValueError(f"{who}_encoder: {e}") from None
            if desc.enc_in != mem.rnn.hidden_size:
                raise ValueError(f"the {who}'s encoder reads {desc.enc_in} columns, its memory's hidden size is {mem.rnn.hidden_size}")
            width = flat + linears[-1].out_features
            if width != stack[0].in_features:
                raise ValueError(f"the {who} reads {stack[0].in_features} columns, its encoder's rows have {width}")
            self.nets.append((desc, linears, width))
        self.a_width, self.c_width = self.nets[0][2], self.nets[1][2]
        lib = _abi.load()
        if lib.lt_rnn_encoder_forward_launches(ctypes.byref(self._net(0)), ctypes.byref(self._net(1))) != 1:
            raise ValueError(lib.lt_last_error().decode())

    def _net(self, which: int, obs=None, h=None, out=None, acts=()):
        """LtRnnEncoderNet of network `which` (0 actor, 1 critic); without tensors: its widths alone.  `acts`: the training form's buffers."""
        desc, linears, _ = self.nets[which]
        net = _abi.LtRnnEncoderNet()
        net.obs_dim, net.flat_dim, net.enc_in, net.num_layers = desc.obs_dim, desc.flat_dim, desc.enc_in, desc.num_layers
        for l in range(desc.num_layers):
            net.dims[l] = desc.dims[l]
        net.activation, net.final_activation = desc.activation, desc.final_activation
        if obs is not None:
            net.obs, net.obs_stride, net.h, net.h_stride, net.out = obs.data_ptr(), obs.stride(0), h.data_ptr(), h.stride(0), out.data_ptr()
            for l, m in enumerate(linears):
                net.weight[l], net.bias[l] = m.weight.data_ptr(), m.bias.data_ptr()
            for l, a in enumerate(acts):
                net.acts[l] = a.data_ptr()
        return net

    @staticmethod
    def _check_rows(*rows) -> None:
        for x in rows:
            if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
                raise ValueError("the encoder reads f32 rows with unit column stride")

    def forward(self, obs, critic_obs, h_a, h_c, out, critic_out) -> None:
        """One launch, the inference form."""
        self._check_rows(obs, critic_obs, h_a, h_c)
        _abi.call("lt_rnn_encoder_forward", self._net(0, obs, h_a, out), self._net(1, critic_obs, h_c, critic_out), obs.shape[0],
                  _abi.stream(obs.device))

    def forward_train(self, obs, critic_obs, h_a, h_c, out, critic_out):
        """One launch, the training form (include/lt_rnn_encoder_train.h).  Returns (actor acts, critic acts): per network the activation
        behind every hidden layer and, with a final activation, the pre-activation embedding - what `backward` reads."""
        self._check_rows(obs, critic_obs, h_a, h_c)
        n = obs.shape[0]
        acts = [EncoderPair._acts(desc, n, obs.device) for desc, _, _ in self.nets]
        _abi.call("lt_rnn_encoder_forward_train", self._net(0, obs, h_a, out, acts[0]), self._net(1, critic_obs, h_c, critic_out, acts[1]), n,
                  _abi.stream(obs.device))
        return acts[0], acts[1]

    def backward(self, dx, outs, acts, grad_of, hs):
        """From dx = (dx_a, dx_c), the gradients w.r.t. the rows `outs` = (out, critic_out) of `forward_train` (f32, unit column stride, any
        row stride), to (dh_a, dh_c), each [n, enc_in]: the gradients w.r.t. `hs` = (h_a, h_c), the contiguous rows that launch read.  ONE
        launch (`lt_rnn_encoder_backward`) leaves every layer's dz_l and dh; the encoders' weight and bias gradients dW_l = dz_l^T in_l
        (in_0 = h, in_l = acts[l - 1]) and db_l = column sums of dz_l are then written IN PLACE into `grad_of[param]`, by the means
        rl/memory_seq.py `direct_backward` uses."""
        from .memory_seq import _wgrad_into

        self._check_rows(*dx)
        n, dev = dx[0].shape[0], dx[0].device
        grads, dzs, dhs = [], [], []
        for k, (desc, linears, width) in enumerate(self.nets):
            g = _abi.LtRnnEncoderGrad()
            g.flat_dim, g.enc_in, g.num_layers = desc.flat_dim, desc.enc_in, desc.num_layers
            g.activation, g.final_activation = desc.activation, desc.final_activation
            if not outs[k].is_contiguous() or outs[k].shape != (n, width):
                raise ValueError("the encoder's output rows must be the contiguous [n, flat_dim + embedding] array of forward_train")
            g.dx, g.dx_stride, g.out = dx[k].data_ptr(), dx[k].stride(0), outs[k].data_ptr()
            dz = [torch.empty(n, desc.dims[l], device=dev, dtype=torch.float32) for l in range(desc.num_layers)]
            dh = torch.empty(n, desc.enc_in, device=dev, dtype=torch.float32)
            for l, m in enumerate(linears):
                g.dims[l], g.weight[l], g.dz[l] = desc.dims[l], m.weight.data_ptr(), dz[l].data_ptr()
            for l, a in enumerate(acts[k]):
                g.acts[l] = a.data_ptr()
            g.dh = dh.data_ptr()
            grads.append(g)
            dzs.append(dz)
            dhs.append(dh)
        _abi.call("lt_rnn_encoder_backward", grads[0], grads[1], n, _abi.stream(dev))
        with torch.no_grad():
            for k, (desc, linears, _) in enumerate(self.nets):
                ins = [hs[k], *acts[k][:desc.num_layers - 1]]
                for l, m in enumerate(linears):
                    torch.sum(dzs[k][l], dim=0, out=grad_of[m.bias])
                    _wgrad_into(grad_of[m.weight], dzs[k][l], ins[l])
        return dhs[0], dhs[1]
