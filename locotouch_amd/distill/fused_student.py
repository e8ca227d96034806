"""Opt-in inference front of the student: one env step through `lt_student_step` (include/lt_student.h, csrc/lt_student.hip) -
three HIP launches instead of the ~25 library launches of `Student.forward`.

`FusedStudent(student)` reads the parameters of a `Student` (it owns none) and offers the call surface of the collection loops:
`__call__(proprioception, tactile)`, `reset(dones=None)`, `get_hidden_states()`, `eval()` / `train()`.  `refresh()` re-packs the
parameters after the module was trained.  An architecture the kernels do not serve raises `ValueError` with the validator's
message - there is no fall-back to the eager path.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from .. import _abi
from ..rl.cnn_train import fill_conv_stack
from ..rl.models import MLP, RNN, CNN2dHead

_ACT = {nn.ELU: "LT_ACT_ELU", nn.ReLU: "LT_ACT_RELU", nn.Tanh: "LT_ACT_TANH"}


def _mlp_desc(mlp: MLP, what: str):
    """(lt_mlp_desc, linears) of an `MLP` (Linear layers with ONE activation between, none behind the last)."""
    mods = list(mlp.model)
    linears = [m for m in mods if isinstance(m, nn.Linear)]
    acts = [m for m in mods if not isinstance(m, nn.Linear)]
    if len(linears) > _abi.CONSTS["LT_MLP_MAX_LAYERS"] or mods[-1] is not linears[-1] or len(acts) != len(linears) - 1:
        raise ValueError(f"FusedStudent: {what}: more than LT_MLP_MAX_LAYERS layers, or an activation behind the last layer")
    kinds = {type(m) for m in acts}
    if len(kinds) > 1 or any(k not in _ACT for k in kinds) or any(isinstance(m, nn.ELU) and m.alpha != 1.0 for m in acts):
        raise ValueError(f"FusedStudent: {what}: activation {sorted(k.__name__ for k in kinds)} is not served")
    d = _abi.LtMlpDesc()
    d.num_layers = len(linears)
    d.dims[0] = linears[0].in_features
    for i, lin in enumerate(linears):
        d.dims[i + 1] = lin.out_features
    d.activation = _abi.CONSTS[_ACT[kinds.pop()]] if kinds else _abi.CONSTS["LT_ACT_ELU"]
    d.input_format = _abi.CONSTS["LT_ROWS_F32"]
    return d, linears


def describe(student):
    """(lt_student_desc, [parameter tensors in lt_student_params order as a dict]) of a `Student`; ValueError for what the
    descriptor cannot express.  What it can express but the kernels do not serve is refused by `lt_student_validate`."""
    pre, enc, bb = getattr(student, "pre_encoder", None), student.student_encoder, student.student_backbone
    if not isinstance(pre, CNN2dHead) or not isinstance(enc, RNN) or not isinstance(bb, MLP):
        raise ValueError("FusedStudent: the fused step serves pre_encoder CNN2dHead -> student_encoder RNN -> student_backbone MLP")
    d = _abi.LtStudentDesc()
    d.img_channels, d.img_height, d.img_width = (int(v) for v in student.tactile_signal_img_shape)
    convs, head = fill_conv_stack(d, pre, "FusedStudent: pre_encoder")
    rnn = enc.memory.rnn
    d.rnn_type = _abi.LT_STUDENT_RNN_GRU if isinstance(rnn, nn.GRU) else _abi.LT_STUDENT_RNN_LSTM
    d.rnn_layers, d.rnn_hidden = rnn.num_layers, rnn.hidden_size
    d.encoder, enc_lin = _mlp_desc(enc.mlp, "student_encoder.mlp")
    d.backbone, bb_lin = _mlp_desc(bb, "student_backbone")
    d.proprio_dim = int(student.proprioception_dim)
    tensors = dict(conv_w=[c.weight for c in convs], conv_b=[c.bias for c in convs], head_w=head.weight, head_b=head.bias,
                   gru_w_ih=rnn.weight_ih_l0, gru_w_hh=rnn.weight_hh_l0, gru_b_ih=getattr(rnn, "bias_ih_l0", None),
                   gru_b_hh=getattr(rnn, "bias_hh_l0", None), enc_w=[l.weight for l in enc_lin], enc_b=[l.bias for l in enc_lin],
                   bb_w=[l.weight for l in bb_lin], bb_b=[l.bias for l in bb_lin])
    return d, tensors


class FusedStudent:
    def __init__(self, student):
        self.student = student
        self.desc, self._tensors = describe(student)
        lib = _abi.load()
        if lib.lt_student_validate(ctypes.byref(self.desc)) != 0:
            raise ValueError(f"FusedStudent: {lib.lt_last_error().decode()}")
        flat = [t for v in self._tensors.values() for t in (v if isinstance(v, list) else [v])]
        if any(t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t in flat):
            raise ValueError("FusedStudent: every parameter must be a contiguous float32 CUDA tensor (convolutions, head and GRU with bias)")
        self.device = flat[0].device
        self.hidden, self.actions_dim = self.desc.rnn_hidden, self.desc.backbone.dims[self.desc.backbone.num_layers]
        self.tactile_dim = self.desc.img_channels * self.desc.img_height * self.desc.img_width
        size = ctypes.c_size_t()
        _abi.call("lt_student_packed_floats", self.desc, ctypes.byref(size))
        self.packed = torch.empty(size.value, dtype=torch.float32, device=self.device)
        self.launches = lib.lt_student_step_launches(ctypes.byref(self.desc), 1)
        self._h = self._ws = self._zero_h = None
        self._dones = None      # the mask `reset(dones)` stored: applied by the next step, inside the GRU launch
        self._fresh = True      # no state yet / reset(): the next step starts from zeros
        self.refresh()

    @classmethod
    def for_student(cls, student) -> "FusedStudent":
        """The fused front of `student`; ValueError (the validator's message) for an architecture the kernels do not serve."""
        return cls(student)

    def refresh(self) -> None:
        """Re-pack the module's parameters (one launch, no host read): call after every update of the `Student`."""
        p = _abi.LtStudentParams()
        for name, v in self._tensors.items():
            if isinstance(v, list):
                for i, t in enumerate(v):
                    getattr(p, name)[i] = t.data_ptr()
            else:
                setattr(p, name, v.data_ptr())
        with torch.cuda.device(self.device):
            _abi.call("lt_student_pack", self.desc, p, self.packed, _abi.stream(self.device))

    def _buffers(self, n: int) -> None:
        if self._h is None or self._h.shape[0] != n:
            size = ctypes.c_size_t()
            _abi.call("lt_student_ws_floats", self.desc, n, ctypes.byref(size))
            self._h = torch.zeros(n, self.hidden, dtype=torch.float32, device=self.device)
            self._ws = torch.empty(size.value, dtype=torch.float32, device=self.device)
            self._dones, self._fresh = None, True

    def __call__(self, proprioception: torch.Tensor, tactile_signal: torch.Tensor) -> torch.Tensor:
        """Actions [n][12] of one env step; the hidden state advances.  `proprioception` may be a column slice of wider rows
        (the env's zero-copy policy rows) and `tactile_signal` any [n][442]-like view with unit column stride: read in place."""
        for name, x, width in (("proprioception", proprioception, self.desc.proprio_dim), ("tactile_signal", tactile_signal, self.tactile_dim)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.device != self.device:
                raise TypeError(f"FusedStudent: {name} must be a float32 tensor on {self.device}")
            if x.dim() != 2 or x.shape[1] != width or (x.shape[1] > 1 and x.stride(1) != 1) or x.shape[0] != proprioception.shape[0]:
                raise ValueError(f"FusedStudent: {name} must be [n][{width}] with unit column stride, got {tuple(x.shape)} strides {x.stride()}")
        n = proprioception.shape[0]
        self._buffers(n)
        if self._fresh:
            self._h.zero_()
            self._fresh = False
        actions = torch.empty(n, self.actions_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.call("lt_student_step", self.desc, self.packed, proprioception, proprioception.stride(0), tactile_signal, tactile_signal.stride(0),
                      self._dones, self._h, n, actions, self._ws, _abi.stream(self.device))
        self._dones = None
        return actions

    def reset(self, dones=None) -> None:
        """`Student.reset`: None forgets the state; a per-env mask is STORED and zeroes those rows inside the next step (no launch
        for a bool / uint8 mask; the tensor must stay unchanged until that step)."""
        if dones is None:
            self._fresh, self._dones = True, None
            return
        if self._h is None or self._fresh:
            return
        d = dones.reshape(-1)
        if d.dtype not in (torch.bool, torch.uint8) or not d.is_contiguous():
            d = (d != 0).contiguous()
        if d.shape[0] != self._h.shape[0] or d.device != self.device:
            raise ValueError("FusedStudent.reset: one mask entry per env, on the student's device")
        if self._dones is not None:  # two resets without a step between them
            d = d.to(torch.bool) | self._dones.to(torch.bool)
        self._dones = d

    def get_hidden_states(self):
        """(1, n, H) like `Memory.get_hidden_states`, with a pending reset applied; None before the first step."""
        if self._h is None or self._fresh:
            return None
        h = self._h if self._dones is None else self._h * (self._dones == 0).to(self._h.dtype)[:, None]
        return h.unsqueeze(0)

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self

    def extract_input_and_forward(self, obs):
        return self(obs["policy"][:, :self.desc.proprio_dim], obs["tactile"])
