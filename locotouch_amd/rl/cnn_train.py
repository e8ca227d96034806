"""Opt-in training front of the tactile CNN head: `CNN2dHead` forward and backward through `lt_cnn_forward` / `lt_cnn_backward`
(include/lt_cnn_train.h, csrc/lt_cnn_train.hip) - direct-convolution HIP kernels that recompute the maps in the backward pass
instead of `Conv2dAsGemm`'s dense GEMMs and autograd's saved maps.

`CNN2dHead.enable_fused_training(img_shape)` switches a module over; a stack the kernels do not serve raises `ValueError` with the
validator's message - there is no fall-back to the module path.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from .. import _abi


def fill_conv_stack(d, pre, who: str):
    """Fills the conv-stack fields of a descriptor (lt_student_desc / lt_cnn_desc: the same names) but the image shape from a
    `CNN2dHead`; returns (convolutions, head Linear).  ValueError, starting with `who`, for what the fields cannot express."""
    from .models import MLP

    mods = list(pre.conv.conv)
    convs = [m for m in mods if isinstance(m, nn.Conv2d)]
    pools = {}
    if len(convs) > _abi.LT_STUDENT_MAX_CONVS:
        raise ValueError(f"{who}: more than LT_STUDENT_MAX_CONVS convolutions")
    d.num_convs = len(convs)
    ci = -1
    for m in mods:
        if isinstance(m, nn.Conv2d):
            ci += 1
        elif isinstance(m, nn.MaxPool2d):
            pools[ci] = int(m.kernel_size if isinstance(m.kernel_size, int) else m.kernel_size[0])
        elif isinstance(m, nn.ReLU):
            d.conv_activation = _abi.CONSTS["LT_ACT_RELU"]
        else:  # another activation, a norm layer, anything else: not served, and said by name
            raise ValueError(f"{who}: {type(m).__name__} in the conv stack is not served (Conv2d, ReLU and MaxPool2d are)")
    d.use_maxpool = int(bool(pools))
    for i, c in enumerate(convs):
        if c.kernel_size[0] != c.kernel_size[1] or c.stride[0] != c.stride[1] or c.padding[0] != c.padding[1] or c.dilation != (1, 1) or c.groups != 1:
            raise ValueError(f"{who}: square kernels, equal strides / paddings, no dilation and no groups are served")
        if pools and c.stride[0] != 1:
            raise ValueError(f"{who}: a strided convolution beside max-pools is not served")
        d.conv_channels[i], d.conv_kernel[i], d.conv_padding[i] = c.out_channels, c.kernel_size[0], c.padding[0]
        d.conv_stride[i] = pools.get(i, 1) if pools else c.stride[0]
    if not isinstance(pre.head, MLP) or len([m for m in pre.head.model if isinstance(m, nn.Linear)]) != 1:
        raise ValueError(f"{who}.head: one Linear layer is served")
    head = pre.head.model[0]
    d.head_out = head.out_features
    return convs, head


def describe_cnn(head, img_shape):
    """(lt_cnn_desc, parameter tensors in lt_cnn_params order: conv weights, conv biases, head weight, head bias) of a `CNN2dHead`."""
    d = _abi.LtCnnDesc()
    d.img_channels, d.img_height, d.img_width = (int(v) for v in img_shape)
    convs, lin = fill_conv_stack(d, head, "CNN2dHead.enable_fused_training")
    return d, [c.weight for c in convs] + [c.bias for c in convs] + [lin.weight, lin.bias]


def _pointers(struct, nconv: int, tensors):
    """lt_cnn_params / lt_cnn_grads over `tensors` (the order of `describe_cnn`)."""
    for i in range(nconv):
        struct.conv_w[i], struct.conv_b[i] = tensors[i].data_ptr(), tensors[nconv + i].data_ptr()
    struct.head_w, struct.head_b = tensors[2 * nconv].data_ptr(), tensors[2 * nconv + 1].data_ptr()
    return struct


def _workspace(desc, n: int, device) -> torch.Tensor:
    size = ctypes.c_size_t()
    _abi.call("lt_cnn_ws_floats", desc, n, ctypes.byref(size))
    return torch.empty(size.value, dtype=torch.float32, device=device)


class _CnnHeadHip(torch.autograd.Function):
    """emb [N][head_out] of x2d [N][C H W]; saves x2d and the parameters only (the backward recomputes every map)."""

    @staticmethod
    def forward(ctx, desc, x2d, *params):
        if x2d.requires_grad:
            raise ValueError("CNN2dHead (fused training): the tactile input is data - the kernels have no input gradient")
        x2d = x2d.detach().contiguous()
        params = [p.detach() for p in params]
        if any(p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() for p in params) or x2d.dtype != torch.float32:
            raise ValueError("CNN2dHead (fused training): input and parameters must be contiguous float32 CUDA tensors")
        n = x2d.shape[0]
        emb = torch.empty(n, desc.head_out, dtype=torch.float32, device=x2d.device)
        with torch.cuda.device(x2d.device):
            ws = _workspace(desc, 1, x2d.device)  # the forward touches the packed weights only
            _abi.call("lt_cnn_forward", desc, _pointers(_abi.LtCnnParams(), desc.num_convs, params), x2d, n, emb, ws, _abi.stream(x2d.device))
        ctx.desc = desc
        ctx.save_for_backward(x2d, *params)
        return emb

    @staticmethod
    def backward(ctx, d_emb):
        x2d, *params = ctx.saved_tensors
        desc, n = ctx.desc, x2d.shape[0]
        grads = [torch.empty_like(p) for p in params]
        with torch.cuda.device(x2d.device):
            ws = _workspace(desc, n, x2d.device)
            _abi.call("lt_cnn_backward", desc, _pointers(_abi.LtCnnParams(), desc.num_convs, params), x2d, d_emb.contiguous(), n,
                      _pointers(_abi.LtCnnGrads(), desc.num_convs, grads), ws, _abi.stream(x2d.device))
        return (None, None, *grads)


def enable(head, img_shape) -> None:
    """`CNN2dHead.enable_fused_training`: validate, then route training forwards through `_CnnHeadHip`."""
    desc, tensors = describe_cnn(head, img_shape)
    lib = _abi.load()
    if lib.lt_cnn_validate(ctypes.byref(desc)) != 0:
        raise ValueError(f"CNN2dHead.enable_fused_training: {lib.lt_last_error().decode()}")
    if any(t is None or t.dtype != torch.float32 or not t.is_cuda for t in tensors):
        raise ValueError("CNN2dHead.enable_fused_training: every parameter must be a float32 CUDA tensor (convolutions and head with bias)")
    head._fused_cnn = desc


def forward(head, x):
    """The fused forward of an enabled head for [N, C, H, W] or [N, C H W] input."""
    desc, tensors = describe_cnn(head, (head._fused_cnn.img_channels, head._fused_cnn.img_height, head._fused_cnn.img_width))
    if bytes(desc) != bytes(head._fused_cnn):
        raise ValueError("CNN2dHead (fused training): the conv stack changed since enable_fused_training")
    return _CnnHeadHip.apply(desc, x.reshape(x.shape[0], -1), *tensors)  # the module's parameters as they are NOW
