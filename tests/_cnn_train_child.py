"""Child of tests/test_hip_cnn_train.py::test_launch_count: ONE lt_cnn_forward and ONE lt_cnn_backward of the registered stack at the n given
on the command line, in a process of its own so that a kernel trace of it counts exactly these launches."""
import ctypes
import sys

import torch

from locotouch_amd import _abi
from locotouch_amd.rl.cnn_train import _pointers, describe_cnn
from locotouch_amd.rl.models import CNN2dHead


def main(n: int) -> None:
    torch.manual_seed(0)
    head = CNN2dHead((2, 17, 13), (24, 24, 24), (4, 3, 2), (2, 1, 1), None, None, 64, "relu", True).cuda()
    desc, params = describe_cnn(head, (2, 17, 13))
    params = [p.detach() for p in params]
    x, d_emb, emb = torch.randn(n, 442, device="cuda"), torch.randn(n, 64, device="cuda"), torch.empty(n, 64, device="cuda")
    grads = [torch.empty_like(p) for p in params]
    size = ctypes.c_size_t()
    _abi.call("lt_cnn_ws_floats", desc, n, ctypes.byref(size))
    ws = torch.empty(size.value, device="cuda")
    _abi.call("lt_cnn_forward", desc, _pointers(_abi.LtCnnParams(), 3, params), x, n, emb, ws, _abi.stream())
    _abi.call("lt_cnn_backward", desc, _pointers(_abi.LtCnnParams(), 3, params), x, d_emb, n, _pointers(_abi.LtCnnGrads(), 3, grads), ws, _abi.stream())
    torch.cuda.synchronize()
    lib = _abi.load()
    print("LAUNCHES", lib.lt_cnn_launches(ctypes.byref(desc), n, 0), lib.lt_cnn_launches(ctypes.byref(desc), n, 1), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]))
