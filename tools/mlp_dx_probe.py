"""dx hop: the kernel of csrc/lt_mlp_dx.hip against unsplit + torch.mm, on the benchmark's shape (24576 rows, 256 -> [512, 256, 128] -> 12 | 1)."""
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locotouch_amd.rl import mlp as M  # noqa: E402

H, m = 256, 24576
torch.manual_seed(0)


def stack(out):
    return nn.Sequential(nn.Linear(H, 512), nn.ELU(), nn.Linear(512, 256), nn.ELU(), nn.Linear(256, 128), nn.ELU(), nn.Linear(128, out)).cuda()


actor, critic = stack(12), stack(1)
pair = M.PackedPair(actor, critic)
xs = [torch.tanh(torch.randn(m, H, device="cuda")) for _ in range(2)]
dys = [torch.randn(m, 12, device="cuda") * 1e-4, torch.randn(m, 1, device="cuda") * 1e-4]
amax = (dys[0].abs().max().reshape(1), dys[1].abs().max().reshape(1))
grads = {p: torch.zeros_like(p) for net in (actor, critic) for p in net.parameters()}
dx = tuple(torch.empty_like(x) for x in xs)


def once(kernel, with_dx):
    M.USE_DX_KERNEL = kernel
    _, acts = pair.forward_raw(*xs, with_dx=with_dx)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    pair.backward_raw(*xs, acts, *dys, grads, dy_amax=amax, dx_out=dx if with_dx else None)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


res = {"kernel": [], "library": [], "no_dx": []}
for it in range(40):
    for name, args in (("kernel", (True, True)), ("library", (False, True)), ("no_dx", (True, False))):
        t = once(*args)
        if it >= 10:
            res[name].append(t)
out = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds": len(v)} for k, v in res.items()}
out["what"] = "PackedPair.backward_raw of both stacks, device events, 30 alternating rounds behind 10 of warm-up; no_dx: without the input gradients"
print("RESULT " + json.dumps(out))
