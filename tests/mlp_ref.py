"""Double-precision references of the fused MLP kernel (locotouch_amd/csrc/lt_mlp.hip) and of the policy head's sampling.

The kernel's forward is an `nn.Sequential` of Linear layers with one activation between them, every layer input saturated to
+-LT_MLP_INPUT_CLAMP (include/lt_env.h, DOMAIN).  `forward64` evaluates that in float64; `forward32` is torch's own fp32 evaluation
of the same modules (the f32 baseline of the ratio rule); `ref_chain` is the f64 backward chain of lt_mlp_backward_pair.  Errors are
reported as {field: (max |cand - ref|, max |ref|, max error as a fraction of REL_BAND * max |ref|)}, the shape
tests/parity_util.f64_ratio_failures takes.
"""
from __future__ import annotations

import numpy as np

from locotouch_amd import _abi

CLAMP = float(_abi.CONSTS["LT_MLP_INPUT_CLAMP"])
REL_BAND = 2e-5  # tests/test_hip_parity.py::test_fused_mlp_matches_torch's tolerance, relative to the field's magnitude


def compiled_instantiations(path: str | None = None) -> set:
    """Every lt_mlp_kernel<RT,KIND,IN> the HIP library holds, read from the mangled kernel symbols in its bytes (lt_mlp_kernel_name's
    spelling).  Host-only."""
    import re

    blob = open(path or _abi.LIB_PATH, "rb").read()
    num = lambda t: -int(t[1:]) if t.startswith("n") else int(t)  # (Itanium mangling writes -1 as n1)
    return {"lt_mlp_kernel<%d,%d,%d>" % tuple(num(g.decode()) for g in m)
            for m in re.findall(rb"13lt_mlp_kernelILi(n?\d+)ELi(n?\d+)ELi(n?\d+)EE", blob)}


def linears(seq):
    import torch.nn as nn

    return [m for m in seq if isinstance(m, nn.Linear)]


def activation(seq):
    """The hidden activation of a Sequential as a function on tensors (identity if there is none)."""
    import torch.nn as nn

    acts = [m for m in seq if not isinstance(m, nn.Linear)]
    return acts[0] if acts else (lambda t: t)


def forward64(seq, x, clamp: bool = True, weights=None):
    """f64: (output, [activation behind hidden layer l]).  `weights`: optional per-layer replacements of the Linear weights."""
    import torch

    lin, act = linears(seq), activation(seq)
    h, acts = x.double(), []
    for l, m in enumerate(lin):
        w = (weights[l] if weights is not None else m.weight).double()
        h = (h.clamp(-CLAMP, CLAMP) if clamp else h) @ w.t() + m.bias.double()
        if l < len(lin) - 1:
            h = act(h)
            acts.append(h)
    return h, acts


def forward32(seq, x):
    """torch's fp32 evaluation of the same modules, the same per-layer saturation: (output, [hidden activations])."""
    import torch

    lin, act = linears(seq), activation(seq)
    h, acts = x.float(), []
    with torch.no_grad():
        for l, m in enumerate(lin):
            h = m(h.clamp(-CLAMP, CLAMP))
            if l < len(lin) - 1:
                h = act(h)
                acts.append(h)
    return h, acts


def split_weights64(seq):
    """The weights as the kernel multiplies them, in f64: hi + lo / 64 with hi = f16(w), lo = f16(64 (w - hi)) (lt_mlp_pack)."""
    import torch

    out = []
    for m in linears(seq):
        w = m.weight.detach().float().clamp(-CLAMP, CLAMP)
        hi = w.half()
        lo = ((w - hi.float()) * 64.0).half()
        out.append(hi.double() + lo.double() / 64.0)
    return out


def ref_chain(seq, x, dy):
    """f64 backward chain of an ELU stack: (dz per hidden layer, dW per layer, db per layer)."""
    import torch

    lin = linears(seq)
    a, acts = x.double(), []
    for l in lin[:-1]:
        a = torch.nn.functional.elu(a @ l.weight.double().t() + l.bias.double())
        acts.append(a)
    g = dy.double()
    dz, dw, db = {}, {}, {}
    L = len(lin)
    for l in range(L - 1, -1, -1):
        inp = acts[l - 1] if l > 0 else x.double()
        if l < L - 1:
            g = g * torch.where(acts[l] > 0, torch.ones_like(acts[l]), acts[l] + 1.0)
            dz[l] = g
        dw[l], db[l] = g.t() @ inp, g.sum(0)
        g = g @ lin[l].weight.double()
    return dz, dw, db


def err(cand, ref) -> tuple:
    """(max |cand - ref|, max |ref|, fraction of REL_BAND * max |ref|) of two tensors / arrays."""
    import torch

    c = cand.double() if isinstance(cand, torch.Tensor) else torch.as_tensor(np.asarray(cand, np.float64))
    r = ref.double() if isinstance(ref, torch.Tensor) else torch.as_tensor(np.asarray(ref, np.float64))
    c, r = c.to(r.device), r
    if not r.numel():
        return (0.0, 0.0, 0.0)
    e, top = float((c - r).abs().max()), float(r.abs().max())
    return (e, top, e / (REL_BAND * top) if top > 0 else 0.0)


def log_normal64(x, mu, sigma):
    """sum over the last axis of log N(x; mu, sigma), f64 - Normal(mu, sigma).log_prob(actions).sum(-1) of the reference (ppo.py:135)."""
    d = (x.double() - mu.double()) / sigma.double()
    return (-0.5 * d * d - sigma.double().log() - 0.5 * np.log(2.0 * np.pi)).sum(-1)


# ---- Philox4x32-10 (oracle/lt_oracle_math.h lt_rng4), vectorised over envs: the policy head's uniforms ------------------------------
def rng4(seed: int, env: np.ndarray, step: int, stream: int) -> np.ndarray:
    """[len(env)][4] float32 uniforms, bit-exact with lt_rng4 / the kernels' rng4."""
    M = np.uint64(0xFFFFFFFF)
    env = np.asarray(env, np.uint64)
    c0, c1 = env & M, np.full_like(env, step & 0xFFFFFFFF)
    c2, c3 = np.full_like(env, stream & 0xFFFFFFFF), np.full_like(env, (step >> 32) & 0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    o = np.stack([c0, c1, c2, c3], axis=1)
    return ((o >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def policy_uniforms(seed: int, n: int, step: int) -> np.ndarray:
    """[n][3][4] float32: the uniforms of action group q of every env (stream 0x400 + q)."""
    e = np.arange(n, dtype=np.uint64)
    return np.stack([rng4(seed, e, step, 0x400 + q) for q in range(3)], axis=1)


def policy_normals32(seed: int, n: int, step: int):
    """torch's fp32 Box-Muller of the same uniforms, [n][12] float32 (the f32 baseline of the sampled fields)."""
    import torch

    u = torch.from_numpy(policy_uniforms(seed, n, step))
    r = torch.sqrt(-2.0 * torch.log(1.0 - u[..., 0::2]))  # [n][3][2]: from u0, u2
    t = 2.0 * np.float32(np.pi) * u[..., 1::2]
    z = torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=-1)  # [n][3][2 (a / c)][2 (cos / sin)]
    return z.reshape(n, 12)
