"""Every instantiation of the fused MLP kernel (locotouch_amd/csrc/lt_mlp.hip) in every mode against float64 (tests/mlp_ref.py).

The kernel must be as close to the f64 answer as torch's own fp32 evaluation of the same modules: per field, e_hip <= F64_RATIO * e_f32 +
F64_ULPS f32 ulps of the field's magnitude (tests/parity_util.f64_ratio_failures, the rule the step kernel is held to).  Each case names
the instantiation it runs (lt_mlp_kernel_name, the function launch() decides with) and the cases together cover every instantiation
compiled into the library.  Modes: lt_mlp_forward; lt_mlp_forward_pair with f32 and split activations, every hidden layer checked;
lt_rollout_policy / lt_rollout_policy_value on a caller-owned step counter (mu, value, the action against mu64 + sigma z64, the log-prob
of the stored action against f64 log N(a; mu64, sigma), sigma bit-equal to std, the draws z against the oracle's f64 twin); the
backward chain of lt_mlp_backward_pair (dz of every hidden layer).  Row counts sit on both sides of the row-tile thresholds, which are
taken from the query."""
import ctypes

import numpy as np
import pytest

from locotouch_amd import _abi
from tests import mlp_ref as R
from tests.parity_util import F64_RATIO, f64_ratio_failures

C = _abi.CONSTS
MODES = {"fwd": C["LT_MLP_MODE_FORWARD"], "pair": C["LT_MLP_MODE_FORWARD"], "policy": C["LT_MLP_MODE_POLICY"],
         "bwd": C["LT_MLP_MODE_BACKWARD"]}
# Per-case, per-field ratio exceptions: measured numbers and a located cause in a comment, capped at 32.  None are needed.
RATIO_EXCEPTIONS: dict = {}
assert all(r <= 32 for ex in RATIO_EXCEPTIONS.values() for r in ex.values())
STD12 = [0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0, 1.2, 1.4]
SEED = 0x5EED_1234_ABCD
Z_TOL = 1e-4  # |z_hip - z64| <= Z_TOL (1 + |z|): Philox keying / row mapping errors are O(1)

# network specs: (input width, hidden widths, outputs, activation, input rows bf16)
A348 = (348, (512, 256, 128), 12, "elu", False)
A270 = (270, (512, 256, 128), 12, "elu", False)
A45 = (45, (64, 40), 12, "elu", False)            # odd input width: run-time staging (IN_ANY); 40 is no multiple of 16
A348_BF16 = (348, (512, 256, 128), 12, "elu", True)
A6 = (348, (256, 256, 136, 128, 72), 12, "elu", False)  # six layers
C348 = (348, (512, 256, 128), 1, "elu", False)
C270 = (270, (512, 256, 128), 1, "elu", False)
C348_BF16 = (348, (512, 256, 128), 1, "elu", True)
C_TANH = (348, (256, 128), 1, "tanh", False)
F33 = (33, (40, 20), 13, "elu", False)
F45_RELU = (45, (64, 64), 7, "relu", False)
F270_TANH = (270, (256, 128, 128), 17, "tanh", False)
F1008 = (1008, (512, 256), 1, "elu", False)       # wide input: four row tiles do not fit the LDS (launch_shape falls back to two)
F6 = (348, (512, 256, 256, 128, 64), 16, "elu", False)
F_NONE = (64, (96,), 14, "none", False)

# (id, mode, spec0, spec1 or None, rows, expected instantiation, extra).  rows: an int, or "rtK" / "rtK-1" = the first row count
# the query gives K row tiles for / the one below it, "+N" suffix: N rows more.  extra: acts split (pair).
CASES = [
    ("fwd-348-m1", "fwd", A348, None, 1, "lt_mlp_kernel<1,1,1>", None),
    ("fwd-348-rt2", "fwd", A348, None, "rt2", "lt_mlp_kernel<2,1,1>", None),
    ("fwd-348-rt4", "fwd", A348, None, "rt4", "lt_mlp_kernel<4,1,1>", None),
    ("fwd-270-m17", "fwd", A270, None, 17, "lt_mlp_kernel<1,1,3>", None),
    ("fwd-270-rt2-1", "fwd", A270, None, "rt2-1", "lt_mlp_kernel<1,1,3>", None),
    ("fwd-33-rt2", "fwd", F33, None, "rt2", "lt_mlp_kernel<2,1,0>", None),
    ("fwd-relu-m37", "fwd", F45_RELU, None, 37, "lt_mlp_kernel<1,-1,0>", None),
    ("fwd-none-m100", "fwd", F_NONE, None, 100, "lt_mlp_kernel<1,-1,0>", None),
    ("fwd-tanh-rt4", "fwd", F270_TANH, None, "rt4", "lt_mlp_kernel<4,-1,0>", None),
    ("fwd-bf16-rt4", "fwd", A348_BF16, None, "rt4", "lt_mlp_kernel<4,1,2>", None),
    ("fwd-1008-rt4-lds", "fwd", F1008, None, "rt4", "lt_mlp_kernel<2,1,1>", None),
    ("fwd-6layer-m300", "fwd", F6, None, 300, "lt_mlp_kernel<1,1,1>", None),
    ("pair-348-m1-f32", "pair", A348, C348, 1, "lt_mlp_kernel<1,1,1>", False),
    ("pair-348-rt4-split", "pair", A348, C348, "rt4+64", "lt_mlp_kernel<4,1,1>", True),
    ("pair-270-m17-split", "pair", A270, C270, 17, "lt_mlp_kernel<1,1,3>", True),
    ("pair-270-rt2-f32", "pair", A270, C270, "rt2", "lt_mlp_kernel<2,1,3>", False),
    ("pair-270-rt4-split", "pair", A270, C270, "rt4+32", "lt_mlp_kernel<4,1,3>", True),
    ("pair-348x270-m48", "pair", A348, C270, 48, "lt_mlp_kernel<1,1,0>", False),
    ("pair-348x270-rt4-1", "pair", A348, C270, "rt4-1", "lt_mlp_kernel<2,1,0>", True),
    ("pair-elu-tanh-rt2", "pair", A348, C_TANH, "rt2", "lt_mlp_kernel<2,-1,0>", False),
    ("pair-bf16-rt2", "pair", A348_BF16, C348_BF16, "rt2+16", "lt_mlp_kernel<2,1,2>", True),
    ("policy-348-rt2-1", "policy", A348, C348, "rt2-1", "lt_mlp_kernel<1,1,1>", None),
    ("policy-348-rt2", "policy", A348, C348, "rt2", "lt_mlp_kernel<2,1,1>", None),
    ("policy-348-rt4", "policy", A348, C348, "rt4", "lt_mlp_kernel<4,1,1>", None),
    ("policy-348-rt4-b1", "policy", A348, C348, "rt4+16", "lt_mlp_kernel<4,1,1>", None),
    ("policy-bf16-m17", "policy", A348_BF16, None, 17, "lt_mlp_kernel<1,1,2>", None),
    ("policy-bf16-32768", "policy", A348_BF16, C348_BF16, 32768, "lt_mlp_kernel<4,1,2>", None),
    ("policy-270-actor-rt2", "policy", A270, None, "rt2", "lt_mlp_kernel<2,1,3>", None),
    ("policy-45-m1", "policy", A45, C348, 1, "lt_mlp_kernel<1,1,0>", None),
    ("policy-348x270-rt4", "policy", A348, C270, "rt4", "lt_mlp_kernel<4,1,0>", None),
    ("policy-elu-tanh-rt4", "policy", A348, C_TANH, "rt4+48", "lt_mlp_kernel<4,-1,0>", None),
    ("policy-6layer-m33", "policy", A6, C348, 33, "lt_mlp_kernel<1,1,1>", None),
    ("bwd-m37", "bwd", A348, C348, 37, "lt_mlp_kernel<1,100,0>", None),
    ("bwd-rt2", "bwd", A348, C348, "rt2", "lt_mlp_kernel<2,100,0>", None),
    ("bwd-rt4", "bwd", (348, (512, 256, 136), 16, "elu", False), C348, "rt4", "lt_mlp_kernel<4,100,0>", None),
]


def desc_of(spec):
    d_in, hidden, out, act, bf16 = spec
    d = _abi.LtMlpDesc()
    dims = [d_in, *hidden, out]
    d.num_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    d.activation = C[{"elu": "LT_ACT_ELU", "relu": "LT_ACT_RELU", "tanh": "LT_ACT_TANH", "none": "LT_ACT_NONE"}[act]]
    d.input_format = C["LT_ROWS_BF16"] if bf16 else C["LT_ROWS_F32"]
    return d


def kernel_name(mode, spec0, spec1, m):
    lib = _abi.load()
    d0 = desc_of(spec0)
    d1 = desc_of(spec1) if spec1 is not None else None
    got = lib.lt_mlp_kernel_name(ctypes.byref(d0), ctypes.byref(d1) if d1 is not None else None, int(m), MODES[mode])
    return got.decode() if got else None


def row_tiles(mode, spec0, spec1, m) -> int:
    return int(kernel_name(mode, spec0, spec1, m).split("<")[1].split(",")[0])


def resolve_rows(rows, mode, two_nets: bool) -> int:
    """`rtK`: the first row count for which the query gives K row tiles to a launch of this mode and number of networks (bisection on
    the query, with the 348-wide networks: the row tiles depend on the rows alone below the LDS fallback); `rtK-1`: one row fewer;
    `+N`: N rows more."""
    if isinstance(rows, int):
        return rows
    base, _, plus = rows.partition("+")
    k, minus = int(base[2]), base.endswith("-1")
    s0, s1 = A348, (C348 if two_nets else None)
    lo, hi = 1, 1 << 20
    assert row_tiles(mode, s0, s1, hi) == 4
    while lo < hi:
        mid = (lo + hi) // 2
        if row_tiles(mode, s0, s1, mid) >= k:
            hi = mid
        else:
            lo = mid + 1
    return lo - (1 if minus else 0) + (int(plus) if plus else 0)


def case_rows(case) -> int:
    _, mode, s0, s1, rows, _, _ = case
    return resolve_rows(rows, mode, s1 is not None)


def test_cases_cover_every_compiled_instantiation():
    """Host-only: every case runs the instantiation it names, and together the cases cover all the library holds."""
    named = set()
    for case in CASES:
        cid, mode, s0, s1, rows, want, _ = case
        m = case_rows(case)
        got = kernel_name(mode, s0, s1, m)
        assert got == want, (cid, m, got, want)
        named.add(got)
    compiled = R.compiled_instantiations()
    assert len(compiled) == 18, compiled
    assert named == compiled, ("instantiations without a case", sorted(compiled - named))
    # grids split by XCD (two networks of equal rows) whose per-network block count leaves blocks idle: b0 % 4 in {1, 2, 3}
    rem = set()
    for case in CASES:
        cid, mode, s0, s1, rows, want, _ = case
        if s1 is None:
            continue
        m = case_rows(case)
        rt = row_tiles(mode, s0, s1, m)
        rem.add(((m + 15) // 16 + rt - 1) // rt % 4)
    assert {1, 2, 3} <= rem, rem


# ---- helpers on the device ------------------------------------------------------------------------------------------------------------
def _net(spec, seed, head_scale=1.0):
    import torch
    from locotouch_amd.rl.modules import build_mlp

    d_in, hidden, out, act, _ = spec
    torch.manual_seed(seed)
    if act == "none":  # (build_mlp knows the reference's activations only)
        dims, mods = [d_in, *hidden, out], []
        for i in range(len(dims) - 1):
            mods += [torch.nn.Linear(dims[i], dims[i + 1])] + ([torch.nn.Identity()] if i < len(dims) - 2 else [])
        seq = torch.nn.Sequential(*mods).to("cuda:0")
    else:
        seq = build_mlp(d_in, list(hidden), out, act).to("cuda:0")
    with torch.no_grad():
        for p in seq.parameters():
            p.mul_(2.0)  # livelier activations than the default init
        if head_scale != 1.0:  # a policy head with means of several units (the log-prob's rounding grows with |mu| / sigma)
            R.linears(seq)[-1].bias.uniform_(-head_scale, head_scale)
    return seq


def _rows(spec, m, seed):
    import torch

    g = torch.Generator(device="cuda:0").manual_seed(seed)
    x = torch.randn(m, spec[0], device="cuda:0", generator=g) * 1.5
    if spec[4]:
        x = x.to(torch.bfloat16)
    return x


def _packed(seq, spec):
    import torch
    from locotouch_amd.rl.mlp import PackedMLP

    net = PackedMLP(seq)
    if spec[4]:
        net.set_input_format(torch.bfloat16)
    return net


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _stream():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dec_split(t):
    """An activation tensor in the split format (one dword per element: f16 hi | f16 lo << 16) -> f64 values hi + lo / 64."""
    import torch

    h = t.contiguous().view(torch.float16).view(t.shape[0], t.shape[1], 2).double()
    return h[..., 0] + h[..., 1] / 64.0


def _check(cid, name, e_hip, e_f32, extra=""):
    ex = RATIO_EXCEPTIONS.get(cid, {})
    rows = [f"[mlp f64] {cid:24s} {name:24s} {extra}"]
    for k, (eh, top, band) in e_hip.items():
        ef = e_f32[k][0]
        rows.append(f"    {k:14s} hip {eh:10.3e}  f32 {ef:10.3e}  ratio {eh / ef if ef > 0 else float('nan'):7.2f}  |ref| {top:9.3e}  band {band:6.3f}")
    print("\n".join(rows))
    bad = f64_ratio_failures(e_hip, e_f32, exceptions=ex)
    assert not bad, f"{cid} ({name}): further from f64 than {F64_RATIO} x torch fp32: " + "; ".join(
        f"{nm} e_hip={ec:.3e} e_f32={eo:.3e} (allowed ratio {r})" for nm, ec, eo, r in bad)


def _run_forward(cid, spec0, m):
    import torch

    seq = _net(spec0, 11)
    x = _rows(spec0, m, 7)
    net = _packed(seq, spec0)
    y = net(x)
    torch.cuda.synchronize()
    xr = x.float()
    y64, _ = R.forward64(seq, xr)
    y32, _ = R.forward32(seq, xr)
    return {"y": R.err(y, y64)}, {"y": R.err(y32, y64)}


def _run_pair(cid, spec0, spec1, m, split):
    import torch

    lib = _abi.load()
    seqs = (_net(spec0, 11), _net(spec1, 12))
    xs = (_rows(spec0, m, 7), _rows(spec1, m, 8))
    nets = [_packed(s, sp) for s, sp in zip(seqs, (spec0, spec1))]
    ys = [torch.empty(m, sp[2], device="cuda:0") for sp in (spec0, spec1)]
    acts = [[torch.empty(m, h, device="cuda:0") for h in sp[1]] for sp in (spec0, spec1)]
    arr = [(ctypes.c_void_p * max(1, len(a)))(*[t.data_ptr() for t in a]) for a in acts]
    _abi.check(lib.lt_mlp_forward_pair(ctypes.byref(nets[0].desc), _vp(nets[0].packed), _vp(xs[0]), ctypes.byref(nets[1].desc),
                                       _vp(nets[1].packed), _vp(xs[1]), m, _vp(ys[0]), _vp(ys[1]), arr[0], arr[1], int(split), _stream()),
               "lt_mlp_forward_pair")
    torch.cuda.synchronize()
    e_hip, e_f32 = {}, {}
    for k in range(2):
        xr = xs[k].float()
        y64, a64 = R.forward64(seqs[k], xr)
        y32, a32 = R.forward32(seqs[k], xr)
        e_hip[f"y{k}"], e_f32[f"y{k}"] = R.err(ys[k], y64), R.err(y32, y64)
        for l, (got, r64, r32) in enumerate(zip(acts[k], a64, a32)):
            got = _dec_split(got) if split else got
            e_hip[f"act{k}.{l}"], e_f32[f"act{k}.{l}"] = R.err(got, r64), R.err(r32, r64)
    return e_hip, e_f32


def _run_policy(cid, spec0, spec1, m):
    import torch

    from tests import oracle_lib

    lib = _abi.load()
    actor = _net(spec0, 11, head_scale=6.0)
    obs = _rows(spec0, m, 7)
    a_net = _packed(actor, spec0)
    std = torch.tensor(STD12, device="cuda:0")
    counter = torch.tensor([5], dtype=torch.int64, device="cuda:0")  # caller-owned: the Philox step is *counter + offset = 7
    offset, step = 2, 7
    st = {k: torch.full((m, 12), float("nan"), device="cuda:0") for k in ("actions", "mu", "sigma", "out")}
    logp = torch.full((m, 1), float("nan"), device="cuda:0")
    tail = [_vp(std), _vp(st["actions"]), _vp(st["mu"]), _vp(st["sigma"]), _vp(logp), _vp(st["out"]), _stream()]
    if spec1 is None:
        _abi.check(lib.lt_rollout_policy(ctypes.byref(a_net.desc), _vp(a_net.packed), _vp(obs), m, SEED, _vp(counter), offset, *tail),
                   "lt_rollout_policy")
    else:
        critic = _net(spec1, 12)
        cobs = _rows(spec1, m, 8)
        c_net = _packed(critic, spec1)
        values = torch.full((m, 1), float("nan"), device="cuda:0")
        _abi.check(lib.lt_rollout_policy_value(ctypes.byref(a_net.desc), _vp(a_net.packed), _vp(obs), ctypes.byref(c_net.desc),
                                               _vp(c_net.packed), _vp(cobs), _vp(values), m, SEED, _vp(counter), offset, *tail),
                   "lt_rollout_policy_value")
    torch.cuda.synchronize()
    mu64, _ = R.forward64(actor, obs.float())
    mu32, _ = R.forward32(actor, obs.float())
    z64 = torch.from_numpy(oracle_lib.policy_normals(SEED, m, step)).cuda()
    z32 = R.policy_normals32(SEED, m, step).cuda()
    s64 = std.double()
    a_ref = mu64 + s64 * z64
    a32 = mu32 + std * z32
    lp32 = torch.distributions.Normal(mu32, std.expand(m, 12)).log_prob(a32).sum(-1)
    # logp: against the exact mean, where the f32 error of mu (divided by sigma) dominates both sides; logp_own: against log N of the
    # stored action around the stored mean - the log-prob formula alone, which must be that of the stored action (ppo.py:135)
    e_hip = {"mu": R.err(st["mu"], mu64), "action": R.err(st["actions"], a_ref),
             "logp": R.err(logp[:, 0], R.log_normal64(st["actions"], mu64, s64.expand(m, 12))),
             "logp_own": R.err(logp[:, 0], R.log_normal64(st["actions"], st["mu"], s64.expand(m, 12)))}
    e_f32 = {"mu": R.err(mu32, mu64), "action": R.err(a32, a_ref), "logp": R.err(lp32, R.log_normal64(a32, mu64, s64.expand(m, 12))),
             "logp_own": R.err(lp32, R.log_normal64(a32, mu32, s64.expand(m, 12)))}
    assert torch.equal(st["sigma"], std.expand(m, 12)), "sigma must be std, bit for bit"
    assert torch.equal(st["out"], st["actions"]), "actions_out must equal the stored actions"
    z_hip = (st["actions"].double() - st["mu"].double()) / s64
    dz = ((z_hip - z64).abs() / (1.0 + z64.abs()))
    zmax = float(dz.max())
    worst = divmod(int(dz.argmax()), 12)
    assert zmax <= Z_TOL, f"{cid}: draws differ from the oracle twin by {zmax:.3e} (1 + |z|) at env {worst[0]}, action {worst[1]}"
    extra = f"z vs oracle twin: max {zmax:.2e} (1 + |z|)"
    if spec1 is not None:
        v64, _ = R.forward64(critic, cobs.float())
        v32, _ = R.forward32(critic, cobs.float())
        e_hip["value"], e_f32["value"] = R.err(values, v64), R.err(v32, v64)
    assert int(counter) == 5  # the kernel reads the counter, it does not advance it
    return e_hip, e_f32, extra


def _chain32(seq, x, dy, acts32):
    """torch fp32 backward chain on the same gated activations: dz per hidden layer."""
    lin = R.linears(seq)
    g, dz = dy.float(), {}
    for l in range(len(lin) - 1, 0, -1):
        g = g @ lin[l].weight.float()
        a = acts32[l - 1]
        g = g * (a > 0).float() + g * (a + 1.0) * (a <= 0).float()
        dz[l - 1] = g
    return dz


def _run_backward(cid, spec0, spec1, m):
    import torch

    lib = _abi.load()
    seqs = (_net(spec0, 11), _net(spec1, 12))
    xs = (_rows(spec0, m, 7).float(), _rows(spec1, m, 8).float())
    g = torch.Generator(device="cuda:0").manual_seed(m)
    dys = [torch.randn(m, sp[2], device="cuda:0", generator=g) * 1e-3 for sp in (spec0, spec1)]
    dys[0][::53] *= 200.0  # heavy-tailed rows, as PPO's are
    nets = [_packed(s, sp) for s, sp in zip(seqs, (spec0, spec1))]
    for n in nets:
        n.pack_backward()
    nblk = int(lib.lt_mlp_backward_blocks(ctypes.byref(nets[0].desc), ctypes.byref(nets[1].desc), m))
    assert nblk > 0
    acts32, dzs, amax, e_hip, e_f32 = [], [], [], {}, {}
    for k in range(2):
        _, a64 = R.forward64(seqs[k], xs[k])
        acts32.append([a.float().contiguous() for a in a64])  # both candidates gate with the same f32 activations
        dzs.append([torch.full_like(a, float("nan")) for a in acts32[k]])
        amax.append([torch.zeros(nblk, device="cuda:0") for _ in acts32[k]])
    arrs = [[(ctypes.c_void_p * len(acts32[k]))(*[t.data_ptr() for t in lst]) for lst in (acts32[k], dzs[k], amax[k])] for k in range(2)]
    sat = torch.zeros(1, device="cuda:0")
    _abi.check(lib.lt_mlp_backward_pair(ctypes.byref(nets[0].desc), _vp(nets[0].bpacked), _vp(dys[0]), *arrs[0],
                                        ctypes.byref(nets[1].desc), _vp(nets[1].bpacked), _vp(dys[1]), *arrs[1],
                                        m, 0, None, None, 0, None, _vp(sat), _stream()), "lt_mlp_backward_pair")
    torch.cuda.synchronize()
    assert float(sat) == 0.0
    for k in range(2):
        rdz, _, _ = R.ref_chain(seqs[k], xs[k], dys[k])
        dz32 = _chain32(seqs[k], xs[k], dys[k], acts32[k])
        for l, ref in rdz.items():
            e_hip[f"dz{k}.{l}"], e_f32[f"dz{k}.{l}"] = R.err(dzs[k][l], ref), R.err(dz32[l], ref)
    return e_hip, e_f32


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mlp_kernel_matches_float64(case):
    cid, mode, s0, s1, rows, want, extra = case
    m = case_rows(case)
    name = kernel_name(mode, s0, s1, m)
    assert name == want, (cid, m, name)
    note = f"m={m}"
    if mode == "fwd":
        e_hip, e_f32 = _run_forward(cid, s0, m)
    elif mode == "pair":
        e_hip, e_f32 = _run_pair(cid, s0, s1, m, extra)
        note += " split" if extra else " f32"
    elif mode == "policy":
        e_hip, e_f32, z = _run_policy(cid, s0, s1, m)
        note += " " + z
    else:
        e_hip, e_f32 = _run_backward(cid, s0, s1, m)
    _check(cid, name, e_hip, e_f32, note)


# ---- magnitude sweep --------------------------------------------------------------------------------------------------------------------
# The weights enter the kernel split as hi + lo / 64 in f16 (lt_mlp_pack): the low part resolves an ABSOLUTE 2^-31 per weight (its f16
# subnormal step 2^-24, over 64, halved), include/lt_env.h DOMAIN.  The sweep scales the head's weights and bias (so that the outputs
# scale with them and no bias hides the products) by 2^-3 .. 2^-12.  Down to 2^SWEEP_F32_DOWN_TO the kernel is held to the ratio rule
# against the exact weights; below it, to the ratio rule against the weights as they are split (mlp_ref.split_weights64) - the
# documented floor - and to the exact answer within that floor plus the rule.
SWEEP_F32_DOWN_TO = -10  # measured (348-512-256-128 stack, 128-input head): ratio 4.5 at 2^-10 (rms |w| 1e-4), 8.0 at 2^-11, 19 at 2^-12


@pytest.mark.gpu
@pytest.mark.parametrize("wexp", list(range(-3, -13, -1)))
def test_weight_magnitude_sweep(wexp):
    import torch

    spec = A348
    seq = _net(spec, 21)
    head = R.linears(seq)[-1]
    with torch.no_grad():
        head.weight.mul_(2.0 ** wexp)
        head.bias.mul_(2.0 ** wexp)
    x = _rows(spec, 1024, 9)
    y = _packed(seq, spec)(x)
    torch.cuda.synchronize()
    y64, _ = R.forward64(seq, x)
    y32, _ = R.forward32(seq, x)
    ys64, _ = R.forward64(seq, x, weights=R.split_weights64(seq))
    e_hip, e_f32 = {"y": R.err(y, y64)}, {"y": R.err(y32, y64)}
    floor = R.err(ys64, y64)[0]
    rms = float(head.weight.detach().pow(2).mean().sqrt())
    note = f"head weights x 2^{wexp}, rms |w| {rms:.2e}; split-weight error {floor:.3e}, ratio to f32 {floor / e_f32['y'][0]:.2f}"
    if wexp >= SWEEP_F32_DOWN_TO:
        _check(f"sweep-w{wexp}", "lt_mlp_kernel<1,1,1>", e_hip, e_f32, note)
    else:
        _check(f"sweep-w{wexp}", "lt_mlp_kernel<1,1,1>", {"y_vs_split": R.err(y, ys64)}, {"y_vs_split": e_f32["y"]}, note)
        assert e_hip["y"][0] <= floor + F64_RATIO * e_f32["y"][0] + 16 * 2.0 ** -24 * e_hip["y"][1], (note, e_hip["y"])


@pytest.mark.gpu
@pytest.mark.parametrize("xexp", list(range(-8, 9, 2)))
def test_input_magnitude_sweep(xexp):
    import torch

    spec = A348
    seq = _net(spec, 22)
    x = _rows(spec, 1024, 10).clamp(-3.0, 3.0) * 2.0 ** xexp  # (|x| <= 768 < LT_MLP_INPUT_CLAMP at 2^8)
    y = _packed(seq, spec)(x)
    torch.cuda.synchronize()
    y64, _ = R.forward64(seq, x)
    y32, _ = R.forward32(seq, x)
    _check(f"sweep-x{xexp}", "lt_mlp_kernel<1,1,1>", {"y": R.err(y, y64)}, {"y": R.err(y32, y64)}, f"inputs x 2^{xexp}")
