"""A plain-torch restatement of the PPO-update entry points of csrc/lt_ppo.hip (`lt_ppo_loss`, `lt_ppo_lr_rule`, `lt_gae`,
`lt_adam_clip_step(_dev)`, `lt_elu_backward_bias(2)`, `lt_head_wgrad`, `lt_partial_sums`; include/lt_env.h), seeded case generators and
the comparator that tests/test_hip_ppo_f64.py holds the kernels to.  Nothing here needs a GPU; tests/test_ppo_ref.py pins it.

Every oracle function is ONE text for every role (`dtype`, `device`): float64 on the CPU is the oracle, float32 on the CPU and float32
on the GPU are baselines.  Inputs are the float32 values that cross the C ABI, hyper-parameters included (`f32` below): the oracle
converts those values to float64 exactly and computes from there.  Gradients of the loss are autograd's, never hand-written formulas.

A result is a dict of named arrays; the key "_terms" holds, for every REDUCED output X, a tensor T with X = T.sum(0): the comparator
scales X's error by sum |T| (what any order of summation errs in proportion to; |X| itself is near zero wherever the summands cancel,
as the surrogate's do), and `sequential` adds T in float32 in row order as a third baseline.

`mutate` exists for tests/test_ppo_ref.py alone: it turns the float32 form into a stand-in for a kernel with one plausible slip, so
that the comparator, the exact checks and the generated inputs are shown to tell the two apart."""
import math

import numpy as np
import torch

from tests.seq_ref import EPS, FACTOR

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
MARGIN = 1.0e-3  # `make_loss_case`: no row closer than this to a branch boundary (in float64)
EXACT_ONLY = ("amax_mu", "amax_v", "amax_blocks")  # held by `exact_problems` to the kernel's own arrays, not by the comparator

# mutation -> (entry point, an array that must reject it)
MUTATIONS = {
    "kl_without_1e-5": ("ppo_loss", "kl"),
    "clipped_branch_gradient_not_zeroed": ("ppo_loss", "dmu"),
    "value_gradient_decided_by_in_v_alone": ("ppo_loss", "dvalue"),
    "dstd_without_minus_inv_sigma": ("ppo_loss", "dstd"),
    "entropy_gradient_dropped": ("ppo_loss", "dstd"),
    "inv_m_of_m_rounded_up_to_256": ("ppo_loss", "dvalue"),
    "old_sigma_read_at_row": ("ppo_loss", "kl"),
    "amax_mu_before_inv_sigma": ("ppo_loss", "amax_mu"),
    "gae_dones_of_next_step": ("gae", "returns"),
    "gae_lambda_term_without_done_mask": ("gae", "returns"),
    "adam_eps_inside_sqrt": ("adam_clip_step", "p"),
    "adam_bias_correction_with_step_minus_1": ("adam_clip_step", "p"),
    "clip_coefficient_without_1e-6": ("adam_clip_step", "g"),
    "weight_decay_before_clip": ("adam_clip_step", "m"),
    "elu_derivative_with_a_ge_0": ("elu_backward_bias", "dz"),
    "amax_skips_last_partial_block": ("elu_backward_bias", "amax_blocks"),
    "mantissa10": ("ppo_loss", "gae", "adam_clip_step", "elu_backward_bias", "head_wgrad", "partial_sums"),
}


def f32(x):
    """the value a float argument has once it has crossed the C ABI, as a Python float (exact)"""
    return float(np.float32(x))


KL_EPS = f32(1.0e-5)    # the kernel's 1.0e-5f; the reference's Python 1e-5 meets float32 tensors and is rounded the same way
CLIP_EPS = f32(1.0e-6)  # ... and clip_grad_norm_'s 1e-6


def _to(case, dtype, device):
    return {k: (v.to(device=device, dtype=dtype if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v) for k, v in case.items()}


def _round_mantissa10(x):
    return ((x.view(torch.int32) + 0x1000) & ~0x1FFF).view(torch.float32)


def _finish(res, terms, mutate):
    res = {k: v.detach() for k, v in res.items()}
    if mutate == "mantissa10":
        res = {k: _round_mantissa10(v.contiguous()) for k, v in res.items()}
    res["_terms"] = {k: v.detach() for k, v in terms.items()}
    return res


# ---- lt_ppo_loss -----------------------------------------------------------------------------------------------------------------------
def _gathered(c):
    """the batch tensors of a loss case at the minibatch's rows (the index form: rows idx of a larger storage)"""
    idx = c["idx"]
    return {k: (c[k] if idx is None else c[k][idx]) for k in ("actions", "old_logp", "adv", "returns", "old_values", "old_mu", "old_sigma")}


def _log_prob(actions, mu, sig):
    z = (actions - mu) / sig
    return -0.5 * z * z - torch.log(sig) - HALF_LOG_2PI


def loss_branches(case, dtype=torch.float64):
    """Which branch every row takes, as bool tensors [M]: inside / above / below for the probability ratio against 1 +- clip, and for
    the value clip v_inside / v_outside_l1 (unclipped loss larger: the gradient flows) / v_outside_l2 (clipped loss larger: it does not)."""
    c = _to(case, dtype, "cpu")
    b = _gathered(c)
    clip = c["clip"]
    ratio = torch.exp(_log_prob(b["actions"], c["mu"], c["std"].expand_as(c["mu"])).sum(-1) - b["old_logp"])
    d = c["value"] - b["old_values"]
    l1, l2 = (c["value"] - b["returns"]) ** 2, (b["old_values"] + d.clamp(-clip, clip) - b["returns"]) ** 2
    v_in = (d >= -clip) & (d <= clip)
    return dict(inside=(ratio >= 1 - clip) & (ratio <= 1 + clip), above=ratio > 1 + clip, below=ratio < 1 - clip, v_inside=v_in,
                v_outside_l1=~v_in & (l1 > l2), v_outside_l2=~v_in & (l1 < l2))


def ppo_loss(case, dtype=torch.float64, device="cpu", mutate=None):
    """The minibatch loss of loco_rl/algorithms/ppo.py:251-311 with its gradients: Normal log-prob of the stored actions, the KL to the
    behaviour policy (`+ 1e-5` inside the log, not differentiated), the clipped surrogate (`torch.max`), the clipped or plain value loss,
    the entropy of the state-independent std.  loss = mean surrogate + vcoef * mean value loss - ecoef * entropy.

    Arrays: dmu [M][A], dvalue [M], dstd [A] (incl. the entropy term: the kernel's out[8 + a]), loss, surrogate, value_loss, entropy, kl
    (out[0 .. 4]); acc_surrogate, acc_value_loss, acc_kl (the row SUMS, acc[0 .. 2]), acc_dstd [A] (acc[4 + a]: the surrogate's share of
    dstd); amax_mu, amax_v = max |dmu|, max |dvalue| of THESE arrays (acc[20], acc[21])."""
    c = _to(case, dtype, device)
    M, A = c["mu"].shape
    b = _gathered(c)
    if mutate == "old_sigma_read_at_row":
        b["old_sigma"] = c["old_sigma"][:M]
    clip, vcoef, ecoef = c["clip"], c["vcoef"], c["ecoef"]
    mu, value, std = (c[k].clone().requires_grad_(True) for k in ("mu", "value", "std"))
    # the std as a leaf PER ROW on the log-prob's side: its gradient is the per-row summands of the surrogate's d / d sigma
    sig = c["std"].expand(M, A).clone().requires_grad_(True)
    if mutate == "dstd_without_minus_inv_sigma":
        z = (b["actions"] - mu) / sig
        logp = (-0.5 * z * z - torch.log(sig.detach()) - HALF_LOG_2PI).sum(-1)
    else:
        logp = _log_prob(b["actions"], mu, sig).sum(-1)
    with torch.no_grad():
        kl_rows = (torch.log(sig / b["old_sigma"] + (0.0 if mutate == "kl_without_1e-5" else KL_EPS))
                   + (b["old_sigma"] ** 2 + (b["old_mu"] - mu) ** 2) / (2.0 * sig ** 2) - 0.5).sum(-1)
    ratio = torch.exp(logp - b["old_logp"])
    s1 = -b["adv"] * ratio
    surr_rows = torch.max(s1, -b["adv"] * torch.clamp(ratio, 1.0 - clip, 1.0 + clip))
    if mutate == "clipped_branch_gradient_not_zeroed":
        surr_rows = s1 + (surr_rows - s1).detach()
    if c["clipped"]:
        d = value - b["old_values"]
        l1, l2 = (value - b["returns"]) ** 2, (b["old_values"] + d.clamp(-clip, clip) - b["returns"]) ** 2
        vl_rows = torch.max(l1, l2)
        if mutate == "value_gradient_decided_by_in_v_alone":
            vl_rows = torch.where(((d >= -clip) & (d <= clip)).detach(), l1, vl_rows.detach())
    else:
        vl_rows = (b["returns"] - value) ** 2
    ent_terms = 0.5 + HALF_LOG_2PI + torch.log(std.detach() if mutate == "entropy_gradient_dropped" else std)
    rows = ((M + 255) // 256) * 256 if mutate == "inv_m_of_m_rounded_up_to_256" else M
    mean = (lambda r: r.sum() / rows) if rows != M else (lambda r: r.mean())
    surrogate, value_loss, kl, entropy = mean(surr_rows), mean(vl_rows), mean(kl_rows), ent_terms.sum()
    loss = surrogate + vcoef * value_loss - ecoef * entropy
    loss.backward()
    dstd_entropy = std.grad if std.grad is not None else torch.zeros_like(std)
    dmu, dvalue, dstd_rows = mu.grad, value.grad, sig.grad
    res = dict(dmu=dmu, dvalue=dvalue, dstd=dstd_rows.sum(0) + dstd_entropy, loss=loss, surrogate=surrogate, value_loss=value_loss,
               entropy=entropy, kl=kl, acc_surrogate=surr_rows.sum(), acc_value_loss=vl_rows.sum(), acc_kl=kl_rows.sum(),
               acc_dstd=dstd_rows.sum(0), amax_v=dvalue.abs().max(),
               amax_mu=(dmu * sig).abs().max() if mutate == "amax_mu_before_inv_sigma" else dmu.abs().max())
    ent = ent_terms.detach()
    terms = dict(surrogate=surr_rows / M, value_loss=vl_rows / M, kl=kl_rows / M, entropy=ent, acc_surrogate=surr_rows, acc_value_loss=vl_rows,
                 acc_kl=kl_rows, acc_dstd=dstd_rows, dstd=torch.cat([dstd_rows, dstd_entropy[None]]),
                 loss=torch.cat([surr_rows / M, vcoef * vl_rows / M, -ecoef * ent]))
    return _finish(res, terms, mutate)


def make_loss_case(M, A, seed, clipped, rows=None, boundary=False, vcoef=1.0, ecoef=0.01):
    """CPU float32 inputs of one lt_ppo_loss call, hyper-parameters as the float32 values the call passes.  The std and a
    state-independent old sigma near it (ratio within +-10 %), mu = old_mu + c * old_sigma * randn (c = 0.05, grown by (12 / A)^0.8
    below 12 actions: the log-ratio is a sum over the actions, and a single action's needs that much for the ratio to leave the clip range
    on a tenth of the rows either side), actions drawn from the
    behaviour policy and old_logp their float64 log-prob under it, advantages of both signs, old_values = value + 0.3 randn around
    clip = 0.2.  Every 64th row is FAR (|z| from 4 to 8 in the action whose two sigmas are closest) and every 32nd has adv == 0.

    Margin: PPO's loss is discontinuous in its inputs - a row whose ratio lies within float32 rounding of 1 +- clip, or whose value
    difference lies within rounding of +- clip, can take the other branch in float32 and be right.  Every row that in float64 is closer
    than MARGIN to a boundary (|ratio - (1 +- clip)|; ||v - ov| - clip|; outside the value clip |l1 - l2| relative to their max) is
    drawn again; case["redrawn"] counts them.  No row is left out of any comparison.

    `rows` = R > M: the index form - the batch tensors have R rows, idx is a random injection [M] -> [R], every unreferenced row is NaN.
    `boundary`: clip = 0.25 and value, old_values multiples of 1 / 8, so that a share of the rows has value - old_value == +- clip
    EXACTLY (those are kept: there the two value losses are equal with equal derivatives, and autograd agrees with `>=` / `<=`)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    clip = f32(0.25 if boundary else 0.2)
    std = 0.4 + 0.4 * ru(A)
    delta = 0.2 * ru(A) - 0.1
    sigma_row = std / (1.0 + delta)
    far_dim = int(delta.abs().argmin())
    c_mu = 0.05 * max(1.0, (12.0 / A) ** 0.8)

    def draw(k, plant=False):
        old_mu, old_sigma, z_old = rn(k, A), sigma_row.expand(k, A).clone(), rn(k, A)
        far = (torch.arange(k) % 64 == 3) & plant
        z_old[far, far_dim] = (torch.where(ru(k) < 0.5, -1.0, 1.0) * (4.0 + 4.0 * ru(k)))[far]
        actions = old_mu + old_sigma * z_old
        mu = old_mu + c_mu * old_sigma * rn(k, A)
        old_logp = _log_prob(actions.double(), old_mu.double(), old_sigma.double()).sum(-1).float()
        adv = torch.where((torch.arange(k) % 32 == 5) & plant, torch.zeros(k), rn(k))
        value, returns = rn(k), rn(k)
        if boundary:
            value = torch.round(value * 8.0) / 8.0
            old_values = value + torch.randint(-4, 5, (k,), generator=gen).float() / 8.0
        else:
            old_values = value + 0.3 * rn(k)
        return dict(mu=mu, value=value, actions=actions, old_logp=old_logp, adv=adv, returns=returns, old_values=old_values, old_mu=old_mu,
                    old_sigma=old_sigma)

    def near(r):
        c = {k: v.double() for k, v in r.items()}
        ratio = torch.exp(_log_prob(c["actions"], c["mu"], std.double().expand_as(c["mu"])).sum(-1) - c["old_logp"])
        bad = ((ratio - (1.0 - clip)).abs() < MARGIN) | ((ratio - (1.0 + clip)).abs() < MARGIN)
        if clipped:
            d = c["value"] - c["old_values"]
            dist = (d.abs() - clip).abs()
            l1, l2 = (c["value"] - c["returns"]) ** 2, (c["old_values"] + d.clamp(-clip, clip) - c["returns"]) ** 2
            bad |= (dist < MARGIN) & ~((dist == 0.0) & bool(boundary))
            bad |= (d.abs() > clip) & ((l1 - l2).abs() < MARGIN * torch.maximum(l1, l2))
        return bad

    r = draw(M, plant=True)
    redrawn = 0
    while True:
        bad = near(r)
        k = int(bad.sum())
        if k == 0:
            break
        redrawn += k
        new = draw(k)
        for name in r:
            r[name][bad] = new[name]
    case = dict(r, std=std, idx=None, clip=clip, vcoef=f32(vcoef), ecoef=f32(ecoef), clipped=int(clipped), redrawn=redrawn,
                far=int((((r["actions"] - r["old_mu"]) / r["old_sigma"]).abs().amax(-1) > 3.9).sum()))
    if rows is not None:
        assert rows > M
        idx = torch.randperm(rows, generator=gen)[:M]
        for name in ("actions", "old_logp", "adv", "returns", "old_values", "old_mu", "old_sigma"):
            big = torch.full((rows, *r[name].shape[1:]), float("nan"))
            big[idx] = r[name]
            case[name] = big
        case["idx"] = idx
    return case


# ---- lt_gae ----------------------------------------------------------------------------------------------------------------------------
def gae(case, dtype=torch.float64, device="cpu", mutate=None):
    """RolloutStorage.compute_returns' recursion (rollout_storage.py:170-186) as a Python time loop, before any normalisation:
    delta = r + (1 - done) gamma V' - V;  A = delta + (1 - done) gamma lambda A';  returns = A + V;  advantages = returns - V."""
    c = _to(case, dtype, device)
    gamma, lam, T = c["gamma"], c["lam"], c["rewards"].shape[0]
    alive_all = 1.0 - c["dones"].to(dtype)
    returns = torch.empty_like(c["rewards"])
    next_v, adv = c["last_values"], torch.zeros_like(c["last_values"])
    for t in range(T - 1, -1, -1):
        alive = alive_all[t]
        if mutate == "gae_dones_of_next_step":
            alive = alive_all[t + 1] if t + 1 < T else torch.ones_like(alive)
        delta = c["rewards"][t] + alive * gamma * next_v - c["values"][t]
        adv = delta + (1.0 if mutate == "gae_lambda_term_without_done_mask" else alive) * gamma * lam * adv
        returns[t] = adv + c["values"][t]
        next_v = c["values"][t]
    return _finish(dict(returns=returns, advantages=returns - c["values"]), {}, mutate)


def make_gae_case(T, N, seed, small_rewards=False):
    """dones at 10 %; with N >= 2 column 0 is done at every step and column N - 1 never.  `small_rewards`: rewards of order 0.01 against
    values of order 10 (the advantages are then small differences of large returns and values)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    dones = (torch.rand(T, N, generator=gen) < 0.1).to(torch.uint8)
    if N >= 2:
        dones[:, 0], dones[:, N - 1] = 1, 0
    if small_rewards:
        rewards, values, last_values = 0.01 * rn(T, N), 10.0 + rn(T, N), 10.0 + rn(N)
    else:
        rewards, values, last_values = rn(T, N), rn(T, N), rn(N)
    return dict(rewards=rewards, dones=dones, values=values, last_values=last_values, gamma=f32(0.99), lam=f32(0.95))


# ---- lt_adam_clip_step -----------------------------------------------------------------------------------------------------------------
def adam_clip_step(case, dtype=torch.float64, device="cpu", mutate=None):
    """clip_grad_norm_ (coefficient min(1, max_norm / (norm + 1e-6)); no clip when max_norm <= 0) followed by Adam with coupled weight
    decay, in torch's order: g += wd p; m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g g; denom = sqrt(v) / sqrt(1 - b2^t) + eps;
    p -= lr / (1 - b1^t) * (m / denom).  b1, b2, eps, lr, wd, max_norm are the float32 values of the call, taken exactly: 1 - b2 is then
    the same number in the moment update and in the bias correction.  Arrays: p, g (the scaled gradients left behind), m, v, grad_norm_sq."""
    c = _to(case, dtype, device)
    p, g, m, v = c["p"], c["g"], c["m"], c["v"]
    b1, b2, eps, wd, lr, step, max_norm = c["b1"], c["b2"], c["eps"], c["wd"], c["lr"], c["step"], c["max_norm"]
    sq = g * g
    norm_sq = sq.sum()
    coef = 1.0
    if max_norm > 0.0:
        coef = torch.clamp(max_norm / (norm_sq.sqrt() + (0.0 if mutate == "clip_coefficient_without_1e-6" else CLIP_EPS)), max=1.0)
    if mutate == "weight_decay_before_clip":
        g = (g + wd * p) * coef
        gi = g
    else:
        g = g * coef
        gi = g + wd * p if wd != 0.0 else g
    m = m + (1.0 - b1) * (gi - m)
    v = b2 * v + (1.0 - b2) * gi * gi
    t = step - 1 if mutate == "adam_bias_correction_with_step_minus_1" else step
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if mutate == "adam_eps_inside_sqrt":
        denom = torch.sqrt(v + eps) / math.sqrt(bc2) if bc2 > 0.0 else torch.sqrt(v + eps) / 0.0
    else:
        denom = (v.sqrt() / math.sqrt(bc2) if bc2 > 0.0 else v.sqrt() / 0.0) + eps
    p = p - (lr / bc1 if bc1 > 0.0 else float("inf")) * (m / denom)
    return _finish(dict(p=p, g=g, m=m, v=v, grad_norm_sq=norm_sq), dict(grad_norm_sq=sq), mutate)


ADAM_REGIMES = {  # regime -> (gradient norm, max_norm, weight decay, step, learning rate)
    "above": (4.37, 1.0, 0.0, 1, 1e-3),        # norm above max_norm: the gradients are scaled
    "below": (0.31, 1.0, 0.0, 1000, 1e-2),     # below: coefficient 1
    "no_clip": (4.37, 0.0, 0.0, 1000, 1e-2),   # max_norm = 0 disables the clip
    "decay": (4.37, 1.0, 0.01, 1, 1e-2),       # coupled weight decay, added AFTER the clip
    "tiny": (3.0e-4, 1.0e-4, 0.0, 1, 1e-3),   # a norm at which the 1e-6 of the coefficient is a visible fraction
}


def make_adam_case(n, seed, regime):
    """Parameters ~ 0.1 N(0, 1) (so that one step of 1e-3 .. 1e-2 is a visible fraction of them), gradients scaled to the regime's norm,
    m and v non-zero.  From n >= 64: a stretch of exactly-zero gradients, and a stretch of 1e-30 ones (g * g underflows in float32) whose
    v is zero and whose m is ~1e-10, so that those parameters move by m / eps."""
    norm, max_norm, wd, step, lr = ADAM_REGIMES[regime]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    g = rn(n)
    zero, tiny = slice(n // 4, n // 4 + n // 8), slice(n // 2, n // 2 + n // 8)
    if n >= 64:
        g[zero], g[tiny] = 0.0, 0.0
    scale = norm / float(g.double().norm()) if float(g.abs().max()) > 0.0 else norm
    g = g * scale
    m, v = 0.5 * scale * rn(n), scale * scale * (0.5 + torch.rand(n, generator=gen))
    if n >= 64:
        g[tiny], v[tiny], m[tiny] = 1.0e-30, 0.0, 1.0e-10 * rn(n // 8)
    return dict(p=0.1 * rn(n), g=g, m=m, v=v, max_norm=f32(max_norm), lr=f32(lr), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8), wd=f32(wd), step=step)


# ---- lt_elu_backward_bias(2) -----------------------------------------------------------------------------------------------------------
def elu_block_rows():
    """rows per block of lt_elu_backward_bias, asked of the library (`lt_elu_backward_bias_nblk` is a host function)"""
    from locotouch_amd import _abi

    lib = _abi.load()
    rows = 1
    while lib.lt_elu_backward_bias_nblk(rows + 1) == 1:
        rows += 1
    return rows


def block_amax(dz, block_rows, skip_last_partial=False):
    """max |dz| over rows [block_rows b, block_rows b + block_rows) for every block, the partial last one included"""
    M = dz.shape[0]
    out = [dz[r:r + block_rows].abs().max() for r in range(0, M, block_rows)]
    if skip_last_partial and M % block_rows:
        out[-1] = torch.zeros_like(out[-1])
    return torch.stack(out)


def elu_backward_bias(case, dtype=torch.float64, device="cpu", mutate=None):
    """dz = da * elu'(z) recovered from the OUTPUT a = elu(z): 1 where a > 0, a + alpha elsewhere; db = dz.sum(0); amax_blocks."""
    c = _to(case, dtype, device)
    a, alpha = c["a"], c["alpha"]
    positive = a >= 0 if mutate == "elu_derivative_with_a_ge_0" else a > 0
    dz = c["da"] * torch.where(positive, torch.ones_like(a), a + alpha)
    amax = block_amax(dz, c["block_rows"], skip_last_partial=mutate == "amax_skips_last_partial_block")
    return _finish(dict(dz=dz, db=dz.sum(0), amax_blocks=amax), dict(db=dz), mutate)


PLANTED_NEAR_ZERO = (0.0, -0.0, 1.0e-45, -1.0e-45, 1.1754944e-38, -1.1754944e-38, 2.0 ** -149 * 3, -1.0e-30)


def make_elu_case(M, N, seed, alpha, block_rows):
    """a = elu(randn) in float32, with exact 0.0, -0.0 and values a few ulps from zero (both signs, subnormal and smallest normal)
    planted at every seventh element; da ~ N(0, 1)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.nn.functional.elu(torch.randn(M, N, generator=gen), alpha=alpha)
    flat = a.view(-1)
    planted = torch.tensor(PLANTED_NEAR_ZERO, dtype=torch.float32)
    spots = torch.arange(0, flat.numel(), 7)
    flat[spots] = planted[torch.arange(spots.numel()) % planted.numel()]
    return dict(da=torch.randn(M, N, generator=gen), a=a, alpha=f32(alpha), block_rows=block_rows)


# ---- lt_head_wgrad ---------------------------------------------------------------------------------------------------------------------
def decode_split(words, dtype=torch.float64):
    """the split format's dwords (int32) as numbers: f16(low 16 bits) + f16(high 16 bits) / 64 - exact in float64"""
    halves = words.contiguous().view(torch.float16).view(*words.shape, 2).to(dtype)  # little endian: [..., 0] is the low half
    return halves[..., 0] + halves[..., 1] / 64.0


def encode_split(x):
    """a host-side split of float32 rows into (hi, lo) halves, for cases built without a GPU: hi = f16(x), lo = f16((x - hi) * 64)"""
    hi = x.half()
    lo = ((x - hi.float()) * 64.0).half()
    return (hi.view(torch.int16).to(torch.int32) & 0xFFFF) | (lo.view(torch.int16).to(torch.int32) << 16)


def head_wgrad(case, dtype=torch.float64, device="cpu", mutate=None):
    """dw = dy^T x [n][k], db = dy.sum(0) [n]; with case["x_words"] the rows are first decoded from the split format."""
    c = _to(case, dtype, device)
    x = decode_split(c["x_words"], dtype) if c.get("x_words") is not None else c["x"]
    dy = c["dy"]
    return _finish(dict(dw=dy.t() @ x, db=dy.sum(0)), dict(dw=dy[:, :, None] * x[:, None, :], db=dy), mutate)


def make_head_case(M, n, k, seed, split=False):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    dy, x = torch.randn(M, n, generator=gen), torch.randn(M, k, generator=gen)
    return dict(dy=dy, x=x, x_words=encode_split(x) if split else None)


# ---- lt_partial_sums -------------------------------------------------------------------------------------------------------------------
def partial_sums(case, dtype=torch.float64, device="cpu", mutate=None):
    """sum[e] = sum over b < nblk of ws[b * stride + e], e < count"""
    c = _to(case, dtype, device)
    part = c["ws"][:c["nblk"] * c["stride"]].view(c["nblk"], c["stride"])[:, :c["count"]]
    return _finish(dict(sum=part.sum(0)), dict(sum=part), mutate)


def make_sums_case(nblk, stride, count, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return dict(ws=torch.randn(nblk * stride, generator=gen), nblk=nblk, stride=stride, count=count)


# ---- lt_ppo_lr_rule --------------------------------------------------------------------------------------------------------------------
def lr_rule(kl, desired, lr_min, lr_max, factor, lr, stats=None, scalars=None):
    """The adaptive rule of ppo.py:273-281 in numpy.float32 arithmetic, one IEEE operation per step as the kernel has them - the
    expectation is bit equality.  kl None or desired <= 0: the rate stays.  -> (lr, stats): stats += (scalars[2], scalars[1], scalars[3])."""
    f = np.float32
    lr = f(lr)
    if kl is not None and f(desired) > f(0):
        kl, desired = f(kl), f(desired)
        if kl > desired * f(2):
            lr = max(f(lr_min), lr / f(factor))
        elif kl < desired * f(0.5) and kl > f(0):
            lr = min(f(lr_max), lr * f(factor))
    if stats is not None and scalars is not None:
        stats = np.array([f(stats[0]) + f(scalars[2]), f(stats[1]) + f(scalars[1]), f(stats[2]) + f(scalars[3])], dtype=f)
    return lr, stats


# ---- the comparator --------------------------------------------------------------------------------------------------------------------
def sequential(res32):
    """The reduced outputs of a float32 CPU result added in float32 in row order - the plainest order anyone would write, as a third
    baseline (a single float32 library sum is one lucky or unlucky draw).  numpy's cumsum: torch's accumulates float32 in double on the CPU."""
    return {n: torch.from_numpy(np.array(np.cumsum(t.cpu().numpy().astype(np.float32), axis=0, dtype=np.float32)[-1])) for n, t in res32["_terms"].items()}


def names_of(res, ref64):
    return [n for n in res if not n.startswith("_") and n not in EXACT_ONLY and n in ref64]


def errors(res, ref64, names):
    """Per named array.  Elementwise outputs: e(X) = max |X - X64| / max |X64|, no clamp, no element left out.  Reduced outputs (those
    with ref64["_terms"]): e(X) = max over elements of |X - X64| / sum |summands of X64|.  A NaN or an infinity gives inf."""
    out = {}
    for name in names:
        r = ref64[name]
        g = res[name].detach().to(device="cpu", dtype=torch.float64)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        diff = (g - r).abs()
        if not torch.isfinite(g).all():
            out[name] = float("inf")
        elif name in ref64["_terms"]:
            scale = ref64["_terms"][name].abs().sum(0)
            q = torch.where(scale > 0.0, diff / scale, torch.where(diff == 0.0, 0.0, float("inf")).to(diff.dtype))
            out[name] = float(q.max())
        else:
            d, scale = float(diff.max()), float(r.abs().max())
            out[name] = d / scale if scale > 0.0 else (0.0 if d == 0.0 else float("inf"))
    return out


def compare(res, ref64, baselines, names=None):
    """name -> (e_kernel, [e_baseline ...], ratio), ratio = e_kernel / (max(e_baseline) + EPS); the kernel passes an array when
    ratio <= FACTOR, i.e. e_kernel <= FACTOR max(e_baseline) + FACTOR * EPS (tests/seq_ref.py `compare` has the reasons for both).
    A baseline that lacks an array (`sequential` holds the reduced ones only) is not asked about it."""
    names = names_of(res, ref64) if names is None else names
    e_k = errors(res, ref64, names)
    e_b = [errors(b, ref64, [n for n in names if n in b]) for b in baselines]
    return {n: (e_k[n], [e[n] for e in e_b if n in e], e_k[n] / (max(e[n] for e in e_b if n in e) + EPS)) for n in names}


def failures(report):
    return {n: v for n, v in report.items() if not v[2] <= FACTOR}


def worst(report):
    """(array name, ratio) of the largest ratio"""
    name = max(report, key=lambda n: report[n][2] if report[n][2] == report[n][2] else float("inf"))
    return name, report[name][2]


def format_report(report):
    return " ".join(f"{n}:{v[0]:.1e}/" + "/".join(f"{b:.1e}" for b in v[1]) + f"={v[2]:.2f}" for n, v in report.items())


def exact_problems(res, block_rows=None):
    """The equalities that hold with no tolerance, over a result's OWN arrays: amax_mu == max |dmu|, amax_v == max |dvalue| (the scales
    the backward chain brings the gradients into f16's range by: too small a value overflows f16 silently), amax_blocks[b] == max |dz|
    over block b's rows.  -> {array: what differs}"""
    bad = {}
    pairs = [(n, res[src].abs().max()) for n, src in (("amax_mu", "dmu"), ("amax_v", "dvalue")) if n in res]
    if "amax_blocks" in res:
        pairs.append(("amax_blocks", block_amax(res["dz"], block_rows)))
    for name, want in pairs:
        got = res[name].detach().cpu().float().reshape(want.shape)
        want = want.detach().cpu().float()
        if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
            bad[name] = f"{got.flatten().tolist()[:4]} != max |.| of the own array {want.flatten().tolist()[:4]}"
    return bad


# ---- the cases tests/test_hip_ppo_f64.py runs (tests/test_ppo_ref.py checks the generators and the comparator on the same ones) --------
LOSS_CASES = [  # (M, A, clipped value loss, variant): one block, an exact block, a block plus one row, 17 blocks of atomics
    (1, 12, 1, "plain"), (255, 1, 1, "plain"), (256, 16, 1, "plain"), (257, 12, 1, "plain"), (4099, 12, 1, "plain"),
    (255, 1, 0, "plain"), (4099, 12, 0, "plain"),
    (257, 12, 1, "index"),      # the batch tensors are 3 M rows of storage, NaN wherever idx does not point
    (256, 12, 1, "boundary"),   # value - old_value == +- clip exactly on a share of the rows
    (257, 12, 1, "no_out"),     # out == NULL: judged on dmu, dvalue and acc
]


def loss_case(M, A, clipped, variant):
    """value_loss_coef = 0.5 at M = 257 and 1 elsewhere; entropy_coef = 0.01"""
    return make_loss_case(M, A, seed=1000 * M + 10 * A + clipped, clipped=clipped, rows=3 * M if variant == "index" else None,
                          boundary=variant == "boundary", vcoef=0.5 if M == 257 else 1.0, ecoef=0.01)


GAE_CASES = [(1, 1, False), (3, 255, False), (24, 256, True), (7, 257, False)]  # (T, N, rewards of order 0.01 against values of order 10)
# (n, regime, variant): n = 1, one block less one, an exact block, a block plus one, and 66 blocks (the second round of the loop over
# block sums).  dev: the rate in a device scalar; null_norm: grad_norm == NULL; two_steps: step 1, then step 2 on the state it wrote
ADAM_CASES = [(1, "above", "host"), (2047, "below", "host"), (2047, "below", "dev"), (2048, "no_clip", "null_norm"), (2049, "decay", "host"),
              (2049, "tiny", "host"), (2049, "above", "two_steps"), (65 * 2048 + 5, "above", "host"), (65 * 2048 + 5, "decay", "dev")]
ELU_SHAPES = [(1, 4), (47, 12), (48, 128), (49, 400), (2407, 1024)]  # a block less one row, an exact one, one more; one row lane at N = 1024
# (M, n, k, x in the split format): every NN instantiation with n below it; 256, 8, 2 and 1 row lanes; 51 blocks at M = 4801
HEAD_CASES = [(1, 1, 4, False), (95, 3, 128, False), (96, 8, 400, False), (97, 12, 128, False), (97, 12, 128, True), (293, 13, 1024, False),
              (293, 13, 1024, True), (4801, 16, 8, False)]
# 24 jobs, the most one launch takes: (nblk, stride, count, split, out1 given, ws off 16-byte alignment by one float).  nblk below and from
# 96 (4 and 16 row lanes), left-over partials of 1 .. 3 per lane; whole float4 columns, a count that is no multiple of 4, a stride that
# is none (scalar loads), a misaligned ws; split < count with out1 and without (those elements are then dropped)
SUMS_JOBS = [job for nblk in (1, 3, 95, 96, 97, 513) for job in ((nblk, 520, 520, 520, False, False), (nblk, 144, 129, 128, True, False),
                                                                  (nblk, 37, 37, 20, False, False), (nblk, 64, 61, 61, False, True))]
