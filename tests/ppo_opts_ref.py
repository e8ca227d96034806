"""A plain-torch restatement of the three entry points of include/lt_ppo_opts.h (`lt_std_from_log`, `lt_ppo_loss_opts`, `lt_adv_stats`;
csrc/lt_ppo.hip), built on the loss oracle and the case generator of tests/ppo_ref.py, with seeded cases and the mutations
tests/test_ppo_opts_ref.py rejects.  Nothing here needs a GPU; tests/test_hip_ppo_opts_f64.py holds the kernels to it with the
comparator of tests/ppo_ref.py.

As there, every function is ONE text for every role (`dtype`, `device`): float64 on the CPU is the oracle, float32 on the CPU and on the
GPU are baselines, and the inputs are the float32 values that cross the C ABI.

A loss case is a case of `ppo_ref.make_loss_case` with two more keys: `std_is_log` (then case["std"] holds LOG sigma) and `adv_stats`
(None, or the two floats (mean, 1 / (std + 1e-8)) the advantages are normalised with where they are loaded).  `plain_case` turns it
into the case `ppo_ref.ppo_loss` takes - sigma = exp(log sigma), advantages normalised - in the role's own arithmetic; the loss and its
gradients with respect to mu, value and SIGMA are then that oracle's (autograd), and the gradient with respect to log sigma is the
sigma gradient times sigma, row by row - the one hand-written line, which tests/test_ppo_opts_ref.py checks against autograd through
this repository's `ActorCritic(noise_std_type="log")`."""
import torch

from tests import ppo_ref as R

ADV_EPS = R.f32(1.0e-8)  # the kernel's 1.0e-8f; the reference's Python 1e-8 meets a float32 tensor and is rounded the same way

# mutation -> (entry point, an array that must reject it)
MUTATIONS = {
    "chain_rule_factor_left_out": ("ppo_loss_opts", "dstd"),         # the sigma gradient handed to log sigma as it is
    "entropy_minus_ecoef_left_out": ("ppo_loss_opts", "dstd"),       # the entropy's share of d loss / d log sigma (-entropy_coef) missing
    "biased_std": ("adv_stats", "inv_std"),                          # / M in place of / (M - 1)
    "without_1e-8": ("adv_stats", "inv_std"),                        # 1 / std
    "mean_over_whole_storage": ("adv_stats", "mean"),                # the mean of every stored advantage, not of the minibatch's rows
    "one_pass_variance": ("adv_stats", "inv_std"),                   # E[x^2] - E[x]^2
}


# ---- lt_std_from_log -------------------------------------------------------------------------------------------------------------------
def std_from_log(case, dtype=torch.float64, device="cpu", mutate=None):
    c = R._to(case, dtype, device)
    return R._finish(dict(std=torch.exp(c["log_std"])), {}, mutate)


def make_log_std_case(A, seed):
    """log sigma spread over [-5, 2] (sigma from 0.007 to 7.4), both ends included from A = 2"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    log_std = -5.0 + 7.0 * torch.rand(A, generator=gen)
    if A >= 2:
        log_std[0], log_std[-1] = -5.0, 2.0
    return dict(log_std=log_std)


# ---- lt_ppo_loss_opts ------------------------------------------------------------------------------------------------------------------
def plain_case(case, dtype=torch.float64, device="cpu"):
    """the case `ppo_ref.ppo_loss` / `ppo_ref.loss_branches` take: std = sigma, adv = the advantages as the loss sees them"""
    c = R._to(case, dtype, device)
    if c.get("adv_stats") is not None:
        c["adv"] = (c["adv"] - c["adv_stats"][0]) * c["adv_stats"][1]
    if c.get("std_is_log"):
        c["std"] = torch.exp(c["std"])
    return c


def ppo_loss_opts(case, dtype=torch.float64, device="cpu", mutate=None):
    """`ppo_ref.ppo_loss` of `plain_case`; with std_is_log the arrays dstd / acc_dstd (out[8 + a] / acc[4 + a]) are the gradients with
    respect to log sigma_a: acc_dstd = sum over rows of (d surrogate / d sigma_a) sigma_a, dstd = acc_dstd - entropy_coef."""
    c = plain_case(case, dtype, device)
    res = R.ppo_loss(c, dtype=dtype, device=device)
    if not c.get("std_is_log"):
        return R._finish({k: v for k, v in res.items() if k != "_terms"}, res["_terms"], mutate)
    terms = dict(res["_terms"])
    sigma, A = c["std"], c["std"].shape[0]
    if mutate != "chain_rule_factor_left_out":
        rows = terms["acc_dstd"] * sigma
        share = torch.zeros(A, dtype=dtype, device=device) if mutate == "entropy_minus_ecoef_left_out" else torch.full((A,), -c["ecoef"], dtype=dtype, device=device)
        terms["acc_dstd"], terms["dstd"] = rows, torch.cat([rows, share[None]])
        res = dict(res, acc_dstd=rows.sum(0), dstd=rows.sum(0) + share)
    return R._finish({k: v for k, v in res.items() if k != "_terms"}, terms, mutate)


def make_opts_case(M, A, seed, clipped, std_is_log, normalise, rows=None, vcoef=1.0, ecoef=0.01):
    """`ppo_ref.make_loss_case` with the options on.  std_is_log: std becomes the float32 log of the generator's sigma (the sigma the
    loss forms moves by a rounding of that log: a few 1e-8 of the log-ratio, far inside the generator's margin - checked, not assumed,
    by tests/test_ppo_opts_ref.py).  normalise: adv_stats = (0.35, 1 / 0.8) + small seeded offsets, the scale of a real minibatch's
    statistics - every advantage below 0.35 changes its sign, the planted zeros stop being zeros."""
    case = R.make_loss_case(M, A, seed, clipped, rows=rows, vcoef=vcoef, ecoef=ecoef)
    gen = torch.Generator(device="cpu").manual_seed(seed + 77)
    case["std_is_log"] = int(bool(std_is_log))
    if std_is_log:
        case["std"] = torch.log(case["std"].double()).float()
    case["adv_stats"] = None
    if normalise:
        case["adv_stats"] = torch.tensor([0.35, 1.25]) + 0.05 * torch.rand(2, generator=gen)
    return case


OPTS = {"log": (1, 0), "norm": (0, 1), "both": (1, 1)}  # option set -> (std_is_log, adv_stats given)
# (M, A, clipped, variant) x every option set: the M values of ppo_ref.LOSS_CASES (one block, an exact block, a block plus one row,
# 17 blocks), A in {1, 12, 16}, with and without idx
OPTS_SHAPES = [(1, 12, 1, "plain"), (255, 1, 1, "plain"), (256, 16, 1, "plain"), (257, 12, 1, "index"), (4099, 12, 1, "plain"), (255, 16, 0, "index")]
OPTS_CASES = [(*s, o) for s in OPTS_SHAPES for o in OPTS]


def opts_case(M, A, clipped, variant, opts):
    log, norm = OPTS[opts]
    return make_opts_case(M, A, seed=1000 * M + 10 * A + clipped, clipped=clipped, std_is_log=log, normalise=norm,
                          rows=3 * M if variant == "index" else None, vcoef=0.5 if M == 257 else 1.0)


def margin_problems(case):
    """Rows of an options case that lie within `ppo_ref.MARGIN` of a branch boundary in float64, by `ppo_ref.loss_branches`: a row's class
    (inside / above / below the ratio clip; inside / outside the value clip) must be the same with the clip range narrowed and widened
    by MARGIN, and the float32 form must take the float64 branch on every row.  -> {what: rows}"""
    c64 = plain_case(case)
    b = R.loss_branches(c64)
    bad = {}
    for d in (-R.MARGIN, R.MARGIN):
        moved = R.loss_branches(dict(c64, clip=c64["clip"] + d))
        for k in ("inside", "above", "below") + (("v_inside",) if case["clipped"] else ()):
            n = int((moved[k] != b[k]).sum())
            if n:
                bad[f"{k} at clip{d:+g}"] = n
    b32 = R.loss_branches(plain_case(case, dtype=torch.float32), dtype=torch.float32)
    for k in b:
        if (k.startswith("v_") and not case["clipped"]) or torch.equal(b[k], b32[k]):
            continue
        bad[f"{k} float32 != float64"] = int((b[k] != b32[k]).sum())
    return bad


# ---- lt_adv_stats ----------------------------------------------------------------------------------------------------------------------
def adv_stats(case, dtype=torch.float64, device="cpu", mutate=None):
    """ppo.py:223-225 per minibatch: mean and 1 / (unbiased std + 1e-8) of rows idx[b M .. (b + 1) M) of `adv` (idx None: the rows
    themselves).  Arrays mean [nmb], inv_std [nmb]."""
    c = R._to(case, dtype, device)
    M, nmb = c["M"], c["nmb"]
    rows = (c["adv"][:nmb * M] if c["idx"] is None else c["adv"][c["idx"][:nmb * M]]).view(nmb, M)
    mean = rows.mean(1)
    if mutate == "mean_over_whole_storage":
        mean = c["adv"].mean().expand(nmb).clone()
    if mutate == "one_pass_variance":
        std = torch.sqrt(((rows * rows).mean(1) - mean * mean).clamp_min(0.0) * (M / (M - 1.0)))
    else:
        std = rows.std(1, unbiased=mutate != "biased_std")
    inv = 1.0 / (std + (0.0 if mutate == "without_1e-8" else ADV_EPS))
    return R._finish(dict(mean=mean, inv_std=inv), dict(mean=rows.t() / M), mutate)


def make_adv_case(M, nmb, seed, kind="plain", storage=None):
    """kind: plain N(0.3, 1.7^2), a different offset per minibatch; `offset` mean 10 and spread 1e-3 (x^2 then carries 10^8 times the
    variance: a one-pass form loses it all in float32); `small` N(0, (1e-5)^2) (the 1e-8 is then a thousandth of the std).
    storage = R > nmb M: idx is the first nmb M entries of a permutation of R rows; the other rows hold 7 + randn (finite, so that a mean
    over the whole storage is a wrong NUMBER; the GPU test overwrites them with NaN to show they are never read)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rows = torch.randn(nmb, M, generator=gen)
    if kind == "offset":
        rows = 10.0 + 1.0e-3 * rows
    elif kind == "small":
        rows = 1.0e-5 * rows
    else:
        rows = 0.3 + 1.7 * rows + 0.5 * torch.arange(nmb).float()[:, None]
    if storage is None:
        return dict(adv=rows.reshape(-1).clone(), idx=None, M=M, nmb=nmb)
    assert storage > nmb * M
    perm = torch.randperm(storage, generator=gen)
    adv = 7.0 + torch.randn(storage, generator=gen)
    adv[perm[:nmb * M]] = rows.reshape(-1)
    return dict(adv=adv, idx=perm[:nmb * M].clone(), M=M, nmb=nmb, unread=perm[nmb * M:])


# (M, nmb, kind, storage rows or None): M = 2, a block of 256 less one, a block plus one; nmb 1 and 4
ADV_CASES = [(2, 1, "plain", None), (2, 4, "plain", None), (255, 1, "plain", None), (255, 4, "plain", None), (257, 1, "plain", None),
             (257, 4, "plain", None), (257, 4, "offset", None), (257, 4, "plain", 3 * 4 * 257 + 5), (6144, 4, "plain", 4 * 6144 + 100)]


def adv_case(M, nmb, kind, storage):
    return make_adv_case(M, nmb, seed=10 * M + nmb, kind=kind, storage=storage)
