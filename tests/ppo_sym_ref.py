"""A plain-torch restatement of two entry points of include/lt_ppo_sym.h (`lt_ppo_loss_sym`, `lt_sym_gather_rows`; csrc/lt_ppo_sym.hip),
built on the loss oracle and the case generators of tests/ppo_ref.py and tests/ppo_opts_ref.py, with seeded cases and the mutations
tests/test_ppo_sym_ref.py rejects.  Nothing here needs a GPU; tests/test_hip_ppo_sym_f64.py holds the kernels to it with the comparator of
tests/ppo_ref.py.

As there, every function is ONE text for every role (`dtype`, `device`): float64 on the CPU is the oracle, float32 on the CPU and on the
GPU are baselines, and the inputs are the float32 values that cross the C ABI.  Gradients are autograd's.

A loss case is a case of `ppo_opts_ref.make_opts_case` whose `mu` [2 M][A] and `value` [2 M] hold the forward outputs of the augmented
batch [original; mirrored], with three more keys: `act_src` (int64 [A]) and `act_sign` ([A], +-1) - the action table - and `mirror_coeff`.
Row M + r is scored against the mirrored action sign_a * actions[idx[r]][src_a] with row r's old log-prob, advantage, return and old
value; sigma is not permuted."""
import torch

from tests import ppo_opts_ref as O
from tests import ppo_ref as R

# mutation -> (entry point, an array that must reject it)
MUTATIONS = {
    "kl_over_all_2m_rows": ("ppo_loss_sym", "kl"),
    "divisor_m_in_place_of_2m": ("ppo_loss_sym", "dvalue"),
    "actions_not_mirrored": ("ppo_loss_sym", "dmu"),
    "action_sign_left_out": ("ppo_loss_sym", "dmu"),
    "mirror_gradient_also_into_the_original_half": ("ppo_loss_sym", "dmu"),
    "mse_divided_by_m": ("ppo_loss_sym", "symmetry"),
    "sigma_permuted": ("ppo_loss_sym", "dmu"),
    "mirror_term_missing_from_amax": ("ppo_loss_sym", "amax_mu"),
}


def mirror(x, src, sign, with_sign=True):
    y = x[..., src]
    return y * sign if with_sign else y


def ppo_loss_sym(case, dtype=torch.float64, device="cpu", mutate=None):
    """The minibatch loss of loco_rl/algorithms/ppo.py:216-337 with data augmentation on, and its gradients.

    Arrays: dmu [2 M][A], dvalue [2 M], dstd [A] (std_is_log: the gradient with respect to log sigma), loss, surrogate, value_loss,
    entropy, kl, symmetry (out[0 .. 5]); acc_surrogate, acc_value_loss, acc_kl, acc_sym (the row SUMS, acc[0 .. 3]), acc_dstd [A]
    (acc[4 + a]); amax_mu, amax_v = max |dmu|, max |dvalue| of THESE arrays over both halves (acc[20], acc[21])."""
    c = O.plain_case(case, dtype, device)
    M2, A = c["mu"].shape
    M = M2 // 2
    b = R._gathered(c)
    src, sign, coeff = c["act_src"], c["act_sign"], c["mirror_coeff"]
    clip, vcoef, ecoef = c["clip"], c["vcoef"], c["ecoef"]
    twice = lambda t: torch.cat([t, t])  # noqa: E731
    if mutate == "actions_not_mirrored":
        actions = twice(b["actions"])
    else:
        actions = torch.cat([b["actions"], mirror(b["actions"], src, sign, with_sign=mutate != "action_sign_left_out")])
    old_logp, adv, returns, old_values = (twice(b[k]) for k in ("old_logp", "adv", "returns", "old_values"))
    mu, value, std = (c[k].clone().requires_grad_(True) for k in ("mu", "value", "std"))
    sig = c["std"].expand(M2, A).clone().requires_grad_(True)  # the std as a leaf PER ROW on the log-prob's side (tests/ppo_ref.py)
    sig_used = torch.cat([sig[:M], sig[M:][:, src]]) if mutate == "sigma_permuted" else sig
    logp = R._log_prob(actions, mu, sig_used).sum(-1)
    with torch.no_grad():
        if mutate == "kl_over_all_2m_rows":
            om, os_, m_kl, s_kl, n_kl = twice(b["old_mu"]), twice(b["old_sigma"]), mu, sig, M2
        else:
            om, os_, m_kl, s_kl, n_kl = b["old_mu"], b["old_sigma"], mu[:M], sig[:M], M
        kl_rows = (torch.log(s_kl / os_ + R.KL_EPS) + (os_ ** 2 + (om - m_kl) ** 2) / (2.0 * s_kl ** 2) - 0.5).sum(-1)
    ratio = torch.exp(logp - old_logp)
    surr_rows = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip))
    if c["clipped"]:
        d = value - old_values
        vl_rows = torch.max((value - returns) ** 2, (old_values + d.clamp(-clip, clip) - returns) ** 2)
    else:
        vl_rows = (returns - value) ** 2
    ent_terms = 0.5 + R.HALF_LOG_2PI + torch.log(std)
    n = M if mutate == "divisor_m_in_place_of_2m" else M2
    surrogate, value_loss, kl, entropy = surr_rows.sum() / n, vl_rows.sum() / n, kl_rows.sum() / n_kl, ent_terms.sum()
    target = mirror(mu[:M], src, sign)
    if mutate != "mirror_gradient_also_into_the_original_half":
        target = target.detach()
    diff = mu[M:] - target
    sq_rows = (diff * diff).sum(-1)
    symmetry = sq_rows.sum() / (M if mutate == "mse_divided_by_m" else M * A)
    loss = surrogate + vcoef * value_loss - ecoef * entropy + coeff * symmetry
    loss.backward()
    dstd_entropy = std.grad if std.grad is not None else torch.zeros_like(std)
    dmu, dvalue, dstd_rows = mu.grad, value.grad, sig.grad
    if c.get("std_is_log"):  # the chain rule's factor sigma_a, row by row; the entropy's share of d loss / d log sigma_a is -ecoef
        dstd_rows = dstd_rows * c["std"]
        dstd_entropy = torch.full((A,), -ecoef, dtype=dtype, device=device)
    amax_mu = dmu.abs().max()
    if mutate == "mirror_term_missing_from_amax":
        plain = dmu.clone()
        plain[M:] -= coeff * 2.0 * diff.detach() / (M * A)
        amax_mu = plain.abs().max()
    res = dict(dmu=dmu, dvalue=dvalue, dstd=dstd_rows.sum(0) + dstd_entropy, loss=loss, surrogate=surrogate, value_loss=value_loss, entropy=entropy,
               kl=kl, symmetry=symmetry, acc_surrogate=surr_rows.sum(), acc_value_loss=vl_rows.sum(), acc_kl=kl_rows.sum(), acc_sym=sq_rows.sum(),
               acc_dstd=dstd_rows.sum(0), amax_mu=amax_mu, amax_v=dvalue.abs().max())
    ent = ent_terms.detach()
    terms = dict(surrogate=surr_rows / n, value_loss=vl_rows / n, kl=kl_rows / n_kl, entropy=ent, symmetry=sq_rows / (M * A), acc_surrogate=surr_rows,
                 acc_value_loss=vl_rows, acc_kl=kl_rows, acc_sym=sq_rows, acc_dstd=dstd_rows, dstd=torch.cat([dstd_rows, dstd_entropy[None]]),
                 loss=torch.cat([surr_rows / n, vcoef * vl_rows / n, -ecoef * ent, coeff * sq_rows / (M * A)]))
    return R._finish(res, terms, mutate)


def action_table(A, seed):
    """a signed permutation of A columns: the Go1's for A = 12 (legs swapped in pairs, hips negated), seeded pair swaps otherwise (an
    involution with fixed points for odd A; A = 1: the sign alone)"""
    if A == 12:
        return torch.tensor([1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10]), torch.tensor([-1.0] * 4 + [1.0] * 8)
    gen = torch.Generator(device="cpu").manual_seed(seed + 5)
    order = torch.randperm(A, generator=gen)
    src = torch.arange(A)
    for k in range(0, A - 1, 2):
        i, j = int(order[k]), int(order[k + 1])
        src[i], src[j] = j, i
    sign = torch.where(torch.rand(A, generator=gen) < 0.5, -1.0, 1.0)
    sign[src] = sign.clone()  # the same sign on both members of a pair: the map is an involution
    if A == 1:
        sign[0] = -1.0
    return src, sign


def half_case(case, h, dtype=torch.float64):
    """half h (0: original, 1: mirrored) of a symmetric case as the plain case `ppo_ref.loss_branches` takes"""
    c = O.plain_case(case, dtype, "cpu")
    M = c["mu"].shape[0] // 2
    b = R._gathered(c)
    if h == 1:
        b["actions"] = mirror(b["actions"], c["act_src"], c["act_sign"])
    return dict(b, mu=c["mu"][h * M:(h + 1) * M], value=c["value"][h * M:(h + 1) * M], std=c["std"], idx=None, clip=c["clip"], clipped=c["clipped"])


def _near(hc, clipped):
    """rows of a half case within `ppo_ref.MARGIN` of a branch boundary (float64), by the rule of `ppo_ref.make_loss_case`"""
    clip = hc["clip"]
    ratio = torch.exp(R._log_prob(hc["actions"], hc["mu"], hc["std"].expand_as(hc["mu"])).sum(-1) - hc["old_logp"])
    bad = ((ratio - (1.0 - clip)).abs() < R.MARGIN) | ((ratio - (1.0 + clip)).abs() < R.MARGIN)
    if clipped:
        d = hc["value"] - hc["old_values"]
        l1, l2 = (hc["value"] - hc["returns"]) ** 2, (hc["old_values"] + d.clamp(-clip, clip) - hc["returns"]) ** 2
        bad |= (d.abs() - clip).abs() < R.MARGIN
        bad |= (d.abs() > clip) & ((l1 - l2).abs() < R.MARGIN * torch.maximum(l1, l2))
    return bad


def make_sym_case(M, A, seed, clipped, std_is_log, normalise, mirror_coeff, rows=None, vcoef=1.0, ecoef=0.01):
    """`ppo_opts_ref.make_opts_case` for the first half; the second half's mu and value are drawn so that it is a case of the SAME family
    under the mirrored actions: with z_old the behaviour policy's standardised residual of the stored action and delta = sigma / old_sigma -
    1, the first half has z = (z_old - c randn) / (1 + delta); the second half gets z' = (mirror(z_old) - c randn) / (1 + delta), i.e.
    mu[M + r] = mirror(action) - sigma z', and value[M + r] = old_value + 0.3 randn.  Rows of the second half within MARGIN of a boundary
    are drawn again (their mu and value alone: the storage rows are shared with the first half)."""
    case = O.make_opts_case(M, A, seed, clipped, std_is_log, normalise, rows=rows, vcoef=vcoef, ecoef=ecoef)
    gen = torch.Generator(device="cpu").manual_seed(seed + 177)
    src, sign = action_table(A, seed)
    case.update(act_src=src, act_sign=sign, mirror_coeff=R.f32(mirror_coeff))
    sigma = (torch.exp(case["std"].double()) if std_is_log else case["std"].double())
    b = {k: v.double() for k, v in R._gathered(case).items()}
    z_old = mirror((b["actions"] - b["old_mu"]) / b["old_sigma"], src, sign.double())
    ratio_sig = sigma / b["old_sigma"][0]  # 1 + delta (the old sigma is state-independent)
    c_mu = 0.05 * max(1.0, (12.0 / A) ** 0.8)
    xm = mirror(b["actions"], src, sign.double())

    def draw(k, zo, x, ov):
        z = (zo - c_mu * torch.randn(k, A, generator=gen).double()) / ratio_sig
        return (x - sigma * z).float(), (ov + 0.3 * torch.randn(k, generator=gen).double()).float()

    mu1, v1 = draw(M, z_old, xm, b["old_values"])
    redrawn = 0
    while True:
        case["mu"], case["value"] = torch.cat([case["mu"][:M], mu1]), torch.cat([case["value"][:M], v1])
        bad = _near(half_case(case, 1), clipped)
        k = int(bad.sum())
        if k == 0:
            break
        redrawn += k
        mu1[bad], v1[bad] = draw(k, z_old[bad], xm[bad], b["old_values"][bad])
    case["redrawn_mirrored"] = redrawn
    return case


def branch_problems(case):
    """Per half: rows within MARGIN of a branch boundary in float64 (a row's class must be the same with the clip range narrowed and
    widened by MARGIN), and rows whose float32 form takes another branch than float64.  -> {what: rows}"""
    bad = {}
    for h in (0, 1):
        c64 = half_case(case, h)
        base = R.loss_branches(c64)
        for d in (-R.MARGIN, R.MARGIN):
            moved = R.loss_branches(dict(c64, clip=c64["clip"] + d))
            for k in ("inside", "above", "below") + (("v_inside",) if case["clipped"] else ()):
                n = int((moved[k] != base[k]).sum())
                if n:
                    bad[f"half {h}: {k} at clip{d:+g}"] = n
        b32 = R.loss_branches(half_case(case, h, dtype=torch.float32), dtype=torch.float32)
        for k in base:
            if (k.startswith("v_") and not case["clipped"]) or torch.equal(base[k], b32[k]):
                continue
            bad[f"half {h}: {k} float32 != float64"] = int((base[k] != b32[k]).sum())
    return bad


def branch_counts(case):
    """half -> {class: rows} of `ppo_ref.loss_branches`"""
    return {h: {k: int(v.sum()) for k, v in R.loss_branches(half_case(case, h)).items()} for h in (0, 1)}


SYM_OPTS = {"plain": (0, 0), "log": (1, 0), "norm": (0, 1), "both": (1, 1)}  # option set -> (std_is_log, adv_stats given)
# tests/ppo_opts_ref.py OPTS_SHAPES x every option set x mirror_coeff in {0, 0.5}
SYM_CASES = [(*s, o, k) for s in O.OPTS_SHAPES for o in SYM_OPTS for k in (0.0, 0.5)]


def sym_case(M, A, clipped, variant, opts, coeff):
    log, norm = SYM_OPTS[opts]
    return make_sym_case(M, A, seed=1000 * M + 10 * A + clipped, clipped=clipped, std_is_log=log, normalise=norm, mirror_coeff=coeff,
                         rows=3 * M if variant == "index" else None, vcoef=0.5 if M == 257 else 1.0)


# ---- lt_sym_gather_rows ----------------------------------------------------------------------------------------------------------------
def sym_gather(case):
    """f32 [nmb][2][m][D]: minibatch b's m storage rows, then their mirror images.  Copies, sign flips and the exact bf16 -> f32 widening
    only: every role gives the same bits, there is one statement and no tolerance."""
    rows = case["rows"].float()[case["idx"]]
    nmb, m, D = case["nmb"], case["m"], rows.shape[1]
    both = torch.stack([rows.view(nmb, m, D), mirror(rows, case["src"], case["sign"]).view(nmb, m, D)], dim=1)
    return both.contiguous()


def signed_permutation(D, seed):
    """a seeded signed permutation of D columns (not an involution: the kernel serves any)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randperm(D, generator=gen), torch.where(torch.rand(D, generator=gen) < 0.5, -1.0, 1.0)


def make_gather_case(D, m, nmb, bf16, seed, table=None):
    """storage of R = 2 nmb m + 3 rows; idx a random injection; rows no index refers to are NaN (never read)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    R_ = 2 * nmb * m + 3
    idx = torch.randperm(R_, generator=gen)[:nmb * m]
    rows = torch.full((R_, D), float("nan"))
    rows[idx] = torch.randn(nmb * m, D, generator=gen)
    src, sign = table if table is not None else signed_permutation(D, seed + 1)
    return dict(rows=rows.bfloat16() if bf16 else rows, idx=idx, nmb=nmb, m=m, src=src, sign=sign)


GATHER_CASES = [(D, m, nmb, bf16) for D in (1, 13, 270, 348) for m in (1, 63, 64, 65) for nmb in (1, 4) for bf16 in (False, True)]
