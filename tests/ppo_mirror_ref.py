"""A plain-torch restatement of `lt_ppo_loss_mirror` (include/lt_ppo_mirror.h; csrc/lt_ppo_sym.hip): the PPO minibatch loss with the
mirror loss and NO data augmentation, built on tests/ppo_sym_ref.py (`mirror`, `action_table`, `make_sym_case`, `branch_problems`), with
seeded cases and the mutations tests/test_ppo_mirror_ref.py rejects.  Nothing here needs a GPU; tests/test_hip_ppo_mirror_f64.py holds the
kernel to it with the comparator of tests/ppo_ref.py.

As there, the function is ONE text for every role (`dtype`, `device`): float64 on the CPU is the oracle, float32 on the CPU and on the
GPU are baselines, and the inputs are the float32 values that cross the C ABI.  Gradients are autograd's.

A case is a case of `ppo_sym_ref.make_sym_case` - `mu` [2 M][A] holds the actor's output on [original; mirrored] rows - whose `value` is
cut to the M original rows: the critic never sees a mirrored row.  Rows r < M are scored as `ppo_opts_ref.ppo_loss_opts` scores them, every
mean over M rows; the mirror term compares mu[M + r] with the (detached) mirror of mu[r] and sends its gradient into row M + r alone."""
import torch

from tests import ppo_opts_ref as O
from tests import ppo_ref as R
from tests import ppo_sym_ref as S

# mutation -> (entry point, an array that must reject it)
MUTATIONS = {
    "divisor_2m_where_m_belongs": ("ppo_loss_mirror", "dvalue"),
    "mirror_gradient_also_into_row_r": ("ppo_loss_mirror", "dmu"),
    "sign_left_out": ("ppo_loss_mirror", "symmetry"),
    "src_left_out": ("ppo_loss_mirror", "symmetry"),
    "coefficient_missing_from_the_loss": ("ppo_loss_mirror", "loss"),
    "kl_over_all_2m_rows": ("ppo_loss_mirror", "kl"),
    "mirrored_rows_in_the_surrogate": ("ppo_loss_mirror", "surrogate"),
    "mse_divided_by_2ma": ("ppo_loss_mirror", "symmetry"),
    "mirror_term_missing_from_amax": ("ppo_loss_mirror", "amax_mu"),
}


def ppo_loss_mirror(case, dtype=torch.float64, device="cpu", mutate=None):
    """The minibatch loss of loco_rl/algorithms/ppo.py:251-337 with `use_data_augmentation=False`, and its gradients.

    Arrays: dmu [2 M][A], dvalue [M], dstd [A] (std_is_log: the gradient with respect to log sigma), loss, surrogate, value_loss, entropy,
    kl, symmetry (out[0 .. 5]); acc_surrogate, acc_value_loss, acc_kl, acc_sym (the row SUMS, acc[0 .. 3]), acc_dstd [A] (acc[4 + a]);
    amax_mu = max |dmu| over all 2 M rows, amax_v = max |dvalue| over M rows, of THESE arrays (acc[20], acc[21])."""
    c = O.plain_case(case, dtype, device)
    M2, A = c["mu"].shape
    M = M2 // 2
    assert c["value"].shape == (M,)
    b = R._gathered(c)
    src, sign, coeff = c["act_src"], c["act_sign"], c["mirror_coeff"]
    clip, vcoef, ecoef = c["clip"], c["vcoef"], c["ecoef"]
    mu, value, std = (c[k].clone().requires_grad_(True) for k in ("mu", "value", "std"))
    wide = mutate == "mirrored_rows_in_the_surrogate"  # the mirrored rows scored against the mirrored actions, as augmentation does
    n_rows = M2 if wide else M
    sig = c["std"].expand(n_rows, A).clone().requires_grad_(True)  # the std as a leaf PER ROW on the log-prob's side (tests/ppo_ref.py)
    twice = lambda t: torch.cat([t, t])  # noqa: E731
    if wide:
        logp = R._log_prob(torch.cat([b["actions"], S.mirror(b["actions"], src, sign)]), mu, sig).sum(-1)
        old_logp, adv = twice(b["old_logp"]), twice(b["adv"])
    else:
        logp, old_logp, adv = R._log_prob(b["actions"], mu[:M], sig).sum(-1), b["old_logp"], b["adv"]
    with torch.no_grad():
        if mutate == "kl_over_all_2m_rows":
            om, os_, m_kl, s_kl, n_kl = twice(b["old_mu"]), twice(b["old_sigma"]), mu, c["std"].expand(M2, A), M2
        else:
            om, os_, m_kl, s_kl, n_kl = b["old_mu"], b["old_sigma"], mu[:M], c["std"].expand(M, A), M
        kl_rows = (torch.log(s_kl / os_ + R.KL_EPS) + (os_ ** 2 + (om - m_kl) ** 2) / (2.0 * s_kl ** 2) - 0.5).sum(-1)
    ratio = torch.exp(logp - old_logp)
    surr_rows = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip))
    if c["clipped"]:
        d = value - b["old_values"]
        vl_rows = torch.max((value - b["returns"]) ** 2, (b["old_values"] + d.clamp(-clip, clip) - b["returns"]) ** 2)
    else:
        vl_rows = (b["returns"] - value) ** 2
    ent_terms = 0.5 + R.HALF_LOG_2PI + torch.log(std)
    n = M2 if mutate == "divisor_2m_where_m_belongs" else M
    surrogate, value_loss, kl, entropy = surr_rows.sum() / n, vl_rows.sum() / n, kl_rows.sum() / n_kl, ent_terms.sum()
    if mutate == "sign_left_out":
        target = S.mirror(mu[:M], src, sign, with_sign=False)
    elif mutate == "src_left_out":
        target = mu[:M] * sign
    else:
        target = S.mirror(mu[:M], src, sign)
    if mutate != "mirror_gradient_also_into_row_r":
        target = target.detach()
    diff = mu[M:] - target
    sq_rows = (diff * diff).sum(-1)
    n_sym = 2 * M * A if mutate == "mse_divided_by_2ma" else M * A
    symmetry = sq_rows.sum() / n_sym
    loss = surrogate + vcoef * value_loss - ecoef * entropy + coeff * symmetry
    loss.backward()
    if mutate == "coefficient_missing_from_the_loss":  # (the gradients still carry the term)
        loss = loss - coeff * symmetry
    dstd_entropy = std.grad if std.grad is not None else torch.zeros_like(std)
    dmu, dvalue, dstd_rows = mu.grad, value.grad, sig.grad
    if c.get("std_is_log"):  # the chain rule's factor sigma_a, row by row; the entropy's share of d loss / d log sigma_a is -ecoef
        dstd_rows = dstd_rows * c["std"]
        dstd_entropy = torch.full((A,), -ecoef, dtype=dtype, device=device)
    amax_mu = dmu.abs().max()
    if mutate == "mirror_term_missing_from_amax":
        amax_mu = dmu[:M].abs().max()
    res = dict(dmu=dmu, dvalue=dvalue, dstd=dstd_rows.sum(0) + dstd_entropy, loss=loss, surrogate=surrogate, value_loss=value_loss, entropy=entropy,
               kl=kl, symmetry=symmetry, acc_surrogate=surr_rows.sum(), acc_value_loss=vl_rows.sum(), acc_kl=kl_rows.sum(), acc_sym=sq_rows.sum(),
               acc_dstd=dstd_rows.sum(0), amax_mu=amax_mu, amax_v=dvalue.abs().max())
    ent = ent_terms.detach()
    sym_share = torch.zeros(0, dtype=dtype, device=device) if mutate == "coefficient_missing_from_the_loss" else coeff * sq_rows / n_sym
    terms = dict(surrogate=surr_rows / n, value_loss=vl_rows / n, kl=kl_rows / n_kl, entropy=ent, symmetry=sq_rows / n_sym, acc_surrogate=surr_rows,
                 acc_value_loss=vl_rows, acc_kl=kl_rows, acc_sym=sq_rows, acc_dstd=dstd_rows, dstd=torch.cat([dstd_rows, dstd_entropy[None]]),
                 loss=torch.cat([surr_rows / n, vcoef * vl_rows / n, -ecoef * ent, sym_share]))
    return R._finish(res, terms, mutate)


def of_sym_case(sym_case):
    """the mirror case of a `ppo_sym_ref` case: the same rows, the critic's output on the M original ones alone"""
    M = sym_case["mu"].shape[0] // 2
    return dict(sym_case, value=sym_case["value"][:M].clone())


AMAX_COEFF = 4096.0  # a mirror coefficient at which the largest |dmu| of the seeded cases lies in the mirrored rows (acc[20] must see them)

# tests/ppo_opts_ref.py OPTS_SHAPES x every option set x mirror_coeff in {0, 0.5}: the cases of tests/ppo_sym_ref.py, cut
MIRROR_CASES = S.SYM_CASES


def sym_parent(M, A, clipped, variant, opts, coeff):
    """the `ppo_sym_ref` case a mirror case is cut from (`branch_problems` is asked about this one: both of its halves)"""
    return S.sym_case(M, A, clipped, variant, opts, coeff)


def mirror_case(M, A, clipped, variant, opts, coeff):
    return of_sym_case(sym_parent(M, A, clipped, variant, opts, coeff))
