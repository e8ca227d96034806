"""tests/ppo_ref.py itself, on the CPU: every oracle function is pinned to an independent float64 formulation at 1e-12, the loss-case
generator's conditions are asserted on the cases the GPU test runs, and the comparator with the exact checks is shown to pass the float32
form and to reject each of `MUTATIONS` on a named array (a float32 CPU form stands in for the kernel)."""
import functools

import numpy as np
import pytest
import torch

from tests import ppo_ref as R

F64, F32 = torch.float64, torch.float32


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


# ---- the oracle against independent formulations, float64, 1e-12 -----------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "index", "boundary"])
@pytest.mark.parametrize("clipped", [1, 0])
def test_loss_oracle_equals_the_normal_distribution_formulation(clipped, variant):
    """torch.distributions.Normal for log-prob and entropy, the KL in the closed form of the older test, ONE std leaf (the oracle's
    per-row std leaves and its row-wise entropy term must add up to that leaf's gradient)."""
    case = R.make_loss_case(300, 12, seed=7, clipped=clipped, rows=900 if variant == "index" else None, boundary=variant == "boundary",
                            vcoef=0.5, ecoef=0.01)
    res = R.ppo_loss(case)
    c = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in case.items()}
    take = (lambda t: t) if c["idx"] is None else (lambda t: t[c["idx"]])
    mu, std, value = (c[k].clone().requires_grad_(True) for k in ("mu", "std", "value"))
    dist = torch.distributions.Normal(mu, std.expand_as(mu))
    ratio = torch.exp(dist.log_prob(take(c["actions"])).sum(-1) - take(c["old_logp"]))
    adv, clip = take(c["adv"]), c["clip"]
    surrogate = torch.max(-adv * ratio, -adv * ratio.clamp(1 - clip, 1 + clip)).mean()
    if clipped:
        vclip = take(c["old_values"]) + (value - take(c["old_values"])).clamp(-clip, clip)
        value_loss = torch.max((value - take(c["returns"])).pow(2), (vclip - take(c["returns"])).pow(2)).mean()
    else:
        value_loss = (take(c["returns"]) - value).pow(2).mean()
    entropy = dist.entropy().sum(-1).mean()
    sig, osig = std.detach().expand_as(mu), take(c["old_sigma"])
    kl = torch.sum(torch.log(sig / osig + R.KL_EPS) + (osig.square() + (take(c["old_mu"]) - mu.detach()).square()) / (2.0 * sig.square()) - 0.5, -1).mean()
    loss = surrogate + c["vcoef"] * value_loss - c["ecoef"] * entropy
    loss.backward()
    want = dict(loss=loss, surrogate=surrogate, value_loss=value_loss, entropy=entropy, kl=kl, dmu=mu.grad, dvalue=value.grad, dstd=std.grad)
    for name, w in want.items():
        assert _rel(res[name], w.detach()) <= 1e-12, (name, _rel(res[name], w.detach()))
    # what the reduced outputs are scaled by adds up to them, and the sums in `acc` are the means times M
    for name, t in res["_terms"].items():
        assert _rel(t.sum(0), res[name]) <= 1e-12 or float(t.abs().sum(0).max()) == 0.0, name
    assert _rel(res["acc_surrogate"] / 300, res["surrogate"]) <= 1e-12
    assert _rel(res["acc_dstd"] - c["ecoef"] / c["std"], res["dstd"]) <= 1e-12
    assert float(res["amax_mu"]) == float(res["dmu"].abs().max()) and float(res["amax_v"]) == float(res["dvalue"].abs().max())


@pytest.mark.parametrize("regime", list(R.ADAM_REGIMES))
def test_adam_oracle_equals_torch_adam_in_float64(regime, monkeypatch):
    """clip_grad_norm_ + torch.optim.Adam on float64 parameters, given the SAME betas as Python doubles (the float32 values of the
    call), for three steps from the case's non-zero moments.  clip_grad_norm_'s 1e-6 is a double here, where the oracle has the
    kernel's float32 constant: with torch's in its place the formula must be torch's."""
    monkeypatch.setattr(R, "CLIP_EPS", 1.0e-6)
    case = R.make_adam_case(300, seed=3, regime=regime)
    p = torch.nn.Parameter(case["p"].double())
    opt = torch.optim.Adam([p], lr=case["lr"], betas=(case["b1"], case["b2"]), eps=case["eps"], weight_decay=case["wd"])
    first = case["step"]
    opt.state[p] = dict(step=torch.tensor(float(first - 1)), exp_avg=case["m"].double(), exp_avg_sq=case["v"].double())
    cur = case
    for k in range(3):
        grad = cur["g"].double().clone()
        p.grad = grad.clone()
        norm = torch.nn.utils.clip_grad_norm_([p], case["max_norm"]) if case["max_norm"] > 0 else grad.norm()
        opt.step()
        res = R.adam_clip_step(dict(cur, step=first + k))
        st = opt.state[p]
        for name, w in dict(p=p.detach(), g=p.grad, m=st["exp_avg"], v=st["exp_avg_sq"], grad_norm_sq=norm.detach() ** 2).items():
            assert _rel(res[name], w) <= 1e-12, (regime, k, name, _rel(res[name], w))
        cur = dict(cur, p=res["p"], g=torch.randn(300, dtype=F64) * float(grad.norm()) / 17.0, m=res["m"], v=res["v"])


def test_gae_oracle_equals_the_sum_over_future_deltas():
    """GAE written without a recursion: A_t = sum over l >= 0 of (gamma lambda)^l delta_{t + l} as long as no step from t to t + l - 1
    was the last of its episode; returns = A + V."""
    case = R.make_gae_case(9, 40, seed=1)
    res = R.gae(case)
    r, v, lv = case["rewards"].double(), case["values"].double(), case["last_values"].double()
    alive = 1.0 - case["dones"].double()
    T = r.shape[0]
    nxt = torch.cat([v[1:], lv[None]])
    delta = r + alive * case["gamma"] * nxt - v
    adv = torch.zeros_like(r)
    for t in range(T):
        open_ = torch.ones_like(lv)
        for l in range(T - t):
            adv[t] += open_ * (case["gamma"] * case["lam"]) ** l * delta[t + l]
            open_ = open_ * alive[t + l]
    assert _rel(res["advantages"], adv) <= 1e-12 and _rel(res["returns"], adv + v) <= 1e-12
    assert bool(case["dones"][:, 0].all()) and not bool(case["dones"][:, -1].any())
    # a column that is done at every step: its advantage is r - V, whatever follows
    assert torch.equal(res["advantages"][:, 0], ((r - v)[:, 0] + v[:, 0]) - v[:, 0])


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_elu_oracle_equals_autograd_of_elu(alpha):
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(100, 12, generator=gen, dtype=F64)
    z.view(-1)[::9] = 0.0  # elu'(0) is the negative side's: alpha
    z.requires_grad_(True)
    a = torch.nn.functional.elu(z, alpha=alpha)
    da = torch.randn(100, 12, generator=gen, dtype=F64)
    (a * da).sum().backward()
    res = R.elu_backward_bias(dict(da=da, a=a.detach(), alpha=alpha, block_rows=48))
    assert _rel(res["dz"], z.grad) <= 1e-12 and _rel(res["db"], z.grad.sum(0)) <= 1e-12
    assert res["amax_blocks"].tolist() == [float(z.grad[:48].abs().max()), float(z.grad[48:96].abs().max()), float(z.grad[96:].abs().max())]


def test_head_oracle_decodes_the_split_format_exactly():
    case = R.make_head_case(50, 3, 8, seed=2, split=True)
    x = case["x"]
    hi = x.half()
    lo = ((x - hi.float()) * 64.0).half()
    dec = R.decode_split(case["x_words"])
    assert torch.equal(dec, hi.double() + lo.double() / 64.0) and _rel(dec, x.double()) <= 2.0 ** -20
    res = R.head_wgrad(case)
    assert _rel(res["dw"], torch.einsum("mn,mk->nk", case["dy"].double(), dec)) <= 1e-12
    assert _rel(res["_terms"]["dw"].sum(0), res["dw"]) <= 1e-12


def test_lr_rule_is_the_reference_rule_and_sequential_sums_in_float32():
    f = np.float32
    assert R.lr_rule(0.03, 0.01, 1e-5, 1e-2, 1.5, 1e-3)[0] == f(1e-3) / f(1.5)            # kl > 2 d
    assert R.lr_rule(0.004, 0.01, 1e-5, 1e-2, 1.5, 1e-3)[0] == f(1e-3) * f(1.5)           # 0 < kl < d / 2
    assert R.lr_rule(f(0.01) * f(2), 0.01, 1e-5, 1e-2, 1.5, 1e-3)[0] == f(1e-3)           # exactly 2 d: stays
    assert R.lr_rule(f(0.01) * f(0.5), 0.01, 1e-5, 1e-2, 1.5, 1e-3)[0] == f(1e-3)         # exactly d / 2: stays
    assert R.lr_rule(0.0, 0.01, 1e-5, 1e-2, 1.5, 1e-3)[0] == f(1e-3)                      # kl == 0: stays
    assert R.lr_rule(0.03, 0.01, 1e-5, 1e-2, 1.5, 1e-5)[0] == f(1e-5) and R.lr_rule(0.004, 0.01, 1e-5, 1e-2, 1.5, 1e-2)[0] == f(1e-2)
    assert R.lr_rule(0.03, 0.0, 1e-5, 1e-2, 1.5, 1e-3)[0] == f(1e-3) and R.lr_rule(None, 0.01, 1e-5, 1e-2, 1.5, 1e-3)[0] == f(1e-3)
    # `sequential` really adds in float32: 2^24 + 1 + 1 stays 2^24 in row order
    seq = R.sequential({"_terms": {"s": torch.tensor([[2.0 ** 24], [1.0], [1.0]])}})["s"]
    assert seq.dtype == F32 and float(seq) == 2.0 ** 24


# ---- the generator's conditions, on the cases the GPU test runs ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss(M, A, clipped, variant):
    case = R.loss_case(M, A, clipped, variant)
    ref64, cpu32 = R.ppo_loss(case), R.ppo_loss(case, dtype=F32)
    return case, ref64, cpu32


@pytest.mark.parametrize("M,A,clipped,variant", R.LOSS_CASES, ids=[f"{m}x{a}-c{c}-{v}" for m, a, c, v in R.LOSS_CASES])
def test_loss_cases_populate_every_branch_away_from_the_boundaries(M, A, clipped, variant):
    case, ref64, cpu32 = _loss(M, A, clipped, variant)
    again = R.loss_case(M, A, clipped, variant)
    assert all(torch.equal(case[k].view(torch.int32), again[k].view(torch.int32)) for k in ("mu", "actions", "old_sigma", "adv"))  # seeded
    b64, b32 = R.loss_branches(case), R.loss_branches(case, dtype=F32)
    shares = {k: float(v.double().mean()) for k, v in b64.items()}
    print(f"\nPPOREF loss ({M},{A}) clipped={clipped} {variant}: redrawn {case['redrawn']} far {case['far']} shares "
          + " ".join(f"{k}={s:.2f}" for k, s in shares.items()))
    assert all(torch.equal(b64[k], b32[k]) for k in b64), "the float32 baseline leaves the float64 branch on some row"
    assert case["redrawn"] <= 0.02 * M
    if M >= 255:
        for k, s in shares.items():
            assert s >= 0.10, (k, s)
        assert case["far"] >= 2 and int((case["adv"] == 0).sum()) >= 2
        ratio = float(case["std"].max() / case["old_sigma"][~case["old_sigma"].isnan().any(-1)][0].max())
        assert 0.8 < ratio < 1.25
    if variant == "index":
        assert case["idx"].unique().numel() == M and int(case["old_sigma"].isnan().any(-1).sum()) == 2 * M
    if variant == "boundary":
        d = case["value"] - case["old_values"]
        assert int((d == case["clip"]).sum()) >= 10 and int((d == -case["clip"]).sum()) >= 10
    for res in (ref64, cpu32):
        assert all(torch.isfinite(v).all() for k, v in res.items() if k != "_terms")


# ---- the comparator: the float32 form passes on every GPU case, every mutation is rejected on a named array ----------------------------
def _judge(fn, case, res, block_rows=None):
    """-> (report, {array: why} of everything that rejects `res`: comparator failures and exact checks)"""
    ref64, cpu32 = fn(case), fn(case, dtype=F32)
    report = R.compare(res, ref64, [cpu32, R.sequential(cpu32)])
    bad = {n: f"ratio {v[2]:.3g}" for n, v in R.failures(report).items()}
    bad.update(R.exact_problems(res, block_rows))
    return report, bad


def _all_gpu_cases():
    rows = R.elu_block_rows()
    out = [(f"loss-{c}", R.ppo_loss, lambda c=c: _loss(*c)[0]) for c in R.LOSS_CASES]
    out += [(f"gae-{c}", R.gae, lambda c=c: R.make_gae_case(c[0], c[1], seed=c[0] + c[1], small_rewards=c[2])) for c in R.GAE_CASES]
    out += [(f"adam-{c}", R.adam_clip_step, lambda c=c: R.make_adam_case(c[0], seed=c[0], regime=c[1])) for c in R.ADAM_CASES]
    out += [(f"elu-{s}-{al}", R.elu_backward_bias, lambda s=s, al=al: R.make_elu_case(*s, seed=s[0] + s[1], alpha=al, block_rows=rows))
            for s in R.ELU_SHAPES for al in (1.0, 0.5)]
    out += [(f"head-{c}", R.head_wgrad, lambda c=c: R.make_head_case(c[0], c[1], c[2], seed=c[0] + c[1] + c[2], split=c[3])) for c in R.HEAD_CASES]
    out += [(f"sums-{j}", R.partial_sums, lambda j=j, i=i: R.make_sums_case(j[0], j[1], j[2], seed=i)) for i, j in enumerate(R.SUMS_JOBS)]
    return out, rows


def test_unmutated_float32_form_passes_on_every_gpu_case():
    cases, rows = _all_gpu_cases()
    assert rows == 48
    for name, fn, make in cases:
        case = make()
        report, bad = _judge(fn, case, fn(case, dtype=F32), rows)
        assert not bad, (name, bad, R.format_report(report))
        assert R.worst(report)[1] <= 1.0, (name, R.worst(report))  # a baseline against itself: e / (e + 2^-24)


@functools.lru_cache(maxsize=None)
def _mutation_case(entry, mutation):
    if entry == "ppo_loss":  # the index form: value_loss_coef 0.5, entropy_coef 0.01, a block plus one row
        return R.ppo_loss, _loss(257, 12, 1, "index")[0]
    if entry == "gae":
        return R.gae, R.make_gae_case(7, 257, seed=264)
    if entry == "adam_clip_step":
        regime = {"clip_coefficient_without_1e-6": "tiny", "weight_decay_before_clip": "decay"}.get(mutation, "above")
        return R.adam_clip_step, R.make_adam_case(2049, seed=2049, regime=regime)
    if entry == "elu_backward_bias":  # alpha != 1 and exact zeros in a: `a >= 0` shows; a partial last block
        return R.elu_backward_bias, R.make_elu_case(49, 400, seed=449, alpha=0.5, block_rows=R.elu_block_rows())
    if entry == "head_wgrad":
        return R.head_wgrad, R.make_head_case(97, 12, 128, seed=237, split=True)
    return R.partial_sums, R.make_sums_case(97, 144, 129, seed=4)


MUTANTS = [(m, e[0], e[1]) for m, e in R.MUTATIONS.items() if m != "mantissa10"]


@pytest.mark.parametrize("mutation,entry,array", MUTANTS, ids=[m for m, _, _ in MUTANTS])
def test_mutated_float32_form_is_rejected(mutation, entry, array):
    fn, case = _mutation_case(entry, mutation)
    report, bad = _judge(fn, case, fn(case, dtype=F32, mutate=mutation), case.get("block_rows"))
    print(f"\nPPOREF {entry} {mutation}: rejected on {sorted(bad)}, worst {R.worst(report)}")
    assert array in bad, (sorted(bad), R.format_report(report))
    if array not in R.EXACT_ONLY:  # far outside, not marginally
        assert report[array][2] >= 100.0, report[array]


@pytest.mark.parametrize("entry", R.MUTATIONS["mantissa10"])
def test_mantissa_rounding_is_rejected_on_every_array(entry):
    fn, case = _mutation_case(entry, "mantissa10")
    report, bad = _judge(fn, case, fn(case, dtype=F32, mutate="mantissa10"), case.get("block_rows"))
    print(f"\nPPOREF {entry} mantissa10: {R.format_report(report)}")
    assert bad.keys() >= report.keys(), sorted(report.keys() - bad.keys())
