"""tests/ppo_opts_ref.py without a GPU: its three float64 statements against torch autograd through this repository's
`ActorCritic(noise_std_type="log")` and the op chain of `PPO._eager_update`; its cases shown to stay away from PPO's branch boundaries
once the options are on; the comparator shown to reject each of its `MUTATIONS` on a named array (a float32 CPU form stands in for the
kernel); and the binding of include/lt_ppo_opts.h."""
import ctypes
import functools
import re

import pytest
import torch

from tests import ppo_opts_ref as O
from tests import ppo_ref as R

F64, F32 = torch.float64, torch.float32


# ---- the statements against autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [False, True], ids=["whole", "per_minibatch"])
@pytest.mark.parametrize("clipped", [1, 0])
def test_log_std_loss_oracle_equals_autograd_through_the_actor_critic(clipped, normalise):
    """The op chain of `PPO._eager_update` in float64 on an `ActorCritic(noise_std_type="log")` whose distribution is built by the
    module's own `_std_like`: loss scalars, dmu, dvalue and the gradient autograd leaves in `log_std.grad`.  With per-minibatch
    normalisation the chain normalises as ppo.py:223-225 does and the oracle takes the two floats of `adv_stats` of the same rows."""
    from torch.distributions import Normal

    from locotouch_amd.rl import ActorCritic

    M, A = 300, 12
    case = O.make_opts_case(M, A, seed=7, clipped=clipped, std_is_log=True, normalise=False, rows=900, vcoef=0.5)
    b = {k: v.double() for k, v in R._gathered(case).items()}
    if normalise:
        st = O.adv_stats(dict(adv=case["adv"], idx=case["idx"], M=M, nmb=1))
        case["adv_stats"] = torch.stack([st["mean"][0], st["inv_std"][0]])  # float64: the chain below normalises in float64 too
    ref = O.ppo_loss_opts(case)

    ac = ActorCritic(4, 4, A, actor_hidden_dims=(8,), critic_hidden_dims=(8,), noise_std_type="log").double()
    with torch.no_grad():
        ac.log_std.copy_(case["std"].double())
    mu, value = case["mu"].double().requires_grad_(True), case["value"].double().requires_grad_(True)
    ac.distribution = Normal(mu, ac._std_like(mu))
    clip, vcoef, ecoef = case["clip"], case["vcoef"], case["ecoef"]
    adv = b["adv"]
    if normalise:
        with torch.no_grad():
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    log_prob = ac.get_actions_log_prob(b["actions"])
    sigma, entropy = ac.action_std, ac.entropy
    kl = torch.sum(torch.log(sigma / b["old_sigma"] + R.KL_EPS) + (b["old_sigma"] ** 2 + (b["old_mu"] - mu) ** 2) / (2.0 * sigma ** 2) - 0.5, -1).mean()
    ratio = torch.exp(log_prob - b["old_logp"])
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    if clipped:
        vc = b["old_values"] + (value - b["old_values"]).clamp(-clip, clip)
        value_loss = torch.max((value - b["returns"]).pow(2), (vc - b["returns"]).pow(2)).mean()
    else:
        value_loss = (b["returns"] - value).pow(2).mean()
    loss = surrogate + vcoef * value_loss - ecoef * entropy.mean()
    loss.backward()
    close = functools.partial(torch.testing.assert_close, rtol=1e-9, atol=1e-13)
    for name, got in (("loss", loss), ("surrogate", surrogate), ("value_loss", value_loss), ("entropy", entropy.mean()), ("kl", kl)):
        close(ref[name], got.detach(), msg=lambda s, name=name: f"{name}: {s}")
    close(ref["dmu"], mu.grad)
    close(ref["dvalue"], value.grad)
    close(ref["dstd"], ac.log_std.grad)
    assert float(ac.log_std.grad.abs().max()) > 10.0 * ecoef / M  # (not the entropy's share alone)
    # the row sums and the summands the comparator scales by are those of the same numbers
    close(ref["_terms"]["dstd"].sum(0), ref["dstd"])
    close(ref["_terms"]["acc_dstd"].sum(0), ref["acc_dstd"])
    close(ref["acc_dstd"] - ecoef, ref["dstd"])


def test_scalar_std_with_both_options_off_is_the_loss_oracle_itself():
    case = O.make_opts_case(257, 12, seed=3, clipped=1, std_is_log=False, normalise=False, rows=771)
    a, b = O.ppo_loss_opts(case), R.ppo_loss(case)
    assert all(torch.equal(a[k], b[k]) for k in b if k != "_terms") and all(torch.equal(a["_terms"][k], b["_terms"][k]) for k in b["_terms"])


def test_adv_stats_oracle_is_torch_mean_and_std_of_the_minibatch_rows():
    case = O.make_adv_case(257, 4, seed=5, storage=2000)
    ref = O.adv_stats(case)
    adv = case["adv"].double()
    for b in range(4):
        rows = adv[case["idx"][b * 257:(b + 1) * 257]]
        assert float(ref["mean"][b]) == pytest.approx(float(rows.mean()), rel=1e-12)
        assert float(ref["inv_std"][b]) == pytest.approx(1.0 / (float(rows.std()) + 1e-8), rel=1e-12)
        normalised = (rows - ref["mean"][b]) * ref["inv_std"][b]
        torch.testing.assert_close(normalised, (rows - rows.mean()) / (rows.std() + 1e-8), rtol=1e-12, atol=1e-14)
    assert not torch.isin(case["unread"], case["idx"]).any() and case["idx"].unique().numel() == 4 * 257
    plain = O.make_adv_case(255, 4, seed=6)
    ref = O.adv_stats(plain)
    torch.testing.assert_close(ref["mean"], plain["adv"].double().view(4, 255).mean(1))


def test_std_from_log_oracle_covers_the_stated_range():
    case = O.make_log_std_case(16, seed=1)
    assert float(case["log_std"].min()) == -5.0 and float(case["log_std"].max()) == 2.0
    torch.testing.assert_close(O.std_from_log(case)["std"], case["log_std"].double().exp())


# ---- the cases the GPU test runs: no row near a branch boundary once the options are on ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _opts(M, A, clipped, variant, opts):
    return O.opts_case(M, A, clipped, variant, opts)


@pytest.mark.parametrize("M,A,clipped,variant,opts", O.OPTS_CASES, ids=[f"{m}x{a}-c{c}-{v}-{o}" for m, a, c, v, o in O.OPTS_CASES])
def test_options_cases_stay_away_from_the_branch_boundaries(M, A, clipped, variant, opts):
    """A normalised advantage changes sign on part of the rows (which surrogate branch is the larger one changes with it), and sigma =
    exp(f32(log sigma)) is not the generator's sigma bit for bit: the margin the generator established is checked again, in float64."""
    case = _opts(M, A, clipped, variant, opts)
    bad = O.margin_problems(case)
    assert not bad, bad
    log, norm = O.OPTS[opts]
    assert case["std_is_log"] == log and (case["adv_stats"] is not None) == bool(norm)
    if norm and M >= 255:
        raw = R._gathered(case)["adv"]
        seen = O.plain_case(case)["adv"] if case["idx"] is None else O.plain_case(case)["adv"][case["idx"]]
        flipped = int(((raw.double() > 0) & (seen < 0)).sum())
        print(f"\nPPOOPTS ({M},{A}) {variant} {opts}: {flipped} of {M} advantages change sign under the normalisation")
        assert flipped >= 0.05 * M and int((seen == 0).sum()) == 0
    if log:
        sigma = case["std"].double().exp()
        assert 0.35 < float(sigma.min()) and float(sigma.max()) < 0.85  # the generator's sigma range, through the log
    ref64, cpu32 = O.ppo_loss_opts(case), O.ppo_loss_opts(case, dtype=F32)
    for res in (ref64, cpu32):
        assert all(torch.isfinite(v).all() for k, v in res.items() if k != "_terms")


# ---- the comparator: the float32 form passes, every mutation is rejected on a named array ----------------------------------------------
def _judge(fn, case, res):
    ref64, cpu32 = fn(case), fn(case, dtype=F32)
    report = R.compare(res, ref64, [cpu32, R.sequential(cpu32)])
    bad = {n: f"ratio {v[2]:.3g}" for n, v in R.failures(report).items()}
    bad.update(R.exact_problems(res))
    return report, bad


def _all_gpu_cases():
    out = [(f"loss-{c}", O.ppo_loss_opts, lambda c=c: _opts(*c)) for c in O.OPTS_CASES]
    out += [(f"adv-{c}", O.adv_stats, lambda c=c: O.adv_case(*c)) for c in O.ADV_CASES]
    out += [(f"std-{a}", O.std_from_log, lambda a=a: O.make_log_std_case(a, seed=a)) for a in (1, 12, 16)]
    return out


def test_unmutated_float32_form_passes_on_every_gpu_case():
    for name, fn, make in _all_gpu_cases():
        case = make()
        report, bad = _judge(fn, case, fn(case, dtype=F32))
        assert not bad, (name, bad, R.format_report(report))
        assert R.worst(report)[1] <= 1.0, (name, R.worst(report))


@functools.lru_cache(maxsize=None)
def _mutation_case(entry, mutation):
    if entry == "ppo_loss_opts":  # both options, the index form, value_loss_coef 0.5, a block plus one row
        return O.ppo_loss_opts, _opts(257, 12, 1, "index", "both")
    if mutation == "without_1e-8":  # a std of 1e-5: the 1e-8 is a thousandth of it
        return O.adv_stats, O.make_adv_case(257, 4, seed=9, kind="small")
    if mutation == "one_pass_variance":
        return O.adv_stats, O.adv_case(257, 4, "offset", None)
    return O.adv_stats, O.adv_case(257, 4, "plain", 3 * 4 * 257 + 5)


MUTANTS = [(m, e[0], e[1]) for m, e in O.MUTATIONS.items()]


@pytest.mark.parametrize("mutation,entry,array", MUTANTS, ids=[m for m, _, _ in MUTANTS])
def test_mutated_float32_form_is_rejected(mutation, entry, array):
    fn, case = _mutation_case(entry, mutation)
    report, bad = _judge(fn, case, fn(case, dtype=F32, mutate=mutation))
    print(f"\nPPOOPTS {entry} {mutation}: rejected on {sorted(bad)}, worst {R.worst(report)}")
    assert array in bad, (sorted(bad), R.format_report(report))
    assert report[array][2] >= 100.0, report[array]  # far outside, not marginally


@pytest.mark.parametrize("entry", ["ppo_loss_opts", "adv_stats"])
def test_mantissa_rounding_is_rejected_on_every_array(entry):
    fn, case = _mutation_case(entry, "mantissa10")
    report, bad = _judge(fn, case, fn(case, dtype=F32, mutate="mantissa10"))
    assert bad.keys() >= report.keys(), sorted(report.keys() - bad.keys())


# ---- the binding -----------------------------------------------------------------------------------------------------------------------
def test_header_is_part_of_the_abi_and_the_library_exports_its_entries():
    """`_abi` lists the three entry points with the header's signatures (derived, not written by hand), lt_env.h includes the header at
    ABI 21, and the library as built for gfx950 exports them and refuses bad arguments on the host with the stated texts."""
    from locotouch_amd import _abi, build

    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _abi.CONSTS["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67
    assert re.search(r'^#include "lt_ppo_opts.h"', open(_abi.HEADER).read(), flags=re.M)
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.PPO_OPTS_HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_\w+)\s*\([^()]*\)\s*;", src))
    S = _abi.PPO_OPTS_SIGNATURES
    assert protos == set(S) == {"lt_std_from_log", "lt_ppo_loss_opts", "lt_adv_stats"}
    assert S["lt_std_from_log"] == (i32, [vp, i32, vp, vp])
    assert S["lt_adv_stats"] == (i32, [vp, vp, i64, i32, vp, vp])
    loss = _abi.SIGNATURES["lt_ppo_loss"][1]
    assert S["lt_ppo_loss_opts"] == (i32, loss[:17] + [i32, vp] + loss[17:]) and loss[13:17] == [f32, f32, f32, i32]
    assert build.ARCH == "gfx950" and f"hipv4-amdgcn-amd-amdhsa--{build.ARCH}".encode() in open(_abi.LIB_PATH, "rb").read()
    lib = _abi.load()
    for name, (restype, argtypes) in S.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
    one, odd, null, bad = vp(16), vp(18), vp(None), _abi.CONSTS["LT_EINVAL"]
    err = lambda: lib.lt_last_error().decode()  # noqa: E731
    assert lib.lt_adv_stats(one, null, 1, 1, one, null) == bad and err().startswith("lt_adv_stats: invalid argument: M must be >= 2")
    assert lib.lt_adv_stats(one, null, 2, 0, one, null) == bad and err() == "lt_adv_stats: invalid argument: nmb must be >= 1"
    assert lib.lt_adv_stats(odd, null, 2, 1, one, null) == bad and err() == "lt_adv_stats: invalid argument: adv must be non-null and 4-byte aligned"
    assert lib.lt_adv_stats(one, vp(20), 2, 1, one, null) == bad and err() == "lt_adv_stats: invalid argument: idx must be NULL or 8-byte aligned"
    assert lib.lt_std_from_log(one, 17, one, null) == bad and err() == "lt_std_from_log: invalid argument: A must be in [1, 16]"
    assert lib.lt_std_from_log(one, 0, one, null) == bad and lib.lt_std_from_log(null, 12, one, null) == bad
    args = [one] * 10 + [null, 64, 12, 0.2, 1.0, 0.01, 1, 1, null, one, one, one, null, null]
    swap = lambda i, v: args[:i] + [v] + args[i + 1:]  # noqa: E731
    assert lib.lt_ppo_loss_opts(*swap(12, 17)) == bad and err() == "lt_ppo_loss_opts: invalid argument: A must be in [1, 16]"
    assert lib.lt_ppo_loss_opts(*swap(11, 0)) == bad and err() == "lt_ppo_loss_opts: invalid argument: M must be >= 1"
    assert lib.lt_ppo_loss_opts(*swap(18, odd)) == bad and err() == "lt_ppo_loss_opts: invalid argument: adv_stats must be NULL or 4-byte aligned"
    assert lib.lt_ppo_loss_opts(*swap(1, odd)) == bad and err() == "lt_ppo_loss_opts: invalid argument: std must be non-null and 4-byte aligned"
    assert lib.lt_ppo_loss_opts(*swap(19, null)) == bad and err() == "lt_ppo_loss_opts: invalid argument: dmu must be non-null and 4-byte aligned"
