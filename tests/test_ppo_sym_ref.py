"""tests/ppo_sym_ref.py without a GPU: its float64 statement of `lt_ppo_loss_sym` against torch autograd through the reference's
formulation of the augmented update (loco_rl ppo.py:216-337: an `ActorCritic`, `mirror_go1`-style augmentation, `.repeat`, MSELoss); its
cases shown to populate every branch class in BOTH halves and to stay away from the branch boundaries; the comparator shown to reject
each of its `MUTATIONS` on a named array (a float32 CPU form stands in for the kernel); the gather's statement; and the binding of
include/lt_ppo_sym.h with its host-side refusals."""
import ctypes
import functools
import re

import pytest
import torch

from tests import ppo_opts_ref as O
from tests import ppo_ref as R
from tests import ppo_sym_ref as S

F64, F32 = torch.float64, torch.float32


# ---- the statement against autograd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coeff", [0.0, 0.5], ids=["logged_only", "mirror_loss"])
@pytest.mark.parametrize("log,normalise", [(False, False), (True, True)], ids=["scalar_whole", "log_per_minibatch"])
@pytest.mark.parametrize("clipped", [1, 0])
def test_loss_oracle_equals_autograd_through_the_reference_formulation(clipped, log, normalise, coeff):
    from torch.distributions import Normal

    from locotouch_amd.rl import ActorCritic

    M, A = 300, 12
    case = S.make_sym_case(M, A, seed=7, clipped=clipped, std_is_log=log, normalise=False, mirror_coeff=coeff, rows=900, vcoef=0.5)
    b = {k: v.double() for k, v in R._gathered(case).items()}
    if normalise:
        st = O.adv_stats(dict(adv=case["adv"], idx=case["idx"], M=M, nmb=1))
        case["adv_stats"] = torch.stack([st["mean"][0], st["inv_std"][0]])
    ref = S.ppo_loss_sym(case)
    src, sign = case["act_src"], case["act_sign"].double()

    def augment(obs=None, actions=None):  # the data_augmentation_func contract on the action table
        return obs, None if actions is None else torch.cat((actions, actions[:, src] * sign), dim=0)

    ac = ActorCritic(4, 4, A, actor_hidden_dims=(8,), critic_hidden_dims=(8,), noise_std_type="log" if log else "scalar").double()
    std_p = ac.log_std if log else ac.std
    with torch.no_grad():
        std_p.copy_(case["std"].double())
    mu, value = case["mu"].double().requires_grad_(True), case["value"].double().requires_grad_(True)
    ac.distribution = Normal(mu, ac._std_like(mu))  # what ac.act(obs_batch) leaves behind for the 2 B augmented rows
    clip, vcoef, ecoef = case["clip"], case["vcoef"], case["ecoef"]
    adv = b["adv"][:, None]
    if normalise:
        with torch.no_grad():
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    _, actions = augment(actions=b["actions"])
    num_aug = actions.shape[0] // M
    old_logp, target_values = b["old_logp"][:, None].repeat(num_aug, 1), b["old_values"][:, None].repeat(num_aug, 1)
    adv, returns = adv.repeat(num_aug, 1), b["returns"][:, None].repeat(num_aug, 1)
    log_prob = ac.get_actions_log_prob(actions)
    value_b = value[:, None]
    mu_b, sigma_b, entropy_b = ac.action_mean[:M], ac.action_std[:M], ac.entropy[:M]
    kl = torch.sum(torch.log(sigma_b / b["old_sigma"] + R.KL_EPS) + (b["old_sigma"] ** 2 + (b["old_mu"] - mu_b) ** 2) / (2.0 * sigma_b ** 2) - 0.5, -1).mean()
    ratio = torch.exp(log_prob - torch.squeeze(old_logp))
    surrogate = torch.max(-torch.squeeze(adv) * ratio, -torch.squeeze(adv) * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    if clipped:
        vc = target_values + (value_b - target_values).clamp(-clip, clip)
        value_loss = torch.max((value_b - returns).pow(2), (vc - returns).pow(2)).mean()
    else:
        value_loss = (returns - value_b).pow(2).mean()
    loss = surrogate + vcoef * value_loss - ecoef * entropy_b.mean()
    mean_actions = mu  # act_inference on the same rows: the same means
    _, symm = augment(actions=mean_actions[:M])
    symmetry = torch.nn.MSELoss()(mean_actions[M:], symm.detach()[M:])
    if coeff:
        loss = loss + coeff * symmetry
    loss.backward()
    close = functools.partial(torch.testing.assert_close, rtol=1e-9, atol=1e-13)
    for name, got in (("loss", loss), ("surrogate", surrogate), ("value_loss", value_loss), ("entropy", entropy_b.mean()), ("kl", kl), ("symmetry", symmetry)):
        close(ref[name], got.detach(), msg=lambda s, name=name: f"{name}: {s}")
    close(ref["dmu"], mu.grad)
    close(ref["dvalue"], value.grad)
    close(ref["dstd"], std_p.grad)
    assert float(ref["dmu"][M:].abs().max()) > 0.0 and float(ref["symmetry"]) > 0.0
    if coeff:  # the mirror term reaches the mirrored half alone: without it the first half's gradient is the same
        plain = S.ppo_loss_sym(dict(case, mirror_coeff=0.0))
        close(plain["dmu"][:M], ref["dmu"][:M])
        close(ref["dmu"][M:] - plain["dmu"][M:], coeff * 2.0 * (mu[M:] - symm[M:]).detach() / (M * A))
    for k in ("dstd", "acc_dstd", "acc_sym", "symmetry", "loss"):
        close(ref["_terms"][k].sum(0), ref[k])
    close(ref["acc_sym"] / (M * A), ref["symmetry"])


# ---- the cases the GPU test runs -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(M, A, clipped, variant, opts, coeff):
    return S.sym_case(M, A, clipped, variant, opts, coeff)


BRANCH_CASES = [c for c in S.SYM_CASES if c[5] == 0.5]  # (the coefficient moves no branch: mu and value are inputs)


@pytest.mark.parametrize("M,A,clipped,variant,opts,coeff", BRANCH_CASES, ids=[f"{m}x{a}-c{c}-{v}-{o}" for m, a, c, v, o, _ in BRANCH_CASES])
def test_cases_populate_every_branch_class_in_both_halves_away_from_the_boundaries(M, A, clipped, variant, opts, coeff):
    case = _case(M, A, clipped, variant, opts, coeff)
    assert case["mu"].shape == (2 * M, A) and case["value"].shape == (2 * M,)
    src, sign = case["act_src"], case["act_sign"]
    assert sorted(src.tolist()) == list(range(A)) and set(sign.tolist()) <= {1.0, -1.0}
    bad = S.branch_problems(case)
    assert not bad, bad
    counts = S.branch_counts(case)
    if M >= 255:
        for h in (0, 1):
            classes = ("inside", "above", "below") + (("v_inside", "v_outside_l1", "v_outside_l2") if clipped else ())
            assert all(counts[h][k] >= 0.03 * M for k in classes), (h, counts[h])
    ref64, cpu32 = S.ppo_loss_sym(case), S.ppo_loss_sym(case, dtype=F32)
    for res in (ref64, cpu32):
        assert all(torch.isfinite(v).all() for k, v in res.items() if k != "_terms")


# ---- the comparator: the float32 form passes, every mutation is rejected on a named array ----------------------------------------------
def _judge(case, res):
    ref64, cpu32 = S.ppo_loss_sym(case), S.ppo_loss_sym(case, dtype=F32)
    report = R.compare(res, ref64, [cpu32, R.sequential(cpu32)])
    bad = {n: f"ratio {v[2]:.3g}" for n, v in R.failures(report).items()}
    bad.update(R.exact_problems(res))
    return report, bad


def test_unmutated_float32_form_passes_on_every_gpu_case():
    for c in S.SYM_CASES:
        case = _case(*c)
        report, bad = _judge(case, S.ppo_loss_sym(case, dtype=F32))
        assert not bad, (c, bad, R.format_report(report))
        assert R.worst(report)[1] <= 1.0, (c, R.worst(report))


MUTANTS = [(m, e[1]) for m, e in S.MUTATIONS.items()]


@pytest.mark.parametrize("mutation,array", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_mutated_float32_form_is_rejected(mutation, array):
    case = _case(257, 12, 1, "index", "both", 0.5)  # both options, the index form, value_loss_coef 0.5, a block plus one row, the mirror loss on
    report, bad = _judge(case, S.ppo_loss_sym(case, dtype=F32, mutate=mutation))
    print(f"\nPPOSYM {mutation}: rejected on {sorted(bad)}, worst {R.worst(report)}")
    assert array in bad, (sorted(bad), R.format_report(report))
    if array in report:
        assert report[array][2] >= 100.0, report[array]  # far outside, not marginally


def test_mantissa_rounding_is_rejected_on_every_array():
    case = _case(257, 12, 1, "index", "both", 0.5)
    report, bad = _judge(case, S.ppo_loss_sym(case, dtype=F32, mutate="mantissa10"))
    assert bad.keys() >= report.keys(), sorted(report.keys() - bad.keys())


# ---- the gather's statement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
def test_gather_statement(bf16):
    case = S.make_gather_case(13, 5, 3, bf16, seed=2)
    out = S.sym_gather(case)
    assert out.shape == (3, 2, 5, 13) and out.dtype == F32 and not torch.isnan(out).any()
    rows = case["rows"].float()
    for b in range(3):
        for j in range(5):
            r = rows[case["idx"][b * 5 + j]]
            assert torch.equal(out[b, 0, j], r)
            for c in range(13):
                assert float(out[b, 1, j, c]) == float(case["sign"][c]) * float(r[case["src"][c]])
    assert len(S.GATHER_CASES) == 4 * 4 * 2 * 2


# ---- the binding -----------------------------------------------------------------------------------------------------------------------
def test_header_is_bound_by_one_row_and_refuses_on_the_host():
    from locotouch_amd import _abi, build

    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    row = [r for r in _abi.HEADERS if r[1] == "lt_ppo_sym.h"]
    assert len(row) == 1 and row[0][0] == "PPO_SYM" and not row[0][2] and row[0][3] == () and row[0][4] == ()
    assert "lt_ppo_sym.h" not in open(_abi.HEADER).read() and _abi.CONSTS["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.PPO_SYM_HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_\w+)\s*\([^()]*\)\s*;", src))
    sig = _abi.PPO_SYM_SIGNATURES
    assert protos == set(sig) == {"lt_sym_table_pack", "lt_sym_gather_rows", "lt_ppo_loss_sym"} and _abi.PPO_SYM_CONSTS == {"LT_SYM_MAX_D": 1024}
    assert sig["lt_sym_table_pack"] == (i32, [vp, vp, i32, vp, vp])
    assert sig["lt_sym_gather_rows"] == (i32, [vp, i32, i64, i32, vp, i32, i64, vp, vp, vp])
    opts = _abi.PPO_OPTS_SIGNATURES["lt_ppo_loss_opts"][1]
    assert sig["lt_ppo_loss_sym"] == (i32, opts[:19] + [vp, f32] + opts[19:23] + [vp] + opts[23:])  # + act_table, mirror_coeff ... + sym_sum
    assert f"hipv4-amdgcn-amd-amdhsa--{build.ARCH}".encode() in open(_abi.LIB_PATH, "rb").read()
    lib = _abi.load()
    assert all(name in _abi._calls for name in sig)
    one, odd, null, bad = vp(16), vp(18), vp(None), _abi.CONSTS["LT_EINVAL"]
    err = lambda: lib.lt_last_error().decode()  # noqa: E731

    def pack(src, sign, D=None, table=one):
        s, g = torch.tensor(src, dtype=torch.int32), torch.tensor(sign, dtype=torch.float32)
        return lib.lt_sym_table_pack(vp(s.data_ptr()), vp(g.data_ptr()), len(src) if D is None else D, table, null)

    assert pack([0, 0, 1], [1.0] * 3) == bad and err() == "lt_sym_table_pack: invalid argument: src must be a permutation of 0 .. D - 1"
    assert pack([0, 3, 1], [1.0] * 3) == bad and pack([0, -1, 1], [1.0] * 3) == bad
    assert pack([1, 0, 2], [1.0, 0.5, -1.0]) == bad and err() == "lt_sym_table_pack: invalid argument: sign must be +1 or -1 in every column"
    assert pack([1, 0, 2], [1.0, 0.0, -1.0]) == bad and pack([1, 0, 2], [1.0, float("nan"), -1.0]) == bad
    assert pack([0], [1.0], D=0) == bad and err() == "lt_sym_table_pack: invalid argument: D must be in [1, 1024]"
    assert pack(list(range(1025)), [1.0] * 1025) == bad and err() == "lt_sym_table_pack: invalid argument: D must be in [1, 1024]"
    assert pack([1, 0], [1.0, -1.0], table=odd) == bad and err() == "lt_sym_table_pack: invalid argument: table must be non-null and 4-byte aligned"
    assert lib.lt_sym_table_pack(null, one, 2, one, null) == bad and err() == "lt_sym_table_pack: invalid argument: src_host must be non-null"
    g = [one, 0, 100, 270, one, 4, 64, one, one, null]
    swap = lambda a, i, v: a[:i] + [v] + a[i + 1:]  # noqa: E731
    assert lib.lt_sym_gather_rows(*swap(g, 3, 0)) == bad and err() == "lt_sym_gather_rows: invalid argument: D must be in [1, 1024]"
    assert lib.lt_sym_gather_rows(*swap(g, 3, 1025)) == bad and err() == "lt_sym_gather_rows: invalid argument: D must be in [1, 1024]"
    assert lib.lt_sym_gather_rows(*swap(g, 0, odd)) == bad and err() == "lt_sym_gather_rows: invalid argument: rows must be non-null and 4-byte aligned"
    assert lib.lt_sym_gather_rows(*swap(swap(g, 0, vp(17)), 1, 1)) == bad and err() == "lt_sym_gather_rows: invalid argument: rows must be non-null and 2-byte aligned"
    assert lib.lt_sym_gather_rows(*swap(g, 4, vp(20))) == bad and err() == "lt_sym_gather_rows: invalid argument: idx must be non-null and 8-byte aligned"
    assert lib.lt_sym_gather_rows(*swap(g, 7, null)) == bad and err() == "lt_sym_gather_rows: invalid argument: table must be non-null and 4-byte aligned"
    assert lib.lt_sym_gather_rows(*swap(g, 5, 0)) == bad and lib.lt_sym_gather_rows(*swap(g, 6, 0)) == bad and lib.lt_sym_gather_rows(*swap(g, 2, 0)) == bad
    args = [one] * 10 + [null, 64, 12, 0.2, 1.0, 0.01, 1, 1, null, one, 0.5, one, one, one, one, one, null]
    assert lib.lt_ppo_loss_sym(*swap(args, 12, 17)) == bad and err() == "lt_ppo_loss_sym: invalid argument: A must be in [1, 16]"
    assert lib.lt_ppo_loss_sym(*swap(args, 11, 0)) == bad and err() == "lt_ppo_loss_sym: invalid argument: M must be in [1, 2^31)"
    assert lib.lt_ppo_loss_sym(*swap(args, 19, null)) == bad and err() == "lt_ppo_loss_sym: invalid argument: act_table must be non-null and 4-byte aligned"
    assert lib.lt_ppo_loss_sym(*swap(args, 5, odd)) == bad and err() == "lt_ppo_loss_sym: invalid argument: adv must be non-null and 4-byte aligned"
    assert lib.lt_ppo_loss_sym(*swap(args, 25, odd)) == bad and err() == "lt_ppo_loss_sym: invalid argument: sym_sum must be NULL or 4-byte aligned"
    assert lib.lt_ppo_loss_sym(*swap(args, 20, float("inf"))) == bad and err() == "lt_ppo_loss_sym: invalid argument: mirror_coeff must be finite"
    assert lib.lt_ppo_loss_sym(*swap(args, 24, null)) == bad and "out must be non-null where sym_sum is given" in err()
