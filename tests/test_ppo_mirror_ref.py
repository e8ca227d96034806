"""tests/ppo_mirror_ref.py without a GPU: its float64 statement of `lt_ppo_loss_mirror` against torch autograd through this package's
`PPO._symmetry_update` (the reference's update as torch ops) in the two modes without augmentation, on the synthetic rollout of
tests/rl_synth.py; its cases shown to stay away from the branch boundaries with every branch class populated; the comparator shown to
reject each of its `MUTATIONS` on a named array (a float32 CPU form stands in for the kernel); and the binding of include/lt_ppo_mirror.h
and include/lt_mlp_rows.h with their host-side refusals."""
import ctypes
import functools
import re
import warnings

import pytest
import torch

from tests import ppo_mirror_ref as MR
from tests import ppo_ref as R
from tests import ppo_sym_ref as S

F64, F32 = torch.float64, torch.float32


# ---- the statement against autograd through _symmetry_update ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mirror_loss", "logging_only"])
def test_statement_equals_autograd_of_the_op_chain_on_the_synthetic_rollout(mode, monkeypatch):
    """One minibatch of the whole synthetic rollout through `_symmetry_update` in float64, the optimizer step held back: the gradients
    that reach the actor's outputs (its M-row forward of the surrogate plus its 2 M-row forward of the symmetry loss), the critic's output
    and the std, and every scalar, against the statement on the same numbers."""
    from locotouch_amd.rl import PPO, ActorCritic
    from locotouch_amd.rl.symmetry import mirror_go1, mirror_tables
    from tests.rl_synth import N_ACT, N_ENVS, N_OBS, N_STEPS, PPO_CFG, synth_rollout
    from tests.symmetry_synth import MIRROR_LOSS_COEFF, TeacherRows, symmetry_cfg

    torch.manual_seed(0)
    env = TeacherRows()
    ac = ActorCritic(N_OBS, N_OBS, N_ACT, init_noise_std=0.8, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32], activation="elu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alg = PPO(ac, device="cpu", symmetry_cfg=symmetry_cfg(mode, mirror_go1, env), **dict(PPO_CFG, num_learning_epochs=1, num_mini_batches=1))
    alg.init_storage(N_ENVS, N_STEPS, [N_OBS], [N_OBS], [N_ACT])
    data = synth_rollout(seed=123)
    for t in range(N_STEPS):
        alg.act(data["obs"][t], data["critic_obs"][t])
        alg.process_env_step(data["rewards"][t], data["dones"][t], {"time_outs": data["time_outs"][t]})
    alg.compute_returns(data["last_critic_obs"])
    with torch.no_grad():  # a behaviour policy and old values a step away, so that the ratio and the value leave their clip ranges on some rows
        for p in ac.actor.parameters():
            p.add_(0.02 * torch.randn_like(p))
        for p in ac.critic.parameters():
            p.add_(0.05 * torch.randn_like(p))
    st = alg.storage
    ac.double()
    for stack in (ac.actor, ac.critic):  # (the minibatch generator hands observation rows over as float32: the stacks widen their input)
        stack.register_forward_pre_hook(lambda mod, inp: (inp[0].double(),))
    for k, v in vars(st).items():
        if torch.is_tensor(v) and v.is_floating_point() and k not in ("observations", "privileged_observations"):
            setattr(st, k, v.double())
    seen = dict(actor=[], critic=[], batch=[], loss=[], kl=[])
    ac.actor.register_forward_hook(lambda mod, inp, out: (out.retain_grad(), seen["actor"].append(out))[1] if out.requires_grad else None)
    ac.critic.register_forward_hook(lambda mod, inp, out: (out.retain_grad(), seen["critic"].append(out))[1] if out.requires_grad else None)
    batches, chain, apply_kl = st.mini_batches, alg._op_chain_loss, alg._apply_kl

    def mini_batches(*a, **k):
        for b in batches(*a, **k):
            seen["batch"].append(b)
            yield b

    monkeypatch.setattr(st, "mini_batches", mini_batches)
    monkeypatch.setattr(alg, "_op_chain_loss", lambda *a, **k: (seen["loss"].append(chain(*a, **k)), seen["loss"][-1])[1])
    monkeypatch.setattr(alg, "_apply_kl", lambda kl, *a, **k: (seen["kl"].append(kl.clone()), apply_kl(kl, *a, **k))[1])
    monkeypatch.setattr(alg, "_optim_step", lambda: None)  # the gradients stay where backward left them
    v_loss, s_loss, ent, _, sym = alg.update()
    assert len(seen["batch"]) == 1 and len(seen["actor"]) == 2 and len(seen["critic"]) == 1 and len(seen["kl"]) == 1
    b, (mu_m, mu_2m), value = seen["batch"][0], seen["actor"], seen["critic"][0]
    M = N_ENVS * N_STEPS
    assert mu_m.shape == (M, N_ACT) and mu_2m.shape == (2 * M, N_ACT) and value.shape == (M, 1)
    coeff = MIRROR_LOSS_COEFF if mode == "mirror_loss" else 0.0
    src, sign = mirror_tables(env).of("action")
    case = dict(mu=mu_2m.detach(), std=ac.std.detach(), value=value.detach().view(-1), actions=b.actions, old_logp=b.log_prob.view(-1), adv=b.advantages.view(-1),
                returns=b.returns.view(-1), old_values=b.values.view(-1), old_mu=b.mu, old_sigma=b.sigma, idx=None, clip=PPO_CFG["clip_param"],
                vcoef=PPO_CFG["value_loss_coef"], ecoef=PPO_CFG["entropy_coef"], clipped=1, std_is_log=0, adv_stats=None, act_src=src.long(),
                act_sign=sign.double(), mirror_coeff=coeff)
    ref = MR.ppo_loss_mirror(case)
    br = R.loss_branches(dict(case, mu=case["mu"][:M]))
    assert all(int(br[k].sum()) > 0 for k in ("inside", "above", "below", "v_inside", "v_outside_l1", "v_outside_l2")), {k: int(v.sum()) for k, v in br.items()}
    close = functools.partial(torch.testing.assert_close, rtol=1e-9, atol=1e-13)
    dmu = torch.zeros_like(mu_2m) if mu_2m.grad is None else mu_2m.grad.clone()  # (logged only: the symmetry loss is detached)
    dmu[:M] += mu_m.grad
    close(ref["dmu"], dmu)
    close(ref["dvalue"], value.grad.view(-1))
    close(ref["dstd"], ac.std.grad)
    loss, surrogate, value_loss = seen["loss"][0]
    for name, got in (("loss", loss.detach() + coeff * sym), ("surrogate", surrogate.detach()), ("value_loss", value_loss.detach()), ("kl", seen["kl"][0]),
                      ("entropy", torch.tensor(ent, dtype=F64)), ("symmetry", torch.tensor(sym, dtype=F64))):
        close(ref[name], torch.as_tensor(got, dtype=F64), msg=lambda s, name=name: f"{name}: {s}")
    close(torch.tensor(v_loss, dtype=F64), ref["value_loss"])
    close(torch.tensor(s_loss, dtype=F64), ref["surrogate"])
    assert float(ref["symmetry"]) > 0.0
    if coeff:  # the mirror term reaches the mirrored rows alone, and they carry nothing else
        close(ref["dmu"][M:], coeff * 2.0 * (case["mu"][M:] - S.mirror(case["mu"][:M], src.long(), sign.double())) / (M * N_ACT))
        close(ref["dmu"][:M], MR.ppo_loss_mirror(dict(case, mirror_coeff=0.0))["dmu"][:M])
    else:
        assert not ref["dmu"][M:].any() and mu_2m.grad is None
    for k in ("dstd", "acc_dstd", "acc_sym", "symmetry", "loss"):
        close(ref["_terms"][k].sum(0), ref[k])


# ---- the cases the GPU test runs -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parent(M, A, clipped, variant, opts, coeff):
    return MR.sym_parent(M, A, clipped, variant, opts, coeff)


def _case(*c):
    return MR.of_sym_case(_parent(*c))


BRANCH_CASES = [c for c in MR.MIRROR_CASES if c[5] == 0.5]  # (the coefficient moves no branch: mu and value are inputs)


@pytest.mark.parametrize("M,A,clipped,variant,opts,coeff", BRANCH_CASES, ids=[f"{m}x{a}-c{c}-{v}-{o}" for m, a, c, v, o, _ in BRANCH_CASES])
def test_cases_stay_away_from_the_branch_boundaries_and_populate_every_class(M, A, clipped, variant, opts, coeff):
    parent = _parent(M, A, clipped, variant, opts, coeff)
    case = _case(M, A, clipped, variant, opts, coeff)
    assert case["mu"].shape == (2 * M, A) and case["value"].shape == (M,) and torch.equal(case["value"], parent["value"][:M])
    bad = S.branch_problems(parent)
    assert not bad, bad
    counts = S.branch_counts(parent)[0]  # the scored rows are the first half's
    if M >= 255:
        classes = ("inside", "above", "below") + (("v_inside", "v_outside_l1", "v_outside_l2") if clipped else ())
        assert all(counts[k] >= 0.03 * M for k in classes), counts
    for res in (MR.ppo_loss_mirror(case), MR.ppo_loss_mirror(case, dtype=F32)):
        assert all(torch.isfinite(v).all() for k, v in res.items() if k != "_terms")
        assert res["dmu"].shape == (2 * M, A) and res["dvalue"].shape == (M,)


# ---- the comparator: the float32 form passes, every mutation is rejected on a named array ----------------------------------------------
def _judge(case, res):
    ref64, cpu32 = MR.ppo_loss_mirror(case), MR.ppo_loss_mirror(case, dtype=F32)
    report = R.compare(res, ref64, [cpu32, R.sequential(cpu32)])
    bad = {n: f"ratio {v[2]:.3g}" for n, v in R.failures(report).items()}
    bad.update(R.exact_problems(res))
    return report, bad


def test_unmutated_float32_form_passes_on_every_gpu_case():
    for c in MR.MIRROR_CASES:
        case = _case(*c)
        report, bad = _judge(case, MR.ppo_loss_mirror(case, dtype=F32))
        assert not bad, (c, bad, R.format_report(report))
        assert R.worst(report)[1] <= 1.0, (c, R.worst(report))


MUTANTS = [(m, e[1]) for m, e in MR.MUTATIONS.items()]


@pytest.mark.parametrize("mutation,array", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_mutated_float32_form_is_rejected(mutation, array):
    case = _case(257, 12, 1, "index", "both", 0.5)  # both options, the index form, value_loss_coef 0.5, a block plus one row, the mirror loss on
    if mutation == "mirror_term_missing_from_amax":  # (at 0.5 the largest gradient sits in the scored rows: a coefficient that moves it)
        case = dict(case, mirror_coeff=MR.AMAX_COEFF)
        res = MR.ppo_loss_mirror(case)
        assert float(res["dmu"][257:].abs().max()) > 2.0 * float(res["dmu"][:257].abs().max())
    report, bad = _judge(case, MR.ppo_loss_mirror(case, dtype=F32, mutate=mutation))
    print(f"\nPPOMIRROR {mutation}: rejected on {sorted(bad)}, worst {R.worst(report)}")
    assert array in bad, (sorted(bad), R.format_report(report))
    if array in report:
        assert report[array][2] >= 100.0, report[array]  # far outside, not marginally


def test_mantissa_rounding_is_rejected_on_every_array():
    case = _case(257, 12, 1, "index", "both", 0.5)
    report, bad = _judge(case, MR.ppo_loss_mirror(case, dtype=F32, mutate="mantissa10"))
    assert bad.keys() >= report.keys(), sorted(report.keys() - bad.keys())


def test_coefficient_zero_leaves_the_mirrored_rows_without_gradient():
    case = _case(257, 12, 1, "index", "both", 0.0)
    for dtype in (F64, F32):
        res = MR.ppo_loss_mirror(case, dtype=dtype)
        assert not res["dmu"][257:].any() and float(res["symmetry"]) > 0.0


# ---- the binding -----------------------------------------------------------------------------------------------------------------------
def _protos(path):
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))
    return set(re.findall(r"\b(lt_\w+)\s*\([^()]*\)\s*;", src))


def test_headers_are_bound_by_one_row_each_and_the_pinned_ones_are_as_they_were():
    from locotouch_amd import _abi, build

    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    for fname, prefix, uses_env in (("lt_ppo_mirror.h", "PPO_MIRROR", False), ("lt_mlp_rows.h", "MLP_ROWS", True)):
        row = [r for r in _abi.HEADERS if r[1] == fname]
        assert len(row) == 1 and row[0][0] == prefix and row[0][2] is uses_env and row[0][3] == () and row[0][4] == ()
        assert fname not in open(_abi.HEADER).read() and fname not in open(_abi.PPO_SYM_HEADER).read()
    assert _abi.CONSTS["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67
    assert set(_abi.PPO_SYM_SIGNATURES) == {"lt_sym_table_pack", "lt_sym_gather_rows", "lt_ppo_loss_sym"}
    assert _protos(_abi.PPO_MIRROR_HEADER) == set(_abi.PPO_MIRROR_SIGNATURES) == {"lt_ppo_loss_mirror"} and _abi.PPO_MIRROR_CONSTS == {}
    rows = {"lt_mlp_forward_pair_rows", "lt_mlp_backward_pair_rows", "lt_mlp_backward_blocks_rows"}
    assert _protos(_abi.MLP_ROWS_HEADER) == set(_abi.MLP_ROWS_SIGNATURES) == rows and _abi.MLP_ROWS_CONSTS == {}
    assert _abi.PPO_MIRROR_SIGNATURES["lt_ppo_loss_mirror"] == _abi.PPO_SYM_SIGNATURES["lt_ppo_loss_sym"]  # the same argument list
    desc_p = ctypes.POINTER(_abi.LtMlpDesc)
    fwd, bwd = _abi.SIGNATURES["lt_mlp_forward_pair"][1], _abi.SIGNATURES["lt_mlp_backward_pair"][1]
    assert fwd[6] is i64 and bwd[12] is i64
    assert _abi.MLP_ROWS_SIGNATURES["lt_mlp_forward_pair_rows"] == (i32, fwd[:6] + [i64, i64] + fwd[7:])  # (m0, m1) in place of m
    assert _abi.MLP_ROWS_SIGNATURES["lt_mlp_backward_pair_rows"] == (i32, bwd[:12] + [i64, i64] + bwd[13:])
    assert _abi.MLP_ROWS_SIGNATURES["lt_mlp_backward_blocks_rows"] == (i32, [desc_p, desc_p, i64, i64, vp, vp])
    assert f32 in _abi.PPO_MIRROR_SIGNATURES["lt_ppo_loss_mirror"][1]
    assert f"hipv4-amdgcn-amd-amdhsa--{build.ARCH}".encode() in open(_abi.LIB_PATH, "rb").read()
    _abi.load()
    assert all(name in _abi._calls for name in rows | {"lt_ppo_loss_mirror"})


def _desc(dims):
    from locotouch_amd import _abi

    d = _abi.LtMlpDesc()
    d.num_layers = len(dims) - 1
    for i, w in enumerate(dims):
        d.dims[i] = w
    d.activation = _abi.CONSTS["LT_ACT_ELU"]
    return d


def test_every_refusal_of_the_new_entries_names_its_field():
    """LT_EINVAL before anything is launched (no GPU is needed to be refused): "<function>: invalid argument: <field> must be ..."."""
    from locotouch_amd import _abi

    lib = _abi.load()
    vp = ctypes.c_void_p
    one, odd, null, bad = vp(16), vp(18), vp(None), _abi.CONSTS["LT_EINVAL"]
    err = lambda: lib.lt_last_error().decode()  # noqa: E731
    swap = lambda a, i, v: a[:i] + [v] + a[i + 1:]  # noqa: E731
    # lt_ppo_loss_mirror: 0 mu 1 std 2 value 3 actions 4 old_logp 5 adv 6 returns 7 old_values 8 old_mu 9 old_sigma 10 idx 11 M 12 A 13 clip 14 vcoef 15 ecoef
    # 16 clipped 17 std_is_log 18 adv_stats 19 act_table 20 mirror_coeff 21 dmu 22 dvalue 23 acc 24 out 25 sym_sum 26 stream
    fn = "lt_ppo_loss_mirror"
    args = [one] * 10 + [null, 64, 12, 0.2, 1.0, 0.01, 1, 1, null, one, 0.5, one, one, one, one, one, null]
    assert lib.lt_ppo_loss_mirror(*swap(args, 12, 17)) == bad and err() == f"{fn}: invalid argument: A must be in [1, 16]"
    assert lib.lt_ppo_loss_mirror(*swap(args, 12, 0)) == bad and err() == f"{fn}: invalid argument: A must be in [1, 16]"
    for m in (0, -3):
        assert lib.lt_ppo_loss_mirror(*swap(args, 11, m)) == bad and err() == f"{fn}: invalid argument: M must be in [1, 2^31)"
    required = {0: "mu", 1: "std", 2: "value", 3: "actions", 4: "old_logp", 5: "adv", 6: "returns", 7: "old_values", 8: "old_mu", 9: "old_sigma",
                19: "act_table", 21: "dmu", 22: "dvalue", 23: "acc"}
    for i, name in required.items():
        for p in (null, odd):
            assert lib.lt_ppo_loss_mirror(*swap(args, i, p)) == bad and err() == f"{fn}: invalid argument: {name} must be non-null and 4-byte aligned", (name, err())
    for i, name in {18: "adv_stats", 24: "out", 25: "sym_sum"}.items():
        assert lib.lt_ppo_loss_mirror(*swap(args, i, odd)) == bad and err() == f"{fn}: invalid argument: {name} must be NULL or 4-byte aligned"
    assert lib.lt_ppo_loss_mirror(*swap(args, 10, vp(20))) == bad and err() == f"{fn}: invalid argument: idx must be NULL or 8-byte aligned"
    assert lib.lt_ppo_loss_mirror(*swap(args, 20, float("inf"))) == bad and err() == f"{fn}: invalid argument: mirror_coeff must be finite"
    assert lib.lt_ppo_loss_mirror(*swap(args, 24, null)) == bad and "out must be non-null where sym_sum is given" in err()

    actor, critic, narrow = _desc([348, 128, 64, 12]), _desc([348, 128, 64, 1]), _desc([348, 128, 62, 12])
    ref = ctypes.byref
    ptrs = (vp * 2)(16, 16)
    nulls = (vp * 2)(16, None)
    # lt_mlp_forward_pair_rows: 0 d0 1 packed0 2 x0 3 d1 4 packed1 5 x1 6 m0 7 m1 8 y0 9 y1 10 acts0 11 acts1 12 acts_split 13 stream
    fn = "lt_mlp_forward_pair_rows"
    f = [ref(actor), one, one, ref(critic), one, one, 34, 17, one, one, ptrs, ptrs, 1, null]
    for i, name in ((6, "m0"), (7, "m1")):
        for m in (0, -1):
            assert lib.lt_mlp_forward_pair_rows(*swap(f, i, m)) == bad and err() == f"{fn}: invalid argument: {name} must be >= 1"
    assert lib.lt_mlp_forward_pair_rows(*swap(f, 0, ref(narrow))) == bad and err() == f"{fn}: invalid argument: network 0: hidden widths must be multiples of 4"
    assert lib.lt_mlp_forward_pair_rows(*swap(f, 3, ref(narrow))) == bad and err() == f"{fn}: invalid argument: network 1: hidden widths must be multiples of 4"
    for i, who, name in ((1, 0, "packed"), (2, 0, "x"), (8, 0, "y"), (4, 1, "packed"), (5, 1, "x"), (9, 1, "y")):
        for p in (null, odd):
            assert lib.lt_mlp_forward_pair_rows(*swap(f, i, p)) == bad and err() == f"{fn}: invalid argument: network {who}: {name} must be non-null and 4-byte aligned"
    assert lib.lt_mlp_forward_pair_rows(*swap(f, 10, None)) == bad and err() == f"{fn}: invalid argument: network 0: acts must be non-null"
    assert lib.lt_mlp_forward_pair_rows(*swap(f, 11, nulls)) == bad and err() == f"{fn}: invalid argument: network 1: acts[l] must be non-null and 4-byte aligned"
    assert lib.lt_mlp_forward_pair_rows(*swap(f, 0, None)) == bad and err().startswith(f"{fn}: invalid argument: network 0: desc must be")
    # lt_mlp_backward_pair_rows: 0 fwd0 1 bpacked0 2 dy0 3 acts0 4 dz0 5 amax0 6 fwd1 7 bpacked1 8 dy1 9 acts1 10 dz1 11 amax1 12 m0 13 m1 14 acts_split
    # 15 in_amax0 16 in_amax1 17 dz_split 18 scales_out 19 sat_count 20 stream
    fn = "lt_mlp_backward_pair_rows"
    g = [ref(actor), one, one, ptrs, ptrs, ptrs, ref(critic), one, one, ptrs, ptrs, ptrs, 34, 17, 1, one, one, 1, one, one, null]
    for i, name in ((12, "m0"), (13, "m1")):
        for m in (0, -1):
            assert lib.lt_mlp_backward_pair_rows(*swap(g, i, m)) == bad and err() == f"{fn}: invalid argument: {name} must be >= 1"
    for i, who, name in ((1, 0, "bpacked"), (2, 0, "dy"), (7, 1, "bpacked"), (8, 1, "dy")):
        for p in (null, odd):
            assert lib.lt_mlp_backward_pair_rows(*swap(g, i, p)) == bad and err() == f"{fn}: invalid argument: network {who}: {name} must be non-null and 4-byte aligned"
    for i, who, name in ((3, 0, "acts"), (4, 0, "dz"), (5, 0, "amax"), (9, 1, "acts"), (10, 1, "dz"), (11, 1, "amax")):
        assert lib.lt_mlp_backward_pair_rows(*swap(g, i, None)) == bad and err() == f"{fn}: invalid argument: network {who}: {name} must be non-null"
        assert lib.lt_mlp_backward_pair_rows(*swap(g, i, nulls)) == bad and err() == f"{fn}: invalid argument: network {who}: {name}[l] must be non-null and 4-byte aligned"
    assert lib.lt_mlp_backward_pair_rows(*swap(g, 15, null)) == bad and err().startswith(f"{fn}: invalid argument: network 0: in_amax must be non-null where dz_split is set")
    assert lib.lt_mlp_backward_pair_rows(*swap(g, 16, odd)) == bad and err() == f"{fn}: invalid argument: network 1: in_amax must be NULL or 4-byte aligned"
    assert lib.lt_mlp_backward_pair_rows(*swap(g, 18, null)) == bad and err().startswith(f"{fn}: invalid argument: scales_out must be")
    assert lib.lt_mlp_backward_pair_rows(*swap(g, 19, odd)) == bad and err() == f"{fn}: invalid argument: sat_count must be NULL or 4-byte aligned"
    assert lib.lt_mlp_backward_pair_rows(*swap(g, 0, ref(narrow))) == bad and err().startswith(f"{fn}: invalid argument: network 0: fwd must be a network with a backward stream")
    # lt_mlp_backward_blocks_rows: the value query
    fn = "lt_mlp_backward_blocks_rows"
    b0, b1 = ctypes.c_int64(-1), ctypes.c_int64(-1)
    q = [ref(actor), ref(critic), 34, 17, ref(b0), ref(b1)]
    for i, name in ((2, "m0"), (3, "m1")):
        assert lib.lt_mlp_backward_blocks_rows(*swap(q, i, 0)) == bad and err() == f"{fn}: invalid argument: {name} must be >= 1"
    assert lib.lt_mlp_backward_blocks_rows(*swap(q, 4, null)) == bad and err() == f"{fn}: invalid argument: blocks0 must be non-null"
    assert lib.lt_mlp_backward_blocks_rows(*swap(q, 1, ref(narrow))) == bad and err().startswith(f"{fn}: invalid argument: network 1: fwd must be")
    assert (b0.value, b1.value) == (-1, -1)


def test_blocks_query_follows_the_row_tile_thresholds():
    """`pick_row_tiles` decides on the 16-row tiles of BOTH networks: one row tile a workgroup up to 511 tiles, two from 512, four from
    1024; with equal rows the query is the equal-row one."""
    from locotouch_amd import _abi

    lib = _abi.load()
    actor, critic = _desc([348, 128, 64, 12]), _desc([348, 128, 64, 1])
    ref = ctypes.byref

    def blocks(m0, m1):
        b0, b1 = ctypes.c_int64(), ctypes.c_int64()
        assert lib.lt_mlp_backward_blocks_rows(ref(actor), ref(critic), m0, m1, ref(b0), ref(b1)) == 0
        return b0.value, b1.value

    tiles = lambda m: (m + 15) // 16  # noqa: E731
    for (m0, m1), rt in (((2, 1), 1), ((34, 17), 1), ((130, 65), 1), ((17, 64), 1), ((5440, 2720), 1), ((5462, 2731), 2), ((10900, 5450), 2), ((10924, 5462), 4)):
        assert tiles(m0) + tiles(m1) in range({1: 1, 2: 512, 4: 1024}[rt], {1: 512, 2: 1024, 4: 1 << 40}[rt]), (m0, m1)
        assert blocks(m0, m1) == ((tiles(m0) + rt - 1) // rt, (tiles(m1) + rt - 1) // rt), (m0, m1)
    assert tiles(5462) + tiles(2731) == 513 and tiles(10924) + tiles(5462) == 1025
    for m in (1, 64, 4096, 24576):
        assert blocks(m, m) == (lib.lt_mlp_backward_blocks(ref(actor), ref(critic), m),) * 2
