"""`symmetry_cfg` WITHOUT data augmentation on the fused PPO path, from the runner down (rl/runner.py, rl/ppo.py `_direct_update`, rl/mlp.py;
include/lt_ppo_mirror.h, include/lt_mlp_rows.h): the modes `mirror_loss` and `logging_only` of tests/symmetry_synth.py.  One optimizer
step of the direct form against the torch op chain in float32 and in float64 from identical parameters and storage; two iterations of
`learn()` with the launches counted and no host read between the steps; and what must not move - the augmented modes and a runner without
`symmetry_cfg` never enter a new entry point, `direct_update=False` keeps the op chain.  64 envs, T = 8, MLPs [128, 64], as
tests/test_hip_ppo_opts_train.py.

One-step figures on the MI355X (`-s` prints them, PPOMIRROR): per parameter e_direct / (e_op_chain + 2^-24) between 0.28 (critic.0.weight) and
1.56 (std) against the bound 4, in both modes; the loss scalars of the direct form and the float32 op chain differ by at most 1e-6
(the value loss, 13.9; the surrogate is 4e-8 at the first step), the learning rates by 1e-8 of themselves."""
import math

import pytest

from tests import ppo_ref as R
from tests.symmetry_synth import MIRROR_LOSS_COEFF, MODES
from tests.test_hip_ppo_opts_train import N, T, _rollout_and_update, count_calls, count_scalar_reads, make_runner
from tests.test_hip_ppo_sym_train import _rollout

pytestmark = pytest.mark.gpu

NEW_ENTRIES = ("lt_ppo_loss_mirror", "lt_mlp_forward_pair_rows", "lt_mlp_backward_pair_rows", "lt_mlp_backward_blocks_rows")
SYM_ENTRIES = ("lt_sym_table_pack", "lt_sym_gather_rows", "lt_ppo_loss_sym")


def _symmetry_cfg(mode):
    from locotouch_amd.rl.symmetry import MIRROR_GO1

    aug, mirror = MODES[mode]
    return dict(use_data_augmentation=aug, use_mirror_loss=mirror, mirror_loss_coeff=MIRROR_LOSS_COEFF, data_augmentation_func=MIRROR_GO1)


@pytest.mark.filterwarnings("ignore:Symmetry not used for learning")
@pytest.mark.parametrize("mode", ["mirror_loss", "logging_only"])
def test_one_direct_step_against_the_op_chain_in_float32_and_float64(mode, monkeypatch):
    """ONE optimizer step from identical parameters on identical storage, three runners: `_direct_update`, the torch op chain
    (`_symmetry_update`) in float32, and the same op chain in float64 (parameters and storage widened after the rollout).  Per parameter
    the direct form's gradient error against float64 is at most FACTOR times the float32 op chain's plus the comparator's floor
    (tests/ppo_ref.py `compare`); the loss scalars agree with the op chain within 2e-4 and the learning rates within 1e-5 of themselves."""
    import torch
    from locotouch_amd.rl import PPO, tuned_gemms

    tuned_gemms.disable()
    ran = []
    real = PPO._direct_update
    monkeypatch.setattr(PPO, "_direct_update", lambda self, *a, **k: (ran.append(self), real(self, *a, **k))[1])
    one = dict(log=False, epochs=1, mini_batches=1, tuned_gemms=False, symmetry_cfg=_symmetry_cfg(mode))
    chain = dict(direct_update=False, fused_loss=False)
    a, b, c = (make_runner(**one, **kw) for kw in (dict(), chain, dict(chain, fused_adam=False, packed_forward=False)))
    seen = count_calls(monkeypatch, NEW_ENTRIES + SYM_ENTRIES)
    outs = []
    for r in (a, b, c):
        _rollout(r)
        if r is c:  # float64 from here: the same rollout, widened (the minibatch generator hands observation rows over as float32 -
            # they ARE float32 values - so the two stacks widen their input themselves)
            st = r.alg.storage
            r.alg.actor_critic.double()
            for stack in (r.alg.actor_critic.actor, r.alg.actor_critic.critic):
                stack.register_forward_pre_hook(lambda mod, inp: (inp[0].double(),))
            for k, v in vars(st).items():
                if torch.is_tensor(v) and v.is_floating_point() and k not in ("observations", "privileged_observations"):
                    setattr(st, k, v.double())
        torch.manual_seed(11)
        outs.append(r.alg.update())
    assert ran == [a.alg], "the direct update must have run for the first runner, and for it alone"
    M = N * T
    assert len(seen["lt_sym_table_pack"]) == 2 and len(seen["lt_sym_gather_rows"]) == 1 and len(seen["lt_ppo_loss_mirror"]) == 1 and not seen["lt_ppo_loss_sym"]
    assert len(seen["lt_mlp_forward_pair_rows"]) == 1 and seen["lt_mlp_forward_pair_rows"][0][6:8] == (2 * M, M)
    if mode == "mirror_loss":
        assert len(seen["lt_mlp_backward_pair_rows"]) == 1 and seen["lt_mlp_backward_pair_rows"][0][12:14] == (2 * M, M)
    else:  # no gradient in the mirrored rows: the chain runs on the first M rows of both networks
        assert not seen["lt_mlp_backward_pair_rows"] and not seen["lt_mlp_backward_blocks_rows"]
    for k in ("observations", "actions", "advantages", "returns", "actions_log_prob"):
        assert torch.equal(getattr(a.alg.storage, k), getattr(b.alg.storage, k)) and torch.equal(getattr(a.alg.storage, k).double(), getattr(c.alg.storage, k).double()), k
    print(f"\nPPOMIRROR one step {mode}: direct {outs[0]} op chain f32 {outs[1]} f64 {outs[2]} lr {a.alg.learning_rate} {b.alg.learning_rate} {c.alg.learning_rate}")
    assert outs[0][3] is None and all(o[4] is not None and math.isfinite(o[4]) and o[4] > 0.0 for o in outs)
    for i in (0, 1, 2, 4):
        x, y = outs[0][i], outs[1][i]
        assert abs(x - y) <= 2e-4 * max(1.0, abs(y)), (i, outs)
    assert abs(a.alg.learning_rate - b.alg.learning_rate) <= 1e-5 * b.alg.learning_rate
    assert abs(a.alg.learning_rate - c.alg.learning_rate) <= 1e-5 * c.alg.learning_rate
    bad = {}
    for (name, pa), pb, pc in zip(a.alg.actor_critic.named_parameters(), b.alg.actor_critic.parameters(), c.alg.actor_critic.parameters()):
        g64 = pc.grad
        scale = float(g64.abs().max())
        e_a, e_b = float((pa.grad.double() - g64).abs().max()) / scale, float((pb.grad.double() - g64).abs().max()) / scale
        print(f"PPOMIRROR   {name}: e_direct {e_a:.3e} e_op_chain {e_b:.3e} ratio {e_a / (e_b + R.EPS):.2f}")
        if not e_a <= R.FACTOR * e_b + R.FACTOR * R.EPS:
            bad[name] = (e_a, e_b)
    assert not bad, bad


def test_learn_gathers_once_per_update_and_reads_the_host_once(tmp_path, monkeypatch):
    import torch
    from locotouch_amd.rl import PPO

    runner = make_runner(log=False, per_mb=True, tmp=str(tmp_path), symmetry_cfg=_symmetry_cfg("mirror_loss"))
    assert runner.alg.symmetry["_env"] is runner.env
    seen = count_calls(monkeypatch, NEW_ENTRIES + SYM_ENTRIES + ("lt_adv_stats", "lt_ppo_loss", "lt_ppo_loss_opts", "lt_ppo_lr_rule", "lt_mlp_forward_pair",
                                                               "lt_mlp_backward_pair"))
    reads, real_update, tolist = [], PPO.update, torch.Tensor.tolist

    def update(self):
        """no `.item()`, no `float(t)` / `bool(t)` / `int(t)` of a tensor and ONE `.tolist()` inside an update"""
        n = [0]

        def refuse(*a, **k):
            raise AssertionError("Tensor.item() inside the update")

        def counted(t, *a, **k):
            n[0] += 1
            return tolist(t, *a, **k)

        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "item", refuse)
            m.setattr(torch.Tensor, "tolist", counted)
            scalars = count_scalar_reads(m)
            out = real_update(self)
        assert scalars == []
        reads.append(n[0])
        return out

    monkeypatch.setattr(PPO, "update", update)
    runner.learn(2)
    assert reads == [1, 1]
    steps = 2 * 2 * 2  # updates x epochs x minibatches
    assert len(seen["lt_sym_table_pack"]) == 2  # the policy rows' table and the actions', once per PPO object: the critic sees no mirrored row
    assert len(seen["lt_sym_gather_rows"]) == 2 and len(seen["lt_adv_stats"]) == 2  # per update: ONE gather, one statistics launch
    assert len(seen["lt_ppo_loss_mirror"]) == steps == len(seen["lt_ppo_lr_rule"])
    assert len(seen["lt_mlp_forward_pair_rows"]) == steps == len(seen["lt_mlp_backward_pair_rows"])
    assert not seen["lt_ppo_loss"] and not seen["lt_ppo_loss_opts"] and not seen["lt_ppo_loss_sym"]
    assert not seen["lt_mlp_forward_pair"] and not seen["lt_mlp_backward_pair"]
    M = N * T // 2
    for args in seen["lt_ppo_loss_mirror"]:
        assert args[11] == M and args[12] == 12 and args[0].shape == (2 * M, 12) and args[2].numel() == M and args[22].numel() == M
        assert args[20] == MIRROR_LOSS_COEFF and args[18] is not None
    for args in seen["lt_sym_gather_rows"]:
        assert args[1] == 0 and args[2] == N * T and args[3] == 348 and args[5] == 2 and args[6] == M and args[8].shape == (2 * 2 * M, 348)
    for args in seen["lt_mlp_forward_pair_rows"]:
        assert args[6:8] == (2 * M, M) and args[2].shape == (2 * M, 348) and args[5].shape == (M, 348)
    for args in seen["lt_mlp_backward_pair_rows"]:
        assert args[12:14] == (2 * M, M)
    assert len(runner.history) == 2
    for rec in runner.history:
        assert all(math.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy", "Loss/learning_rate", "Loss/symmetry"))
        assert rec["Loss/symmetry"] > 0.0
    print(f"\nPPOMIRROR learn: Loss/symmetry {[rec['Loss/symmetry'] for rec in runner.history]} with mirror_loss_coeff {MIRROR_LOSS_COEFF}")


@pytest.mark.parametrize("mode", ["augment", "both", None], ids=["augment", "both", "no_symmetry"])
def test_the_other_modes_never_enter_the_new_entry_points(mode, monkeypatch):
    """As every run before: rollout storage and parameters after one update are bit-equal to those of a twin for which a call of any of
    the new entry points is an error."""
    import torch

    kw = dict(log=False) if mode is None else dict(log=False, symmetry_cfg=_symmetry_cfg(mode))
    a = make_runner(**kw)
    out_a = _rollout_and_update(a)
    count_calls(monkeypatch, NEW_ENTRIES, forbid=True)
    b = make_runner(**kw)
    out_b = _rollout_and_update(b)
    for k in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "actions_log_prob", "returns", "advantages"):
        assert torch.equal(getattr(a.alg.storage, k), getattr(b.alg.storage, k)), k
    for (name, pa), pb in zip(a.alg.actor_critic.named_parameters(), b.alg.actor_critic.parameters()):
        assert torch.equal(pa, pb), name
    assert out_a == out_b and a.alg.learning_rate == b.alg.learning_rate
    assert (out_a[4] is None) == (mode is None)


def test_direct_update_false_keeps_the_op_chain(monkeypatch):
    from locotouch_amd.rl import PPO

    ran = []
    real = PPO._symmetry_update
    monkeypatch.setattr(PPO, "_symmetry_update", lambda self: (ran.append(self), real(self))[1])
    runner = make_runner(log=False, epochs=1, mini_batches=1, symmetry_cfg=_symmetry_cfg("mirror_loss"), direct_update=False)
    count_calls(monkeypatch, NEW_ENTRIES, forbid=True)
    assert not runner.alg._symmetry_direct_ok()
    out = _rollout_and_update(runner)
    assert ran == [runner.alg] and out[4] is not None and math.isfinite(out[4]) and out[4] > 0.0
