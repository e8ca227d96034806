"""`symmetry_cfg` on the fused PPO path, from the runner down (rl/runner.py, rl/ppo.py `_direct_update`, rl/symmetry.py;
include/lt_ppo_sym.h): one optimizer step of the direct form against the torch op chain in float32 and in float64 from identical
parameters and storage; two iterations of `learn()` with the launches counted and no host read between the steps; and a runner
without `symmetry_cfg`, which never enters a new entry point.  64 envs, T = 8, MLPs [128, 64], as tests/test_hip_ppo_opts_train.py.

One-step figures on the MI355X (`-s` prints them, PPOSYM): per parameter e_direct / (e_op_chain + 2^-24) between 0.07 (critic.0.weight) and
1.48 (std) against the bound 4, with and without the mirror loss; the loss scalars of the direct form and the float32 op chain differ by
at most 4e-7 of themselves, the learning rates by 1e-8."""
import math

import pytest

from tests import ppo_ref as R
from tests.test_hip_ppo_opts_train import N, T, count_calls, count_scalar_reads, make_runner

pytestmark = pytest.mark.gpu

NEW_ENTRIES = ("lt_sym_table_pack", "lt_sym_gather_rows", "lt_ppo_loss_sym")


def _symmetry_cfg(coeff):
    from locotouch_amd.rl.symmetry import MIRROR_GO1

    return dict(use_data_augmentation=True, use_mirror_loss=coeff > 0.0, mirror_loss_coeff=coeff, data_augmentation_func=MIRROR_GO1)


def _rollout(runner):
    import torch

    fused = runner._make_fused()
    fused.begin()
    fused.rollout(T)
    with torch.inference_mode():
        runner.alg.compute_returns(fused.last_critic_obs)


@pytest.mark.parametrize("coeff", [0.0, 0.5], ids=["augmentation", "augmentation_and_mirror_loss"])
def test_one_direct_step_against_the_op_chain_in_float32_and_float64(coeff, monkeypatch):
    """ONE optimizer step from identical parameters on identical storage, three runners: `_direct_update` with symmetry, the torch op chain
    (`_symmetry_update`) in float32, and the same op chain in float64 (parameters and storage widened after the rollout).  Per parameter
    the direct form's gradient error against float64 is at most FACTOR times the float32 op chain's plus the comparator's floor
    (tests/ppo_ref.py `compare`); the loss scalars agree with the op chain within 2e-4 and the learning rates within 1e-5 of themselves."""
    import torch
    from locotouch_amd.rl import PPO, tuned_gemms

    tuned_gemms.disable()
    ran = []
    real = PPO._direct_update
    monkeypatch.setattr(PPO, "_direct_update", lambda self, *a, **k: (ran.append(self), real(self, *a, **k))[1])
    one = dict(log=False, epochs=1, mini_batches=1, tuned_gemms=False, symmetry_cfg=_symmetry_cfg(coeff))
    chain = dict(direct_update=False, fused_loss=False)
    a, b, c = (make_runner(**one, **kw) for kw in (dict(), chain, dict(chain, fused_adam=False, packed_forward=False)))
    seen = count_calls(monkeypatch, NEW_ENTRIES)
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
    assert len(seen["lt_sym_table_pack"]) == 3 and len(seen["lt_sym_gather_rows"]) == 2 and len(seen["lt_ppo_loss_sym"]) == 1
    for k in ("observations", "actions", "advantages", "returns", "actions_log_prob"):
        assert torch.equal(getattr(a.alg.storage, k), getattr(b.alg.storage, k)) and torch.equal(getattr(a.alg.storage, k).double(), getattr(c.alg.storage, k).double()), k
    print(f"\nPPOSYM one step coeff={coeff}: direct {outs[0]} op chain f32 {outs[1]} f64 {outs[2]} lr {a.alg.learning_rate} {b.alg.learning_rate} {c.alg.learning_rate}")
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
        print(f"PPOSYM   {name}: e_direct {e_a:.3e} e_op_chain {e_b:.3e} ratio {e_a / (e_b + R.EPS):.2f}")
        if not e_a <= R.FACTOR * e_b + R.FACTOR * R.EPS:
            bad[name] = (e_a, e_b)
    assert not bad, bad


def test_learn_launches_the_gather_twice_per_update_and_reads_the_host_once(tmp_path, monkeypatch):
    import torch
    from locotouch_amd.rl import PPO

    runner = make_runner(log=False, per_mb=True, tmp=str(tmp_path), symmetry_cfg=_symmetry_cfg(0.5))
    assert runner.alg.symmetry["_env"] is runner.env
    seen = count_calls(monkeypatch, NEW_ENTRIES + ("lt_adv_stats", "lt_ppo_loss", "lt_ppo_loss_opts", "lt_ppo_lr_rule"))
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
    assert len(seen["lt_sym_table_pack"]) == 3  # the three tables, once per PPO object
    assert len(seen["lt_sym_gather_rows"]) == 2 * 2 and len(seen["lt_adv_stats"]) == 2  # per update: two gathers, one statistics launch
    assert len(seen["lt_ppo_loss_sym"]) == 2 * 2 * 2 == len(seen["lt_ppo_lr_rule"])  # updates x epochs x minibatches
    assert not seen["lt_ppo_loss"] and not seen["lt_ppo_loss_opts"]
    M = N * T // 2
    for args in seen["lt_ppo_loss_sym"]:
        assert args[11] == M and args[12] == 12 and args[0].shape == (2 * M, 12) and args[2].numel() == 2 * M and args[20] == 0.5 and args[18] is not None
    for args in seen["lt_sym_gather_rows"]:
        assert args[1] == 0 and args[2] == N * T and args[3] == 348 and args[5] == 2 and args[6] == M and args[8].shape == (2 * 2 * M, 348)
    assert len(runner.history) == 2
    for rec in runner.history:
        assert all(math.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy", "Loss/learning_rate", "Loss/symmetry"))
        assert rec["Loss/symmetry"] > 0.0
    print(f"\nPPOSYM learn: Loss/symmetry {[rec['Loss/symmetry'] for rec in runner.history]} with mirror_loss_coeff 0.5")


def test_runner_without_symmetry_never_enters_the_new_entry_points(monkeypatch):
    """As every run before: rollout storage and parameters after one update are bit-equal to those of a twin for which a call of any of
    the three new entry points is an error, and whose records carry no Loss/symmetry."""
    import torch
    from tests.test_hip_ppo_opts_train import _rollout_and_update

    a = make_runner(log=False)
    out_a = _rollout_and_update(a)
    count_calls(monkeypatch, NEW_ENTRIES, forbid=True)
    b = make_runner(log=False)
    assert b.alg.symmetry is None and b.alg._sym_tables is None
    out_b = _rollout_and_update(b)
    for k in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "actions_log_prob", "returns", "advantages"):
        assert torch.equal(getattr(a.alg.storage, k), getattr(b.alg.storage, k)), k
    for (name, pa), pb in zip(a.alg.actor_critic.named_parameters(), b.alg.actor_critic.parameters()):
        assert torch.equal(pa, pb), name
    assert out_a == out_b and out_a[3:] == (None, None) and a.alg.learning_rate == b.alg.learning_rate
    b.learn(1)
    assert "Loss/symmetry" not in b.history[0]
