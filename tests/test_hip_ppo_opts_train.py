"""`noise_std_type="log"` and `normalize_advantage_per_mini_batch` on the fused PPO path, from the runner down (rl/runner.py, rl/fused.py,
rl/ppo.py, rl/fused_loss.py; include/lt_ppo_opts.h): the rollout of a log-std policy is fused and stores the sigma its own launch
formed, a replayed hipGraph follows `log_std`, one optimizer step of `_direct_update` equals the autograd form within the bounds of
tests/test_hip_ppo_graph.py's one-step check, the statistics launch runs once per update, and a scalar-std runner never enters the new
entry points.  64 envs, T = 8, MLPs [128, 64], as tests/test_hip_recurrent_rollout.py."""
import math

import pytest

from tests import ppo_opts_ref as O
from tests import ppo_ref as R

pytestmark = pytest.mark.gpu

TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
N, T = 64, 8
# tests/test_hip_parity.py::test_fused_rollout_kernels_match_torch: mu rtol = atol = 1e-5, log-prob 1e-4
TOL, TOL_LP = dict(rtol=1e-5, atol=1e-5), dict(rtol=1e-4, atol=1e-4)
NEW_ENTRIES = ("lt_std_from_log", "lt_ppo_loss_opts", "lt_adv_stats")


def make_runner(log=True, per_mb=False, tmp=None, epochs=2, mini_batches=2, **alg_over):
    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    env = make(TASK, num_envs=N, device="cuda:0", seed=3, max_episode_length=3)  # episodes end inside the rollout
    cfg = train_cfg(TASK)
    cfg["policy"] = dict(class_name="ActorCritic", init_noise_std=1.0, actor_hidden_dims=[128, 64], critic_hidden_dims=[128, 64], activation="elu",
                         noise_std_type="log" if log else "scalar")
    cfg["num_steps_per_env"] = T
    cfg["algorithm"] = dict(cfg["algorithm"], num_mini_batches=mini_batches, num_learning_epochs=epochs, normalize_advantage_per_mini_batch=per_mb,
                            **alg_over)
    torch.manual_seed(11)
    runner = OnPolicyRunner(env, cfg, log_dir=tmp, device="cuda:0")
    ac = runner.alg.actor_critic
    with torch.no_grad():
        if log:
            ac.log_std.copy_(torch.log(torch.linspace(0.3, 1.4, 12)))
        else:
            ac.std.copy_(torch.linspace(0.3, 1.4, 12))
    return runner


def count_calls(monkeypatch, names=NEW_ENTRIES, forbid=False):
    """-> {entry: [argument tuples]} of every `_abi.call` of `names` from here on (`forbid`: such a call fails the test instead)"""
    from locotouch_amd import _abi

    seen, real = {n: [] for n in names}, _abi.call

    def call(name, *args):
        if name in seen:
            assert not forbid, f"{name} was called on the scalar-std path"
            seen[name].append(args)
        return real(name, *args)

    monkeypatch.setattr(_abi, "call", call)
    return seen


def count_scalar_reads(monkeypatch):
    """-> [dunder names] of every `float(t)`, `bool(t)` / `if t:` and `int(t)` of a tensor from here on: on a device tensor each is a
    blocking host read that watching `.item()` and `.tolist()` does not see.  `monkeypatch`: the fixture, or a context of it."""
    import torch

    seen = []
    for name in ("__float__", "__bool__", "__int__"):
        def wrapped(t, *a, _real=getattr(torch.Tensor, name), _name=name, **k):
            seen.append(_name)
            return _real(t, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, wrapped)
    return seen


def test_log_std_rollout_is_fused_and_stores_the_sigma_its_launch_formed(monkeypatch):
    import torch
    from locotouch_amd.rl import FusedRollout
    from tests.test_hip_recurrent_rollout import mlp64

    runner = make_runner()
    ac, st = runner.alg.actor_critic, runner.alg.storage
    fused = runner._make_fused()
    assert isinstance(fused, FusedRollout) and fused.actor_mlp is not None and fused.launches_per_step == 2
    seen = count_calls(monkeypatch)
    fused.begin()
    fused.rollout(T)
    torch.cuda.synchronize()
    assert len(seen["lt_std_from_log"]) == 1  # one launch per rollout, not per step
    buf = fused._std_buf
    assert buf.shape == (12,)
    case = dict(log_std=ac.log_std.detach().cpu())
    ref64 = O.std_from_log(case)
    report = R.compare(dict(std=st.sigma[0, 0].cpu()), ref64, [O.std_from_log(case, dtype=torch.float32), O.std_from_log(case, dtype=torch.float32, device="cuda:0")])
    print(f"\nPPOOPTS rollout sigma: {R.format_report(report)}")
    assert not R.failures(report), R.format_report(report)
    sig64 = ref64["std"].cuda()
    for t in range(T):
        assert torch.equal(st.sigma[t], buf.expand(N, 12))
        torch.testing.assert_close(st.mu[t].double(), mlp64(ac.actor, st.observations[t].double()), **TOL)
        lp = torch.distributions.Normal(st.mu[t].double(), sig64.expand(N, 12)).log_prob(st.actions[t].double()).sum(-1, keepdim=True)
        torch.testing.assert_close(st.actions_log_prob[t].double(), lp, **TOL_LP)
    z = (st.actions[:T] - st.mu[:T]) / buf
    assert not torch.equal(st.actions[0], st.actions[1]) and abs(float(z.mean())) < 0.1 and abs(float(z.std()) - 1.0) < 0.1


def test_replayed_graph_follows_log_std():
    """The refresh launch sits inside the captured region: a replay stores the sigma of the log_std it finds, not of the one captured."""
    import torch
    from locotouch_amd import _abi

    runner = make_runner()
    ac, st = runner.alg.actor_critic, runner.alg.storage
    fused = runner._make_fused()
    fused.begin()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fused.rollout(T)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        fused.rollout(T)
    g.replay()
    torch.cuda.synchronize()
    before = st.sigma[T - 1, 0].clone()
    with torch.no_grad():
        ac.log_std.add_(0.25)
    g.replay()
    torch.cuda.synchronize()
    want = torch.empty(12, device="cuda:0")
    _abi.call("lt_std_from_log", ac.log_std.data, 12, want, _abi.stream(torch.device("cuda:0")))
    torch.cuda.synchronize()
    for t in (0, T - 1):
        assert torch.equal(st.sigma[t], want.expand(N, 12))
    # (roundings between the two: log_std + 0.25, two exponentials of an ulp each, one product - under 5e-7 together)
    torch.testing.assert_close(want, before * math.exp(0.25), rtol=1e-6, atol=0)


def _rollout_and_update(runner, seed=11):
    import torch

    fused = runner._make_fused()
    fused.begin()
    fused.rollout(T)
    with torch.inference_mode():
        runner.alg.compute_returns(fused.last_critic_obs)
    torch.manual_seed(seed)
    return runner.alg.update()


@pytest.mark.parametrize("log,per_mb", [(True, False), (False, True), (True, True)], ids=["log_std", "per_minibatch_norm", "both"])
def test_one_direct_step_equals_the_autograd_form(log, per_mb, monkeypatch):
    """ONE optimizer step from identical parameters on identical storage: `_direct_update` against `_fused_update` (the same kernels
    behind autograd nodes, the host deciding the learning rate) - loss scalars to 1e-6, gradients to 3e-6 of the largest, parameters to
    one Adam step, the learning rate to 1e-5 of itself: the bounds of tests/test_hip_ppo_graph.py
    ::test_direct_update_without_host_reads_equals_the_autograd_form.  The torch op chain (`fused_loss=False`) on the same storage agrees
    in the loss scalars to 2e-4, the bound of ::test_update_with_fused_loss_equals_update_with_torch_ops."""
    import torch
    from locotouch_amd.rl import PPO, tuned_gemms

    tuned_gemms.disable()
    ran = []
    real = PPO._direct_update
    monkeypatch.setattr(PPO, "_direct_update", lambda self, *a, **k: (ran.append(self), real(self, *a, **k))[1])
    one = dict(epochs=1, mini_batches=1, tuned_gemms=False)
    a, b, c = (make_runner(log, per_mb, **one, **kw) for kw in (dict(), dict(direct_update=False), dict(fused_loss=False, direct_update=False)))
    seen = count_calls(monkeypatch)
    outs = [_rollout_and_update(r) for r in (a, b, c)]
    assert ran == [a.alg], "the direct update must have run for the first runner, and for it alone"
    assert len(seen["lt_ppo_loss_opts"]) == 2 and len(seen["lt_adv_stats"]) == (2 if per_mb else 0) and len(seen["lt_std_from_log"]) == (3 if log else 0)
    print(f"\nPPOOPTS one step log={log} per_mb={per_mb}: direct {outs[0][:3]} autograd {outs[1][:3]} torch ops {outs[2][:3]} lr {a.alg.learning_rate}")
    for x, y in zip(outs[0][:3], outs[1][:3]):
        assert abs(x - y) <= 1e-6 * max(1.0, abs(y)), outs
    for x, y in zip(outs[0][:3], outs[2][:3]):
        assert abs(x - y) <= 2e-4 * max(1.0, abs(y)), outs
    assert abs(a.alg.learning_rate - b.alg.learning_rate) <= 1e-5 * b.alg.learning_rate
    assert abs(a.alg.learning_rate - c.alg.learning_rate) <= 1e-5 * c.alg.learning_rate
    name_std = "log_std" if log else "std"
    for (name, pa), pb in zip(a.alg.actor_critic.named_parameters(), b.alg.actor_critic.parameters()):
        assert float((pa.grad - pb.grad).abs().max()) <= 3e-6 * float(pb.grad.abs().max()), name
        torch.testing.assert_close(pa, pb, rtol=0, atol=2 * a.alg.learning_rate)
        assert float((pa - pb).abs().mean()) < 1e-6, name
    assert name_std in dict(a.alg.actor_critic.named_parameters()) and float(getattr(a.alg.actor_critic, name_std).grad.abs().max()) > 0.0


def test_plain_direct_update_reads_the_host_once(monkeypatch):
    """`_direct_update` of a scalar-std runner without symmetry (2 epochs x 2 minibatches): ONE `.tolist()`, no `.item()`, and no
    `float(t)` / `bool(t)` / `int(t)` of a tensor inside `update()` - the domain record comes back in that one read."""
    import torch
    from locotouch_amd.rl import PPO

    runner = make_runner(log=False)
    ran = []
    real = PPO._direct_update
    monkeypatch.setattr(PPO, "_direct_update", lambda self, *a, **k: (ran.append(self), real(self, *a, **k))[1])
    fused = runner._make_fused()
    fused.begin()
    fused.rollout(T)
    with torch.inference_mode():
        runner.alg.compute_returns(fused.last_critic_obs)
    torch.cuda.synchronize()
    tolist, lists = torch.Tensor.tolist, []

    def refuse(*a, **k):
        raise AssertionError("Tensor.item() inside the update")

    def counted(t, *a, **k):
        lists.append(tuple(t.shape))
        return tolist(t, *a, **k)

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "item", refuse)
        m.setattr(torch.Tensor, "tolist", counted)
        scalars = count_scalar_reads(m)
        out = runner.alg.update()
    assert ran == [runner.alg]
    assert len(lists) == 1 and scalars == [], (lists, scalars)
    assert lists[0] == (6,)  # lr, three sums, the saturation count, the domain record
    assert all(math.isfinite(v) for v in out[:3]) and out[3:] == (None, None) and runner.alg.storage.step == 0


def test_learn_runs_the_statistics_once_per_update_and_checkpoints_log_std(tmp_path, monkeypatch):
    import torch
    from locotouch_amd.rl import PPO

    runner = make_runner(True, True, tmp=str(tmp_path))
    ran = []
    real = PPO._direct_update
    monkeypatch.setattr(PPO, "_direct_update", lambda self, *a, **k: (ran.append(self), real(self, *a, **k))[1])
    seen = count_calls(monkeypatch)
    log_std0 = runner.alg.actor_critic.log_std.detach().clone()
    runner.learn(2)
    assert len(ran) == 2 and len(seen["lt_adv_stats"]) == 2 and len(seen["lt_std_from_log"]) == 2  # per update / per rollout
    steps = seen["lt_ppo_loss_opts"]
    assert len(steps) == 2 * 2 * 2  # updates x epochs x minibatches
    # minibatch i of every epoch takes the two floats lt_adv_stats wrote for minibatch i
    for u in range(2):
        stats = seen["lt_adv_stats"][u][4]
        assert stats.shape == (2, 2) and seen["lt_adv_stats"][u][2:4] == (N * T // 2, 2)
        for k, args in enumerate(steps[4 * u:4 * u + 4]):
            assert args[17] == 1 and args[18].data_ptr() == stats.data_ptr() + 8 * (k % 2) and args[11] == N * T // 2
    assert len(runner.history) == 2
    for rec in runner.history:
        assert all(math.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy", "Loss/learning_rate", "Policy/mean_noise_std"))
    log_std = runner.alg.actor_critic.log_std.detach()
    assert bool(torch.isfinite(log_std).all()) and not torch.equal(log_std, log_std0)
    path = str(tmp_path / "ckpt.pt")
    runner.save(path)
    other = make_runner(True, True)
    assert not torch.equal(other.alg.actor_critic.log_std.detach(), log_std)
    other.load(path)
    assert torch.equal(other.alg.actor_critic.log_std.detach(), log_std)
    for pa, pb in zip(runner.alg.actor_critic.parameters(), other.alg.actor_critic.parameters()):
        assert torch.equal(pa, pb)


def test_scalar_std_runner_never_enters_the_new_entry_points(monkeypatch):
    """A scalar-std runner without the option, as every run before: its rollout storage and its parameters after one update are
    bit-equal to those of a twin for which a call of any of the three new entry points is an error, and which has no std buffer."""
    import torch

    a = make_runner(log=False)
    out_a = _rollout_and_update(a)
    count_calls(monkeypatch, forbid=True)
    b = make_runner(log=False)
    fused = b._make_fused()
    assert fused._std_buf is None and fused.launches_per_step == 2
    out_b = _rollout_and_update(b)
    for k in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "actions_log_prob", "returns", "advantages"):
        assert torch.equal(getattr(a.alg.storage, k), getattr(b.alg.storage, k)), k
    for (name, pa), pb in zip(a.alg.actor_critic.named_parameters(), b.alg.actor_critic.parameters()):
        assert torch.equal(pa, pb), name
    assert out_a[:3] == out_b[:3] and a.alg.learning_rate == b.alg.learning_rate
