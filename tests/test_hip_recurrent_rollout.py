"""The fused rollout of a recurrent (LSTM) policy - runner cfg `fused_recurrent_rollout` - on the HIP env: three launches per step
(csrc/lt_memory.hip, the policy + value launch on the two h buffers, the env step).  The storage it fills is checked for SELF-CONSISTENCY
against float64 torch on the modules' own parameters, which pins the path without depending on either noise stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
T, HID = 8, 64
# mu / value / log-prob tolerances: the ones of the fused-MLP rollout test, tests/test_hip_parity.py::test_fused_rollout_kernels_match_torch
# (mu and value rtol = atol = 1e-5, log-prob 1e-4, bootstrapped reward 1e-6); the f32 LSTM state is held to the mu / value figure
TOL, TOL_LP, TOL_REW = dict(rtol=1e-5, atol=1e-5), dict(rtol=1e-4, atol=1e-4), dict(rtol=1e-6, atol=1e-6)


def make_runner(n, tmp=None, rnn_type="lstm", switch=True, **cfg_over):
    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    env = make(TASK, num_envs=n, device="cuda:0", seed=3, max_episode_length=3)  # episodes end inside the rollout
    cfg = train_cfg(TASK)
    cfg["policy"] = dict(class_name="ActorCriticRecurrent", init_noise_std=1.0, actor_hidden_dims=[128, 64], critic_hidden_dims=[128, 64],
                         activation="elu", rnn_type=rnn_type, rnn_hidden_size=HID, rnn_num_layers=1)
    cfg["num_steps_per_env"] = T
    cfg["algorithm"] = dict(cfg["algorithm"], num_mini_batches=2, num_learning_epochs=2)
    if switch:
        cfg["fused_recurrent_rollout"] = True
    cfg.update(cfg_over)
    torch.manual_seed(11)
    runner = OnPolicyRunner(env, cfg, log_dir=tmp, device="cuda:0")
    with torch.no_grad():
        runner.alg.actor_critic.std.copy_(torch.linspace(0.3, 1.4, 12))
    return runner


def cell64(rnn, x, h, c):
    import torch

    a = (x.double() @ rnn.weight_ih_l0.double().t() + rnn.bias_ih_l0.double() + h.double() @ rnn.weight_hh_l0.double().t()
         + rnn.bias_hh_l0.double())
    i, f, g, o = a.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c.double() + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def mlp64(seq, x):
    import torch

    for m in seq:
        if hasattr(m, "weight"):
            x = x @ m.weight.double().t() + m.bias.double()
        else:
            assert isinstance(m, torch.nn.ELU)
            x = torch.nn.functional.elu(x)
    return x


def storage_snapshot(runner):
    st = runner.alg.storage
    keys = ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "actions_log_prob")
    snap = {k: getattr(st, k).clone() for k in keys}
    for name in ("saved_hidden_states_a", "saved_hidden_states_c"):
        for j, s in enumerate(getattr(st, name)):
            snap[f"{name}{j}"] = s.clone()
    ac = runner.alg.actor_critic
    for name, mem in (("memory_a", ac.memory_a), ("memory_c", ac.memory_c)):
        for j, s in enumerate(mem.hidden_states):
            snap[f"{name}{j}"] = s.clone()
    return snap


@pytest.mark.parametrize("n", [64, 40], ids=["rows_in_storage", "not_a_multiple_of_16"])
def test_rollout_storage_is_self_consistent_against_float64(n):
    _check_self_consistency(n, packed=True)


def test_torch_module_path_is_self_consistent_against_float64():
    """`use_packed_mlp=False` (`_step_torch`, the path of stacks outside lt_mlp's limits) behind the memory step: the same checks with the
    same tolerances - the float64 comparison does not care which GEMM produced mu."""
    _check_self_consistency(64, packed=False)


def _check_self_consistency(n, packed):
    import torch
    from locotouch_amd.rl import FusedRollout

    runner = make_runner(n)
    ac, alg, env = runner.alg.actor_critic, runner.alg, runner.env
    fused = runner._make_fused() if packed else FusedRollout(env, alg, use_packed_mlp=False)
    assert isinstance(fused, FusedRollout) and fused.recurrent and fused.rows_in_storage == (n % 16 == 0)
    # the packed path: memory step, policy + value, env step; the torch-module path: the memory step in front of its 11
    assert (fused.actor_mlp is not None) == packed and fused.launches_per_step == (3 if packed else 12)
    fused.begin()
    assert all(torch.count_nonzero(x) == 0 and x.shape == (1, n, HID) for m in (ac.memory_a, ac.memory_c) for x in m.hidden_states)
    fused.rollout(T)
    torch.cuda.synchronize()
    st = alg.storage
    dones = st.dones[:, :, 0] != 0
    assert bool(dones[:T - 1].any()), "no episode ended at a step t < T - 1: no reset was carried into a following step"
    assert bool((~dones[:T - 1]).any())
    std = ac.std.detach()
    nets = ((ac.memory_a, st.observations, st.saved_hidden_states_a, 0), (ac.memory_c, st.privileged_observations, st.saved_hidden_states_c, 1))
    for mem, rows, saved, k in nets:
        assert len(saved) == 2 and all(s.shape == (T, 1, n, HID) for s in saved)
        assert torch.count_nonzero(saved[0][0]) == 0 and torch.count_nonzero(saved[1][0]) == 0  # the rollout started from zeros
        for t in range(T):
            h64, c64 = cell64(mem.rnn, rows[t], saved[0][t, 0], saved[1][t, 0])
            keep = (~dones[t]).unsqueeze(1)
            zero = torch.zeros_like(h64)
            nxt = (saved[0][t + 1, 0], saved[1][t + 1, 0]) if t < T - 1 else (mem.hidden_states[0][0], mem.hidden_states[1][0])
            torch.testing.assert_close(nxt[0].double(), torch.where(keep, h64, zero), **TOL)
            torch.testing.assert_close(nxt[1].double(), torch.where(keep, c64, zero), **TOL)
            assert torch.count_nonzero(nxt[0][dones[t]]) == 0 and torch.count_nonzero(nxt[1][dones[t]]) == 0  # a reset is an exact zero
            if k == 0:
                torch.testing.assert_close(st.mu[t].double(), mlp64(ac.actor, h64), **TOL)
            else:
                torch.testing.assert_close(st.values[t].double(), mlp64(ac.critic, h64), **TOL)  # plain critic(h_t): the bootstrap is in the rewards
        # the modules' state: where(dones[T - 1], 0, raw state of the last step), exactly
        raw = fused._hc[(T - 1) & 1][k]
        keep = (~dones[T - 1]).unsqueeze(1)
        for j in range(2):
            assert torch.equal(mem.hidden_states[j][0], torch.where(keep, raw[j][:n], torch.zeros_like(raw[j][:n])))
    for t in range(T):
        assert torch.equal(st.sigma[t], std.expand(n, 12))
        lp = torch.distributions.Normal(st.mu[t].double(), std.double().expand(n, 12)).log_prob(st.actions[t].double()).sum(-1, keepdim=True)
        torch.testing.assert_close(st.actions_log_prob[t].double(), lp, **TOL_LP)
    assert not torch.equal(st.actions[0], st.actions[1])
    # the time-out bootstrap goes into the rewards (as tests/test_hip_parity.py::test_fused_rollout_kernels_match_torch checks it)
    exp_rew = env.reward_buf + alg.gamma * st.values[T - 1].squeeze(1) * env.time_out_buf.float()
    torch.testing.assert_close(st.rewards[T - 1].squeeze(1), exp_rew, **TOL_REW)
    assert torch.equal(st.dones[T - 1].squeeze(1), env.dones_buf.to(torch.uint8))
    # one further EAGER step from the state the rollout left
    state = [tuple(x.clone() for x in m.hidden_states) for m in (ac.memory_a, ac.memory_c)]
    with torch.inference_mode():
        ac.act(env.obs_policy)
        value = ac.evaluate(env.obs_critic)
    h64, _ = cell64(ac.memory_a.rnn, env.obs_policy, state[0][0][0], state[0][1][0])
    torch.testing.assert_close(ac.action_mean.double(), mlp64(ac.actor, h64), **TOL)
    h64, _ = cell64(ac.memory_c.rnn, env.obs_critic, state[1][0][0], state[1][1][0])
    torch.testing.assert_close(value.double(), mlp64(ac.critic, h64), **TOL)


def test_captured_rollout_replays_to_the_same_storage():
    """Two twin runners (same seeds): a warm rollout each, then a second rollout - launched directly on one, captured into a hipGraph
    and replayed on the other - from the same env state, counters and memory state."""
    import torch

    a, b = make_runner(64), make_runner(64)
    fa, fb = a._make_fused(), b._make_fused()
    for f in (fa, fb):
        f.begin()
    fa.rollout(T)
    fa.rollout(T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fb.rollout(T)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fb.rollout(T)
    graph.replay()
    torch.cuda.synchronize()
    sa, sb = storage_snapshot(a), storage_snapshot(b)
    assert bool(sa["dones"][:T - 1].any())
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.env.counters[[0, 3]], b.env.counters[[0, 3]])


def test_learn_iteration_with_the_switch_on(tmp_path, monkeypatch):
    import os

    import torch
    from locotouch_amd.rl import FusedRollout
    from locotouch_amd.rl.storage import RolloutStorage

    calls = {"rollout": 0, "batches": 0}
    rollout, batches = FusedRollout.rollout, RolloutStorage.recurrent_mini_batches

    def counted_rollout(self, *a, **k):
        calls["rollout"] += 1
        return rollout(self, *a, **k)

    def counted_batches(self, *a, **k):
        assert self.saved_hidden_states_a is not None and self.saved_hidden_states_c is not None
        for b in batches(self, *a, **k):
            calls["batches"] += 1
            yield b

    monkeypatch.setattr(FusedRollout, "rollout", counted_rollout)
    monkeypatch.setattr(RolloutStorage, "recurrent_mini_batches", counted_batches)
    runner = make_runner(64, tmp=str(tmp_path))
    before = [p.detach().clone() for p in runner.alg.actor_critic.parameters()]
    runner.learn(1)
    assert calls["rollout"] == 1 and calls["batches"] == 4  # 2 epochs x 2 mini-batches read the slots the kernel filled
    rec = runner.history[-1]
    assert all(np.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    assert any(not torch.equal(p, q) for p, q in zip(runner.alg.actor_critic.parameters(), before))
    ck = os.path.join(str(tmp_path), "model_0.pt")
    assert os.path.exists(ck)
    twin = make_runner(64)
    twin.load(ck)
    for p, q in zip(runner.alg.actor_critic.parameters(), twin.alg.actor_critic.parameters()):
        assert torch.equal(p, q)


def test_what_keeps_the_eager_loop():
    from locotouch_amd.rl import FusedRollout

    assert make_runner(64, switch=False)._make_fused() is None  # opt-in: off, the policy collects in the eager loop as before
    gru = make_runner(64, rnn_type="gru")
    assert gru._make_fused() is None
    with pytest.raises(ValueError, match="GRU"):
        FusedRollout(gru.env, gru.alg)
    norm = make_runner(64, empirical_normalization=True)
    assert norm._make_fused() is None
    with pytest.raises(ValueError, match="normalis"):
        FusedRollout(norm.env, norm.alg, obs_normalizer=norm.obs_normalizer, critic_obs_normalizer=norm.critic_obs_normalizer)
