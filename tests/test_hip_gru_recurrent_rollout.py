"""The fused rollout of a recurrent GRU policy - runner cfg `fused_recurrent_rollout` together with `fused_gru_memories` - on the HIP env:
three launches per step (csrc/lt_memory_gru.hip, the policy + value launch on the two h buffers, the env step).  The storage it fills is
checked for SELF-CONSISTENCY against float64 torch on the modules' own parameters, driven by the same actions - the GRU counterpart of
tests/test_hip_recurrent_rollout.py, with its tolerances."""
import numpy as np
import pytest

from .test_hip_recurrent_rollout import HID, T, TOL, TOL_LP, mlp64
from .test_hip_recurrent_rollout import make_runner as make_lstm_runner

pytestmark = pytest.mark.gpu


def make_runner(n, tmp=None, key=True, **cfg_over):
    return make_lstm_runner(n, tmp=tmp, rnn_type="gru", **({"fused_gru_memories": True} if key else {}), **cfg_over)


def cell64(rnn, x, h):
    import torch

    gi = x.double() @ rnn.weight_ih_l0.double().t() + rnn.bias_ih_l0.double()
    gh = h.double() @ rnn.weight_hh_l0.double().t() + rnn.bias_hh_l0.double()
    (ir, iz, i_n), (hr, hz, hn) = gi.chunk(3, dim=1), gh.chunk(3, dim=1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    return (1 - z) * torch.tanh(i_n + r * hn) + z * h.double()


def storage_snapshot(runner):
    st = runner.alg.storage
    keys = ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "actions_log_prob")
    snap = {k: getattr(st, k).clone() for k in keys}
    ac = runner.alg.actor_critic
    for name, saved, mem in (("a", st.saved_hidden_states_a, ac.memory_a), ("c", st.saved_hidden_states_c, ac.memory_c)):
        snap[f"saved_{name}"], snap[f"state_{name}"] = saved[0].clone(), mem.hidden_states.clone()
    return snap


def test_the_key_is_what_opens_the_fused_path():
    from locotouch_amd.rl import FusedRollout

    off = make_runner(64, key=False)
    assert off._make_fused() is None and not off.alg.fused_gru_memories  # as before: a GRU policy collects in the eager loop
    with pytest.raises(ValueError, match="GRU"):
        FusedRollout(off.env, off.alg)
    alone = make_runner(64, switch=False)
    assert alone._make_fused() is None and alone.alg.fused_gru_memories  # on its own the key does nothing
    on = make_runner(64)
    fused = on._make_fused()
    assert isinstance(fused, FusedRollout) and fused.recurrent and fused.gru and fused.launches_per_step == 3
    assert isinstance(FusedRollout(on.env, on.alg, fused_gru_memories=True), FusedRollout)
    norm = make_runner(64, empirical_normalization=True)
    assert norm._make_fused() is None
    with pytest.raises(ValueError, match="normalis"):
        FusedRollout(norm.env, norm.alg, obs_normalizer=norm.obs_normalizer, critic_obs_normalizer=norm.critic_obs_normalizer,
                     fused_gru_memories=True)


def test_rollout_storage_is_self_consistent_against_float64():
    import torch

    n = 64
    runner = make_runner(n)
    ac, alg, env = runner.alg.actor_critic, runner.alg, runner.env
    with torch.no_grad():  # b_hn of order 0.3: its place inside r * (...) is not a rounding matter
        for mem in (ac.memory_a, ac.memory_c):
            mem.rnn.bias_hh_l0.copy_(0.3 * torch.randn_like(mem.rnn.bias_hh_l0))
    fused = runner._make_fused()
    assert fused.actor_mlp is not None and fused.launches_per_step == 3  # the packed path: memory step, policy + value, env step
    fused.begin()
    assert all(torch.is_tensor(m.hidden_states) and m.hidden_states.shape == (1, n, HID) and torch.count_nonzero(m.hidden_states) == 0
               for m in (ac.memory_a, ac.memory_c))
    fused.rollout(T)
    torch.cuda.synchronize()
    st = alg.storage
    dones = st.dones[:, :, 0] != 0
    assert bool(dones[:T - 1].any()), "no episode ended at a step t < T - 1: no reset was carried into a following step"
    assert bool((~dones[:T - 1]).any())
    std = ac.std.detach()
    nets = ((ac.memory_a, st.observations, st.saved_hidden_states_a, 0), (ac.memory_c, st.privileged_observations, st.saved_hidden_states_c, 1))
    for mem, rows, saved, k in nets:
        assert len(saved) == 1 and saved[0].shape == (T, 1, n, HID)
        assert torch.count_nonzero(saved[0][0]) == 0  # the rollout started from zeros
        for t in range(T):
            h64 = cell64(mem.rnn, rows[t], saved[0][t, 0])
            keep = (~dones[t]).unsqueeze(1)
            nxt = saved[0][t + 1, 0] if t < T - 1 else mem.hidden_states[0]
            torch.testing.assert_close(nxt.double(), torch.where(keep, h64, torch.zeros_like(h64)), **TOL)
            assert torch.count_nonzero(nxt[dones[t]]) == 0  # a reset is an exact zero
            if k == 0:
                torch.testing.assert_close(st.mu[t].double(), mlp64(ac.actor, h64), **TOL)
            else:
                torch.testing.assert_close(st.values[t].double(), mlp64(ac.critic, h64), **TOL)
        # the modules' state: where(dones[T - 1], 0, raw state of the last step), exactly
        raw = fused._hc[(T - 1) & 1][k][0][:n]
        assert torch.equal(mem.hidden_states[0], torch.where((~dones[T - 1]).unsqueeze(1), raw, torch.zeros_like(raw)))
    for t in range(T):
        assert torch.equal(st.sigma[t], std.expand(n, 12))
        lp = torch.distributions.Normal(st.mu[t].double(), std.double().expand(n, 12)).log_prob(st.actions[t].double()).sum(-1, keepdim=True)
        torch.testing.assert_close(st.actions_log_prob[t].double(), lp, **TOL_LP)
    # the storage serves the eager update's batches: one state tensor per memory
    raw = next(iter(st.recurrent_mini_batches(2, 1)))
    assert torch.is_tensor(raw[9][0]) and raw[9][0].shape[0] == 1 and raw[9][0].shape[2] == HID
    # one further EAGER step from the state the rollout left
    state = [m.hidden_states.clone() for m in (ac.memory_a, ac.memory_c)]
    with torch.inference_mode():
        ac.act(env.obs_policy)
        value = ac.evaluate(env.obs_critic)
    torch.testing.assert_close(ac.action_mean.double(), mlp64(ac.actor, cell64(ac.memory_a.rnn, env.obs_policy, state[0][0])), **TOL)
    torch.testing.assert_close(value.double(), mlp64(ac.critic, cell64(ac.memory_c.rnn, env.obs_critic, state[1][0])), **TOL)


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


def test_learn_iteration_with_the_eager_update(tmp_path, monkeypatch):
    import torch
    from locotouch_amd.rl import FusedRollout
    from locotouch_amd.rl.storage import RolloutStorage

    calls = {"rollout": 0, "batches": 0}
    rollout, batches = FusedRollout.rollout, RolloutStorage.recurrent_mini_batches

    def counted_rollout(self, *a, **k):
        calls["rollout"] += 1
        return rollout(self, *a, **k)

    def counted_batches(self, *a, **k):
        assert len(self.saved_hidden_states_a) == 1 and len(self.saved_hidden_states_c) == 1
        for b in batches(self, *a, **k):
            calls["batches"] += 1
            yield b

    monkeypatch.setattr(FusedRollout, "rollout", counted_rollout)
    monkeypatch.setattr(RolloutStorage, "recurrent_mini_batches", counted_batches)
    runner = make_runner(64, tmp=str(tmp_path))
    assert not runner.alg.fused_recurrent_update
    before = [p.detach().clone() for p in runner.alg.actor_critic.parameters()]
    runner.learn(1)
    assert calls["rollout"] == 1 and calls["batches"] == 4  # 2 epochs x 2 mini-batches read the slots the kernel filled
    rec = runner.history[-1]
    assert all(np.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    assert any(not torch.equal(p, q) for p, q in zip(runner.alg.actor_critic.parameters(), before))
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())
