"""The equivalence `PPO(fused_recurrent_update=True)` rests on, in float64 on the CPU: one pass of the two LSTM memories over the whole
rollout [T, E] of an env block, the carried state zeroed wherever dones[t - 1] is set (rl/memory_seq.py, the PyTorch-op form), equals
the padded trajectories of the reference's recurrent update (`recurrent_mini_batches` + `act(..., masks, hidden_states)` / `evaluate`) -
outputs, every parameter gradient, and a whole `PPO.update()`."""
import copy

import pytest
import torch

from locotouch_amd.rl import PPO, memory_seq
from locotouch_amd.rl.memory_seq import memory_rollout_sequence
from locotouch_amd.rl.modules import ActorCriticRecurrent
from locotouch_amd.rl.storage import Batch

T, N, H, OBS, COBS, ACT = 6, 8, 64, 11, 14, 5


def dones_pattern(n=N):
    """env 0: no done; 1: t = 0; 2: t = T - 1; 3: two consecutive steps; 4: every step; 5: t = 0 and T - 1; 6, 7: one in the middle."""
    d = torch.zeros(T, n, dtype=torch.bool)
    d[0, 1] = d[T - 1, 2] = d[2, 3] = d[3, 3] = True
    d[:, 4] = True
    d[0, 5] = d[T - 1, 5] = True
    d[1, 6] = d[4, 7] = True
    for e in range(8, n):  # wider storages repeat the pattern
        d[:, e] = d[:, e % 8]
    return d


def filled(num_mini_batches, n=N, device="cpu", dtype=torch.float64, epochs=2, **ppo_kw):
    """A PPO whose storage the eager ActorCriticRecurrent loop (`act` / `process_env_step` -> `reset(dones)`) filled."""
    torch.manual_seed(5)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        ac = ActorCriticRecurrent(OBS, COBS, ACT, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_type="lstm", rnn_hidden_size=H)
        alg = PPO(ac, num_learning_epochs=epochs, num_mini_batches=num_mini_batches, schedule="adaptive", desired_kl=0.01, entropy_coef=0.01,
                  learning_rate=1e-3, device=device, **ppo_kw)
        alg.init_storage(n, T, [OBS], [COBS], [ACT])
        st = alg.storage
        for name in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "values", "returns", "advantages",
                     "actions_log_prob"):
            setattr(st, name, getattr(st, name).to(dtype))
        d = dones_pattern(n).to(device)
        g = torch.Generator().manual_seed(9)
        with torch.no_grad():
            for t in range(T):
                obs, cobs = torch.randn(n, OBS, generator=g).to(device), torch.randn(n, COBS, generator=g).to(device)
                alg.act(obs, cobs)
                alg.process_env_step(torch.randn(n, generator=g).to(device), d[t], {})
            st.saved_hidden_states_a = [s.to(dtype) for s in st.saved_hidden_states_a]
            st.saved_hidden_states_c = [s.to(dtype) for s in st.saved_hidden_states_c]
            alg.compute_returns(torch.randn(n, COBS, generator=g).to(device))
    finally:
        torch.set_default_dtype(prev)
    return alg


def test_the_pattern_holds_every_case_the_argument_has_to_survive():
    d = dones_pattern()
    assert not d[:, 0].any() and d[0, 1] and d[T - 1, 2] and (d[2, 3] and d[3, 3]) and d[:, 4].all()


@pytest.mark.parametrize("num_mini_batches", [2, 3], ids=["even_blocks", "leftover_envs_dropped"])
def test_one_pass_over_the_rollout_equals_the_padded_trajectories(num_mini_batches):
    alg = filled(num_mini_batches)
    ac, st = alg.actor_critic, alg.storage
    per = N // num_mini_batches
    assert st.saved_hidden_states_a[0].dtype == torch.float64 and (num_mini_batches != 3 or per * 3 < N)
    params = dict(ac.named_parameters())
    g = torch.Generator().manual_seed(3)
    for i, raw in enumerate(st.recurrent_mini_batches(num_mini_batches, 1)):
        b, (hid_a, hid_c), masks = Batch(*raw[:9]), raw[9], raw[10]
        wa, wc = torch.randn(T, per, ACT, generator=g, dtype=torch.float64), torch.randn(T, per, 1, generator=g, dtype=torch.float64)
        # the padded path, as `_eager_update` runs it
        ac.zero_grad()
        ac.act(b.obs, masks=masks, hidden_states=hid_a)
        mu_p = ac.action_mean
        v_p = ac.evaluate(b.critic_obs, masks=masks, hidden_states=hid_c)
        ((mu_p * wa).sum() + (v_p * wc).sum() + ac.get_actions_log_prob(b.actions).sum()).backward()
        grad_p = {k: p.grad.clone() for k, p in params.items() if p.grad is not None}
        # one pass over the block
        sl = (slice(None), slice(i * per, (i + 1) * per))
        ac.zero_grad()
        out_a, out_c = memory_rollout_sequence(ac.memory_a, ac.memory_c, st.observations[sl], st.privileged_observations[sl], st.dones[sl],
                                               tuple(h[0][sl] for h in st.saved_hidden_states_a), tuple(h[0][sl] for h in st.saved_hidden_states_c))
        assert out_a.shape == (T, per, H) and out_c.shape == (T, per, H)
        ac.update_distribution(out_a)
        mu_s, v_s = ac.action_mean, ac.critic(out_c)
        assert float((mu_s - mu_p).abs().max()) <= 1e-12 and float((v_s - v_p).abs().max()) <= 1e-12
        with torch.no_grad():  # the memories' outputs themselves
            pad_a = ac.memory_a(b.obs, masks, hid_a)
            pad_c = ac.memory_c(b.critic_obs, masks, hid_c)
        assert float((out_a - pad_a).abs().max()) <= 1e-12 and float((out_c - pad_c).abs().max()) <= 1e-12
        ((mu_s * wa).sum() + (v_s * wc).sum() + ac.get_actions_log_prob(st.actions[sl]).sum()).backward()
        assert set(grad_p) == {k for k, p in params.items() if p.grad is not None} and any("memory_a" in k for k in grad_p)
        for k, gp in grad_p.items():
            err = float((params[k].grad - gp).abs().max()) / max(float(gp.abs().max()), 1.0)
            assert err <= 1e-10, (k, err)


def test_a_whole_update_with_the_switch_on_equals_the_eager_update():
    off = filled(2)
    on = filled(2, fused_recurrent_update=True)
    assert on.fused_recurrent_update and not off.fused_recurrent_update
    for p, q in zip(off.actor_critic.parameters(), on.actor_critic.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(off.storage.advantages, on.storage.advantages)
    before = [p.detach().clone() for p in on.actor_critic.parameters()]
    r_off, r_on = off.update(), on.update()
    assert off.learning_rate == on.learning_rate and off.learning_rate != 1e-3  # the schedule moved, the same way in both
    assert [g["lr"] for g in off.optimizer.param_groups] == [g["lr"] for g in on.optimizer.param_groups]
    for (k, p), q, p0 in zip(off.actor_critic.named_parameters(), on.actor_critic.parameters(), before):
        assert float((p - q).abs().max()) <= 1e-9, k
        assert not torch.equal(q, p0), k
    for a, b in zip(r_off[:3], r_on[:3]):
        assert abs(a - b) <= 1e-9 * max(abs(a), 1.0)
    assert on.storage.step == 0


def test_the_switch_refuses_what_it_does_not_serve():
    from locotouch_amd.rl.modules import ActorCritic

    with pytest.raises(ValueError, match="GRU"):
        PPO(ActorCriticRecurrent(OBS, COBS, ACT, rnn_type="gru", rnn_hidden_size=H), fused_recurrent_update=True)
    with pytest.raises(ValueError, match="2 layers"):
        PPO(ActorCriticRecurrent(OBS, COBS, ACT, rnn_hidden_size=H, rnn_num_layers=2), fused_recurrent_update=True)
    with pytest.raises(ValueError, match="hidden size 96"):
        PPO(ActorCriticRecurrent(OBS, COBS, ACT, rnn_hidden_size=96), fused_recurrent_update=True)
    with pytest.raises(ValueError, match="ActorCritic"):
        PPO(ActorCritic(OBS, COBS, ACT), fused_recurrent_update=True)
    alg = PPO(ActorCriticRecurrent(OBS, COBS, ACT, rnn_hidden_size=H), fused_recurrent_update=True)
    alg.init_storage(N, T, [OBS], [COBS], [ACT], obs_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bfloat16"):
        alg.update()


@pytest.mark.parametrize("cell", [memory_seq.LSTM, memory_seq.GRU], ids=["lstm", "gru"])
def test_the_cell_table_names_only_what_the_headers_declare(cell):
    """A field or an entry point renamed in include/lt_memory*.h fails here, not first in a launch on the GPU."""
    from locotouch_amd import _abi

    def fields(struct):
        return [f for f, _ in struct._fields_]

    shared = ["w_ih", "w_hh", "b_ih", "b_hh"]
    record, dgates, short = [k for k, _ in cell.record], [k for k, _ in cell.dgates], [s[0] for s in cell.state]
    assert set(fields(cell.seq_net)) == {"x", "x_stride", "I", *shared, *cell.state, *record}
    assert set(fields(cell.seq_grad)) == {"dout", "w_hh", *cell.reads, *dgates, cell.carry}
    assert set(cell.reads) <= set(record) and {cell.d_ih, cell.d_hh} == set(dgates) and record[0] == "out" and "h_prev" in record
    # rl/fused.py fills the step structure by position
    assert fields(cell.step_net) == ["x", "I", *shared, *(f"{s}_in" for s in short), *(f"{s}_out" for s in short), *(f"saved_{s}" for s in short)]
    signatures = {**_abi.MEMORY_SIGNATURES, **_abi.MEMORY_SEQ_SIGNATURES, **_abi.MEMORY_GRU_SIGNATURES}
    for name in (cell.step, cell.finish, cell.seq_forward, cell.seq_backward, cell.backward_units):
        assert name in signatures, name
    assert len(signatures[cell.finish][1]) == 4 * len(cell.state) + 4  # raw and masked state of both memories, dones, N, H, stream
