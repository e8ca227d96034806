"""ActorCriticRNNEncoder (GRU and LSTM memories) + the PPO recurrent branch against tests/golden/rl_rnn_encoder.npz, recorded from the
reference's own `loco_rl` classes on the seeded rollout of tests/rnn_encoder_synth.py (tools/gen_golden_rnn_encoder.py): parameter
names / shapes / seeded initial weights, the rollout (hidden state carried, reset at dones, saved per step), advantages, the three
losses of one update, the adaptive learning rate and the post-update parameters - with the tolerances of tests/test_rl_policies.py.
Then the class on the runner's eager path (learn, checkpoints, the inference accessors), the critic without an encoder, and what is
refused by the class's name.  CPU only."""
import os

import numpy as np
import pytest
import torch

from locotouch_amd.rl import PPO, ActorCriticRNNEncoder, OnPolicyRunner
from tests.rnn_encoder_synth import CELLS, rnn_encoder_case

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rl_rnn_encoder.npz")
GROUPS = ["std", "actor.", "critic.", "memory_a.rnn.", "actor_encoder.", "memory_c.rnn.", "critic_encoder."]


@pytest.mark.parametrize("kind", CELLS)
def test_policy_class_rollout_and_update_match_reference(kind):
    torch.set_num_threads(1)
    g = np.load(GOLD)
    case = rnn_encoder_case(kind)
    torch.manual_seed(case["seed"])
    ac = ActorCriticRNNEncoder(*case["args"], **case["kwargs"])
    assert ac.is_recurrent
    sd = ac.state_dict()
    assert list(sd.keys()) == g[f"{kind}_keys"].tolist()
    groups = []  # the key groups in registration order
    for k in sd:
        grp = next(p for p in GROUPS if k.startswith(p))
        if not groups or groups[-1] != grp:
            groups.append(grp)
    assert groups == GROUPS
    assert [str(tuple(v.shape)) for v in sd.values()] == g[f"{kind}_shapes"].tolist()
    np.testing.assert_allclose([float(v.double().sum()) for v in sd.values()], g[f"{kind}_init_sums"], rtol=1e-9, atol=1e-9)
    alg = PPO(ac, device="cpu", **case["ppo"])
    N, T, D, A = case["N"], case["T"], case["D"], case["A"]
    alg.init_storage(N, T, [D], [D], [A])
    torch.manual_seed(case["seed"] + 1)
    with torch.inference_mode():
        for t in range(T):
            alg.act(case["obs"][t], case["cobs"][t])
            np.testing.assert_allclose(alg._t["log_prob"].numpy(), g[f"{kind}_logp"][t], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(alg._t["values"].numpy(), g[f"{kind}_values"][t], rtol=1e-5, atol=1e-6)
            alg.process_env_step(case["rewards"][t], case["dones"][t], {})
        alg.compute_returns(case["last_cobs"])
    np.testing.assert_allclose(alg.storage.actions.numpy(), g[f"{kind}_actions"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(alg.storage.advantages.numpy(), g[f"{kind}_adv"], rtol=1e-4, atol=1e-5)
    ns = 2 if kind == "lstm" else 1
    for saved in (alg.storage.saved_hidden_states_a, alg.storage.saved_hidden_states_c):
        assert len(saved) == ns and all(s.shape == (T, 1, N, 24) for s in saved)
        assert all((s[0] == 0).all() for s in saved)  # before the first step the memories hold nothing
    d = case["dones"].bool()
    t, e = [(int(a), int(b)) for a, b in d.nonzero() if a < T - 1][0]
    assert (alg.storage.saved_hidden_states_a[0][t + 1, 0, e] == 0).all()  # reset right after a done
    assert (alg.storage.saved_hidden_states_a[0][t + 1, 0, 2] != 0).any()  # (env 2 never finishes)
    torch.manual_seed(case["seed"] + 2)
    losses = alg.update()
    np.testing.assert_allclose(losses[:3], g[f"{kind}_losses"], rtol=2e-5, atol=1e-6)
    assert abs(alg.learning_rate - float(g[f"{kind}_lr"])) < 1e-12
    post = ac.state_dict()
    np.testing.assert_allclose([float(v.double().sum()) for v in post.values()], g[f"{kind}_post_sums"], rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose([float(v.double().abs().sum()) for v in post.values()], g[f"{kind}_post_abs"], rtol=1e-4, atol=2e-4)


def test_constructor_defaults_and_recurrent_distribution():
    import inspect

    p = inspect.signature(ActorCriticRNNEncoder.__init__).parameters
    assert (p["encoder_rnn_type"].default, p["encoder_rnn_hidden_size"].default, p["encoder_rnn_num_layers"].default) == ("gru", 256, 1)
    assert (p["encoder_activation"].default, p["encoder_final_activation"].default, p["activation"].default, p["init_noise_std"].default) == ("elu", None, "elu", 1.0)
    case = rnn_encoder_case("gru")
    torch.manual_seed(0)
    ac = ActorCriticRNNEncoder(*case["args"], **case["kwargs"])
    obs = case["obs"][0]
    mean = ac.act_inference(obs)
    h = ac.get_hidden_states()[0].clone()
    ac.reset()
    emb = ac.act_encoder_inference(obs[:, -5:])
    torch.testing.assert_close(ac.act_backbone_inference(obs[:, :9], emb), mean)
    torch.testing.assert_close(ac.get_hidden_states()[0], h)
    # the distribution of a padded batch from given hidden states: what `act(obs, masks, hidden_states)` builds, without the sample
    masks = torch.ones(2, case["N"], dtype=torch.bool)
    ac.update_distribution_recurrent(case["obs"][:2], masks, torch.zeros(1, case["N"], 24))
    assert ac.action_mean.shape == (2, case["N"], case["A"])
    torch.testing.assert_close(ac.action_mean[0], mean)


def runner_cfg(env, cell="gru", **keys):
    from locotouch_amd.agents import train_cfg

    d = env.get_observations()[0].shape[1]
    cfg = train_cfg("Isaac-RandCylinderTransportTeacher-LocoTouch-v1")
    cfg["policy"] = dict(class_name="ActorCriticRNNEncoder", init_noise_std=1.0, actor_flatten_obs_end_idx=d - 8, actor_encoder_obs_start_idx=-8,
                         actor_encoder_hidden_dims=[16], actor_encoder_embedding_dim=8, actor_hidden_dims=[32], critic_flatten_obs_end_idx=d - 8,
                         critic_encoder_obs_start_idx=-8, critic_encoder_hidden_dims=[16], critic_encoder_embedding_dim=8, critic_hidden_dims=[32],
                         encoder_rnn_type=cell, encoder_rnn_hidden_size=16, encoder_final_activation="tanh", activation="elu")
    cfg["num_steps_per_env"], cfg["algorithm"]["num_mini_batches"], cfg["algorithm"]["num_learning_epochs"] = 6, 2, 1
    cfg.update(keys)
    return cfg


@pytest.mark.parametrize("cell", CELLS)
def test_runner_builds_the_class_learns_and_round_trips_a_checkpoint(cell, tmp_path):
    from tests.distill_synth import ScriptedEnv

    torch.manual_seed(3)
    env = ScriptedEnv(6, form="tuple")
    r = OnPolicyRunner(env, runner_cfg(env, cell), log_dir=None, device="cpu")
    assert type(r.alg.actor_critic) is ActorCriticRNNEncoder and r._make_fused() is None
    before = {k: v.clone() for k, v in r.alg.actor_critic.state_dict().items()}
    r.learn(2)
    assert len(r.history) == 2
    assert all(np.isfinite(r.history[-1][k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    after = r.alg.actor_critic.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith("memory_a."))  # the update reaches the memories
    path = str(tmp_path / "model.pt")
    r.save(path)
    r2 = OnPolicyRunner(ScriptedEnv(6, form="tuple"), runner_cfg(env, cell), log_dir=None, device="cpu")
    r2.load(path)
    assert r2.current_learning_iteration == r.current_learning_iteration
    for k, v in after.items():
        assert torch.equal(v, r2.alg.actor_critic.state_dict()[k]), k
    # the inference accessors on the eager path: both runners step the same rows from a fresh memory to the same actions
    obs = env.get_observations()[0]
    with torch.inference_mode():  # (the state the rollout left in the memories was made in inference mode, as scripts/play.py steps)
        for x in (r, r2):
            x.alg.actor_critic.reset()
        a1, a2 = r.get_inference_policy()(obs), r2.get_inference_policy()(obs)
        assert a1.shape == (6, env.num_actions) and torch.equal(a1, a2)
        enc = r.get_inference_encoder()
        r.alg.actor_critic.reset()
        emb = enc(obs[:, -8:])
        assert emb.shape == (6, 8)
        torch.testing.assert_close(r.alg.actor_critic.act_backbone_inference(obs[:, :-8], emb), a1)


def test_critic_without_encoder_returns_no_critic_state_and_survives_an_update_with_dones():
    torch.set_num_threads(1)
    case = rnn_encoder_case("gru")
    kw = dict(case["kwargs"], critic_flatten_obs_end_idx=None, critic_encoder_obs_start_idx=None, critic_encoder_hidden_dims=None,
              critic_encoder_embedding_dim=None)
    torch.manual_seed(case["seed"])
    ac = ActorCriticRNNEncoder(*case["args"], **kw)
    assert not ac.critic_with_encoder and not hasattr(ac, "memory_c") and ac.critic[0].in_features == case["D"]
    assert not any(k.startswith(("memory_c.", "critic_encoder.")) for k in ac.state_dict())
    alg = PPO(ac, device="cpu", **case["ppo"])
    N, T, D, A = case["N"], case["T"], case["D"], case["A"]
    alg.init_storage(N, T, [D], [D], [A])
    assert case["dones"][:-1].any()  # trajectories end inside the rollout: the padded batch has more columns than envs
    with torch.inference_mode():
        for t in range(T):
            alg.act(case["obs"][t], case["cobs"][t])
            h_a, h_c = ac.get_hidden_states()
            assert h_a.shape == (1, N, 24) and h_c is None
            alg.process_env_step(case["rewards"][t], case["dones"][t], {})
        alg.compute_returns(case["last_cobs"])
    assert alg.storage.saved_hidden_states_c is None
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    losses = alg.update()  # (the reference's class fails here with a shape error: its evaluate does not unpad the critic's rows)
    assert all(np.isfinite(x) for x in losses[:3])
    assert not torch.equal(before["critic.0.weight"], ac.state_dict()["critic.0.weight"])


REFUSED_KEYS = [dict(fused_recurrent_update=True), dict(fused_recurrent_update=True, direct_recurrent_update=True), dict(fused_encoder_policy=True),
                dict(fused_recurrent_rollout=True)]


@pytest.mark.parametrize("keys", REFUSED_KEYS, ids=lambda k: "+".join(k))
def test_keys_of_other_kinds_are_refused_by_the_class_name(keys):
    from tests.distill_synth import ScriptedEnv

    env = ScriptedEnv(6, form="tuple")
    with pytest.raises((ValueError, NotImplementedError), match=rf"^{list(keys)[-1]}: .*ActorCriticRNNEncoder"):
        OnPolicyRunner(env, runner_cfg(env, **keys), log_dir=None, device="cpu")
    case = rnn_encoder_case("gru")
    ppo_keys = {k: v for k, v in keys.items() if k != "fused_recurrent_rollout"}
    if ppo_keys:
        with pytest.raises(ValueError, match="ActorCriticRNNEncoder"):
            PPO(ActorCriticRNNEncoder(*case["args"], **case["kwargs"]), device="cpu", **ppo_keys)


def test_fused_inference_and_export_are_refused_by_the_class_name(tmp_path):
    from locotouch_amd.compat.runtime import export_policy_as_jit
    from tests.distill_synth import ScriptedEnv

    env = ScriptedEnv(6, form="tuple")
    r = OnPolicyRunner(env, runner_cfg(env), log_dir=None, device="cpu")
    with pytest.raises(NotImplementedError, match="ActorCriticRNNEncoder"):
        r.get_inference_policy(fused=True)
    with pytest.raises(NotImplementedError, match="ActorCriticRNNEncoder"):
        export_policy_as_jit(r.alg.actor_critic, None, path=str(tmp_path))
    assert not os.listdir(tmp_path)


def test_the_off_key_keeps_the_eager_loop_and_the_names_are_exported():
    import locotouch_amd.compat.loco_rl.modules as compat_modules
    import locotouch_amd.rl as rl
    from tests.distill_synth import ScriptedEnv

    assert compat_modules.ActorCriticRNNEncoder is rl.ActorCriticRNNEncoder is ActorCriticRNNEncoder
    assert "ActorCriticRNNEncoder" in rl.__all__ and "ActorCriticRNNEncoder" in compat_modules.__all__
    env = ScriptedEnv(6, form="tuple")
    cfg = runner_cfg(env)
    cfg["policy"]["class_name"] = "ActorCriticPreEncoderRNNEncoder"
    with pytest.raises(NotImplementedError, match=r"'ActorCriticPreEncoderRNNEncoder'.*ActorCritic, ActorCriticRecurrent, ActorCriticEncoder, ActorCriticRNNEncoder are"):
        OnPolicyRunner(env, cfg, log_dir=None, device="cpu")
