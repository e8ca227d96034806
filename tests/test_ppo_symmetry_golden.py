"""PPO's `symmetry_cfg` branch as a chain of torch ops (rl/ppo.py `_symmetry_update`) on the CPU against what the reference's own
loco_rl PPO.update() produced with this project's `mirror_go1` on the same seeded 64-env x 24-step synthetic rollout
(tests/golden/ppo_symmetry.npz, tools/gen_golden_ppo_symmetry.py), in the four modes of a symmetry_cfg.  The five returned values, the
learning rate and sums over the parameters, with the tolerances of tests/test_rl_parity.py::test_ppo_update_matches_reference."""
import os
import warnings

import numpy as np
import pytest
import torch

from locotouch_amd.rl import PPO, ActorCritic
from locotouch_amd.rl.modules import ActorCriticRecurrent
from locotouch_amd.rl.symmetry import MIRROR_GO1, mirror_go1
from tests.rl_synth import N_ACT, N_ENVS, N_OBS, N_STEPS, POLICY_CFG, PPO_CFG, synth_rollout
from tests.symmetry_synth import MODES, TeacherRows, symmetry_cfg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_symmetry.npz")


def _run(mode, func=mirror_go1):
    torch.set_num_threads(1)
    torch.manual_seed(0)
    ac = ActorCritic(N_OBS, N_OBS, N_ACT, **POLICY_CFG)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alg = PPO(ac, device="cpu", symmetry_cfg=symmetry_cfg(mode, func, TeacherRows()), **PPO_CFG)
    alg.init_storage(N_ENVS, N_STEPS, [N_OBS], [N_OBS], [N_ACT])
    data = synth_rollout(seed=123)
    for t in range(N_STEPS):
        alg.act(data["obs"][t], data["critic_obs"][t])
        alg.process_env_step(data["rewards"][t], data["dones"][t], {"time_outs": data["time_outs"][t]})
    alg.compute_returns(data["last_critic_obs"])
    return alg


@pytest.mark.parametrize("mode", list(MODES))
def test_symmetric_update_matches_reference(mode):
    g = np.load(GOLD)
    alg = _run(mode, MIRROR_GO1 if mode == "both" else mirror_go1)  # (the module:function string resolves to the same function)
    assert alg.symmetry["data_augmentation_func"] is mirror_go1
    v, s, e, rnd, sym = alg.update()
    assert rnd is None
    np.testing.assert_allclose([v, s, e, sym], g[f"{mode}/losses"], rtol=1e-5, atol=1e-6)
    assert abs(alg.learning_rate - float(g[f"{mode}/learning_rate"])) < 1e-12
    sd = alg.actor_critic.state_dict()
    assert list(sd.keys()) == list(g[f"{mode}/param_names"])
    np.testing.assert_allclose([p.double().sum().item() for p in sd.values()], g[f"{mode}/param_sum"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose([p.double().abs().sum().item() for p in sd.values()], g[f"{mode}/param_abs_sum"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sd["std"].numpy(), g[f"{mode}/std"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(sd["actor.6.bias"].numpy(), g[f"{mode}/actor_last_bias"], rtol=1e-5, atol=1e-6)


def test_the_modes_differ_and_no_symmetry_keeps_its_five_values():
    g = np.load(GOLD)
    assert len({tuple(g[f"{m}/param_sum"].tolist()) for m in MODES}) == len(MODES)  # the golden tells the four modes apart
    torch.manual_seed(0)
    alg = PPO(ActorCritic(N_OBS, N_OBS, N_ACT, **POLICY_CFG), device="cpu", **PPO_CFG)
    assert alg.symmetry is None


def test_refusals():
    ac = lambda: ActorCritic(8, 8, 2, actor_hidden_dims=[8], critic_hidden_dims=[8], activation="elu")  # noqa: E731
    with pytest.raises(NotImplementedError, match=r"rnd_cfg.*DESIGN\.md §7"):
        PPO(ac(), device="cpu", rnd_cfg=dict(weight=1.0))
    rec = ActorCriticRecurrent(8, 8, 2, actor_hidden_dims=[8], critic_hidden_dims=[8], rnn_type="lstm", rnn_hidden_size=4)
    with pytest.raises(ValueError, match=r"symmetry_cfg.*recurrent"):
        PPO(rec, device="cpu", symmetry_cfg=symmetry_cfg("augment", mirror_go1, None))
    with pytest.raises(ValueError, match=r"symmetry_cfg.*callable"):
        PPO(ac(), device="cpu", symmetry_cfg=dict(use_data_augmentation=True, use_mirror_loss=False, data_augmentation_func=3))
    with pytest.raises(ValueError, match=r"module:function"):
        PPO(ac(), device="cpu", symmetry_cfg=dict(use_data_augmentation=True, use_mirror_loss=False, data_augmentation_func="nowhere:nothing"))
    with pytest.raises(ValueError, match=r"symmetry_cfg: unknown keys \['mirror_coef'\]"):
        PPO(ac(), device="cpu", symmetry_cfg=dict(use_data_augmentation=True, mirror_coef=1.0, data_augmentation_func=mirror_go1))
    with pytest.warns(UserWarning, match="logging"):
        PPO(ac(), device="cpu", symmetry_cfg=symmetry_cfg("logging_only", mirror_go1, None))
    assert PPO(ac(), device="cpu", some_other_key=1, symmetry_cfg=None).symmetry is None  # any other key still falls into **unused


def test_the_runner_hands_the_env_over_and_logs_the_symmetry_loss_only_when_configured(tmp_path):
    from locotouch_amd.rl import OnPolicyRunner

    class Env(TeacherRows):
        num_envs, num_actions, device, max_episode_length = 4, N_ACT, "cpu", 10

        def __init__(self):
            super().__init__()
            self.episode_length_buf = torch.zeros(4, dtype=torch.long)

        def get_observations(self):
            return torch.randn(4, N_OBS), {"observations": {}}

        def step(self, actions):
            return torch.randn(4, N_OBS), torch.randn(4), torch.zeros(4, dtype=torch.long), {"observations": {}}

    def runner(sym):
        alg = dict(PPO_CFG, num_mini_batches=2, num_learning_epochs=1)
        if sym:
            alg["symmetry_cfg"] = dict(use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=0.5, data_augmentation_func=MIRROR_GO1)
        cfg = dict(algorithm=alg, policy=dict(class_name="ActorCritic", init_noise_std=1.0, actor_hidden_dims=[16], critic_hidden_dims=[16], activation="elu"),
                   num_steps_per_env=3, save_interval=100)
        return OnPolicyRunner(Env(), cfg, log_dir=None, device="cpu")

    torch.manual_seed(0)
    r = runner(True)
    assert r.alg.symmetry["_env"] is r.env and "symmetry_cfg" in r.alg_cfg and "_env" not in r.cfg["algorithm"]["symmetry_cfg"]
    r.learn(1)
    assert np.isfinite(r.history[0]["Loss/symmetry"]) and r.history[0]["Loss/symmetry"] > 0.0
    # a symmetry_cfg that arrives as a config OBJECT (the agent cfg classes of compat/) reaches PPO as a dict of its own
    import types

    from locotouch_amd.compat.configclass import configclass

    @configclass
    class SymmetryCfg:
        use_data_augmentation: bool = True
        use_mirror_loss: bool = False
        mirror_loss_coeff: float = 0.0
        data_augmentation_func: str = MIRROR_GO1

    for obj in (SymmetryCfg(), types.SimpleNamespace(use_data_augmentation=True, use_mirror_loss=False, data_augmentation_func=MIRROR_GO1)):
        cfg = dict(algorithm=dict(PPO_CFG, symmetry_cfg=obj), policy=dict(init_noise_std=1.0, actor_hidden_dims=[16], critic_hidden_dims=[16], activation="elu"),
                   num_steps_per_env=3)
        o = OnPolicyRunner(Env(), cfg, log_dir=None, device="cpu")
        assert isinstance(o.alg.symmetry, dict) and o.alg.symmetry["data_augmentation_func"] is mirror_go1 and o.alg.symmetry["_env"] is o.env
    plain = runner(False)
    plain.learn(1)
    assert "Loss/symmetry" not in plain.history[0] and set(r.history[0]) - set(plain.history[0]) == {"Loss/symmetry"}
