"""`PPO(fused_recurrent_update=True)` on the GPU (rl/ppo.py `_recurrent_update`: csrc/lt_memory.hip per optimizer step) against a float64
CPU run of the eager update on copies of the same policy and storage, beside the switch-off GPU update."""
import numpy as np
import pytest

from .test_recurrent_update_form import ACT, COBS, H, OBS, T, filled

pytestmark = pytest.mark.gpu
N = 16


def twin(src, device, dtype, **ppo_kw):
    """A PPO on `device` / `dtype` holding copies of `src`'s policy and filled storage."""
    import torch

    dst = filled(2, n=N, device=device, dtype=dtype, **ppo_kw)
    with torch.no_grad():
        for p, q in zip(dst.actor_critic.parameters(), src.actor_critic.parameters()):
            p.copy_(q)
        for name in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "returns", "advantages",
                     "actions_log_prob"):
            getattr(dst.storage, name).copy_(getattr(src.storage, name))
        for a, b in zip(dst.storage.saved_hidden_states_a + dst.storage.saved_hidden_states_c,
                        src.storage.saved_hidden_states_a + src.storage.saved_hidden_states_c):
            a.copy_(b)
    return dst


def test_update_with_the_switch_on_is_as_close_to_float64_as_the_switch_off_update():
    import torch

    src = filled(2, n=N, device="cuda:0", dtype=torch.float32)
    ref = twin(src, "cpu", torch.float64)
    off, off2 = twin(src, "cuda:0", torch.float32), twin(src, "cuda:0", torch.float32)
    on = twin(src, "cuda:0", torch.float32, fused_recurrent_update=True)
    assert on.fused_recurrent_update and not off.fused_recurrent_update and on._flat_adam is not None
    r_ref, r_off, r_off2, r_on = ref.update(), off.update(), off2.update(), on.update()
    torch.cuda.synchronize()
    # the old path is what it was: two switch-off runs (the new module imported, a switch-on PPO alive) give the same bits
    for p, q in zip(off.actor_critic.parameters(), off2.actor_critic.parameters()):
        assert torch.equal(p, q)
    assert r_off == r_off2
    assert ref.learning_rate == off.learning_rate == on.learning_rate
    err_on = err_off = 0.0
    for (k, p64), p_off, p_on in zip(ref.actor_critic.named_parameters(), off.actor_critic.parameters(), on.actor_critic.parameters()):
        e_off = float((p_off.double().cpu() - p64).abs().max())
        e_on = float((p_on.double().cpu() - p64).abs().max())
        print(f"\n{k}: max |err| vs the f64 eager update  switch on {e_on:.3e}  switch off {e_off:.3e}")
        err_on, err_off = max(err_on, e_on), max(err_off, e_off)
        assert e_on <= 2.0 * e_off + 1e-6, (k, e_on, e_off)
    print(f"\nPPO.update N={N} T={T} H={H}: max |parameter err| vs f64  switch on {err_on:.3e}  switch off {err_off:.3e}")
    assert err_off > 0.0
    for a, b in zip(r_off[:3], r_on[:3]):
        assert abs(a - b) <= 1e-5 * max(abs(a), abs(b)), (r_off, r_on)
    for a, b in zip(r_ref[:3], r_on[:3]):
        assert abs(a - b) <= 1e-4 * max(abs(a), 1.0), (r_ref, r_on)


def test_the_switch_refuses_on_the_gpu_what_it_does_not_serve():
    from locotouch_amd.rl import PPO
    from locotouch_amd.rl.modules import ActorCriticRecurrent

    with pytest.raises(ValueError, match="GRU"):
        PPO(ActorCriticRecurrent(OBS, COBS, ACT, rnn_type="gru", rnn_hidden_size=H), device="cuda:0", fused_recurrent_update=True)
    with pytest.raises(ValueError, match="2 layers"):
        PPO(ActorCriticRecurrent(OBS, COBS, ACT, rnn_hidden_size=H, rnn_num_layers=2), device="cuda:0", fused_recurrent_update=True)


def test_learn_iteration_with_both_recurrent_switches_on(monkeypatch):
    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner, memory_seq
    from locotouch_amd.rl.storage import RolloutStorage

    task = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
    env = make(task, num_envs=64, device="cuda:0", seed=3, max_episode_length=3)  # episodes end inside the rollout
    cfg = train_cfg(task)
    cfg["policy"] = dict(class_name="ActorCriticRecurrent", init_noise_std=1.0, actor_hidden_dims=[128, 64], critic_hidden_dims=[128, 64],
                         activation="elu", rnn_type="lstm", rnn_hidden_size=64, rnn_num_layers=1)
    cfg["num_steps_per_env"] = 8
    cfg["algorithm"] = dict(cfg["algorithm"], num_mini_batches=2, num_learning_epochs=2)
    cfg["fused_recurrent_rollout"] = cfg["fused_recurrent_update"] = True
    torch.manual_seed(11)
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    assert runner.alg.fused_recurrent_update and runner._make_fused() is not None
    calls = {"hip": 0}
    forward = memory_seq.hip_forward

    def counted(*a, **k):
        calls["hip"] += 1
        return forward(*a, **k)

    def no_padding(self, *a, **k):
        raise AssertionError("recurrent_mini_batches ran with fused_recurrent_update on")

    monkeypatch.setattr(memory_seq, "hip_forward", counted)
    monkeypatch.setattr(RolloutStorage, "recurrent_mini_batches", no_padding)
    before = [p.detach().clone() for p in runner.alg.actor_critic.parameters()]
    runner.learn(1)
    assert calls["hip"] == 4  # 2 epochs x 2 mini-batches went through csrc/lt_memory.hip
    rec = runner.history[-1]
    assert all(np.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    assert any(not torch.equal(p, q) for p, q in zip(runner.alg.actor_critic.parameters(), before))
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())
