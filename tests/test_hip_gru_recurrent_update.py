"""`PPO(fused_recurrent_update=True, fused_gru_memories=True)` on the GPU (rl/ppo.py `_recurrent_update`: csrc/lt_memory_gru.hip per
optimizer step) against `_eager_update` from the same state - a float64 CPU run of it as the reference, the f32 GPU run of it as the
yardstick - at 64 envs x 8 steps.  The GRU counterpart of tests/test_hip_recurrent_update.py, with its tolerances: per parameter the
switch-on error against float64 is at most 2 x the switch-off error + 1e-6; the statistics agree to 1e-5 (on / off) and 1e-4 (on / f64).

The policy has nn.GRU's own initialisation, as the LSTM test's has nn.LSTM's.  With the float64 form test's memories (W_ih x 4, biases
of order 1: saturated gates, many elements of dW_hh near zero) the per-tensor figure is decided by Adam's normalised step, lr * m /
(sqrt(v) + eps), which turns the f32 rounding of a near-zero gradient element into up to 1e-5 of parameter error in EITHER leg: on the
MI355X that input gave memory_a.rnn.weight_hh_l0 4.68e-6 (switches on) against 1.00e-6 (eager) while the eager leg itself was 1.21e-5
off on critic.0.weight, and the same two updates in plain f32 PyTorch ops on the CPU give 8.2e-6 against 8.9e-6 on that tensor."""
import numpy as np
import pytest

from . import test_gru_update_form as form

pytestmark = pytest.mark.gpu
N, T = 64, 8
ON = dict(fused_recurrent_update=True, fused_gru_memories=True)


def twin(src, device, dtype, **ppo_kw):
    """A PPO on `device` / `dtype` holding copies of `src`'s policy and filled storage."""
    import torch

    dst = form.filled(2, n=N, device=device, dtype=dtype, default_init=True, **ppo_kw)
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


def test_update_with_the_switches_on_is_as_close_to_float64_as_the_eager_update(monkeypatch):
    import torch

    from locotouch_amd.rl import memory_seq

    monkeypatch.setattr(form, "T", T)  # 8 steps: the pattern's dones at T - 1 move with it
    src = form.filled(2, n=N, device="cuda:0", dtype=torch.float32, default_init=True)
    assert src.storage.observations.shape[:2] == (T, N)
    ref = twin(src, "cpu", torch.float64)
    off = twin(src, "cuda:0", torch.float32)
    on = twin(src, "cuda:0", torch.float32, **ON)
    assert on.fused_recurrent_update and on.fused_gru_memories and not off.fused_recurrent_update and on._flat_adam is not None
    calls = {"hip": 0}
    forward = memory_seq.hip_forward

    def counted(*a, **k):
        calls["hip"] += 1
        return forward(*a, **k)

    monkeypatch.setattr(memory_seq, "hip_forward", counted)
    r_ref, r_off, r_on = ref._eager_update(), off._eager_update(), on.update()
    torch.cuda.synchronize()
    assert calls["hip"] == 4  # 2 epochs x 2 mini-batches went through csrc/lt_memory_gru.hip
    assert ref.learning_rate == off.learning_rate == on.learning_rate
    err_on = err_off = 0.0
    for (k, p64), p_off, p_on in zip(ref.actor_critic.named_parameters(), off.actor_critic.parameters(), on.actor_critic.parameters()):
        e_off = float((p_off.detach().double().cpu() - p64.detach()).abs().max())
        e_on = float((p_on.detach().double().cpu() - p64.detach()).abs().max())
        print(f"\n{k}: max |err| vs the f64 eager update  switches on {e_on:.3e}  eager {e_off:.3e}")
        err_on, err_off = max(err_on, e_on), max(err_off, e_off)
        assert e_on <= 2.0 * e_off + 1e-6, (k, e_on, e_off)
    print(f"\nPPO.update GRU N={N} T={T} H={form.H}: max |parameter err| vs f64  switches on {err_on:.3e}  eager {err_off:.3e}")
    assert err_off > 0.0
    for a, b in zip(r_off[:3], r_on[:3]):
        assert abs(a - b) <= 1e-5 * max(abs(a), abs(b)), (r_off, r_on)
    for a, b in zip(r_ref[:3], r_on[:3]):
        assert abs(a - b) <= 1e-4 * max(abs(a), 1.0), (r_ref, r_on)


def test_the_switch_refuses_on_the_gpu_what_it_does_not_serve():
    from locotouch_amd.rl import PPO
    from locotouch_amd.rl.modules import ActorCriticRecurrent

    args = (form.OBS, form.COBS, form.ACT)
    with pytest.raises(ValueError, match="GRU"):
        PPO(ActorCriticRecurrent(*args, rnn_type="gru", rnn_hidden_size=form.H), device="cuda:0", fused_recurrent_update=True)
    with pytest.raises(ValueError, match="2 layers"):
        PPO(ActorCriticRecurrent(*args, rnn_type="gru", rnn_hidden_size=form.H, rnn_num_layers=2), device="cuda:0", **ON)


def test_learn_iteration_with_all_three_switches_on(monkeypatch):
    import torch
    from locotouch_amd.rl import memory_seq
    from locotouch_amd.rl.storage import RolloutStorage

    from .test_hip_gru_recurrent_rollout import make_runner

    runner = make_runner(64, fused_recurrent_update=True)
    assert runner.alg.fused_recurrent_update and runner.alg.fused_gru_memories and runner._make_fused() is not None
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
    assert calls["hip"] == 4  # 2 epochs x 2 mini-batches went through csrc/lt_memory_gru.hip
    rec = runner.history[-1]
    assert all(np.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    assert any(not torch.equal(p, q) for p, q in zip(runner.alg.actor_critic.parameters(), before))
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())
