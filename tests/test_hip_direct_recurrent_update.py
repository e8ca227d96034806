"""`PPO(fused_recurrent_update=True, direct_recurrent_update=True)` on the GPU (rl/ppo.py `_direct_recurrent_update`): the whole-rollout
update of a recurrent policy with no autograd graph and one host read, against its autograd form (`fused_recurrent_update` alone) and a
float64 CPU run of the eager update, from identical parameters and storage.  LSTM and GRU memories, on the fixtures of
tests/test_recurrent_update_form.py / tests/test_gru_update_form.py (T = 6, H = 64, the dones pattern that holds every reset case).

What is pinned tightly is ONE optimizer step: the clipped gradients of every parameter against float64, with the autograd form's own error
as the yardstick.  Over several steps PPO is a discontinuous map of its parameters (tests/test_hip_ppo_graph.py: the ratio clip and the
value clip pick a branch per sample), so a whole update is held to that file's statistical bounds, which catch gross errors only."""
import numpy as np
import pytest

from .test_recurrent_update_form import ACT, COBS, H, OBS, T, dones_pattern

pytestmark = pytest.mark.gpu
KEYS = dict(fused_recurrent_update=True, direct_recurrent_update=True)


def build(rnn, n, device, dtype, nmb, epochs, log_std=False, **ppo_kw):
    """A PPO whose storage the eager ActorCriticRecurrent loop filled, as `filled` of the two fixture files builds it (the GRU one with
    its biases of order 1); `log_std`: the policy keeps log sigma (the constructor of a recurrent policy has no such argument, as in the
    reference, so the parameter is exchanged by hand)."""
    import torch

    from locotouch_amd.rl import PPO
    from locotouch_amd.rl.modules import ActorCriticRecurrent

    torch.manual_seed(5)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        ac = ActorCriticRecurrent(OBS, COBS, ACT, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_type=rnn, rnn_hidden_size=H)
        g = torch.Generator().manual_seed(9)
        with torch.no_grad():
            for mem in (ac.memory_a, ac.memory_c) if rnn == "gru" else ():
                mem.rnn.weight_ih_l0.mul_(4.0)
                mem.rnn.bias_ih_l0.copy_(torch.randn(3 * H, generator=g))
                mem.rnn.bias_hh_l0.copy_(torch.randn(3 * H, generator=g))
        if log_std:
            ac.log_std = torch.nn.Parameter(torch.log(ac.std.detach().clone()))
            del ac.std
            ac.noise_std_type = "log"
        kw = dict(fused_gru_memories=True) if rnn == "gru" else {}
        alg = PPO(ac, num_learning_epochs=epochs, num_mini_batches=nmb, schedule="adaptive", desired_kl=0.01, entropy_coef=0.01,
                  learning_rate=1e-3, device=device, **kw, **ppo_kw)
        alg.init_storage(n, T, [OBS], [COBS], [ACT])
        st = alg.storage
        for name in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "values", "returns", "advantages",
                     "actions_log_prob"):
            setattr(st, name, getattr(st, name).to(dtype))
        d = dones_pattern(max(n, 8))[:, :n].to(device)  # (the pattern is written for 8 envs; 5 keep its first five cases)
        with torch.no_grad():
            for t in range(T):
                alg.act(torch.randn(n, OBS, generator=g).to(device), torch.randn(n, COBS, generator=g).to(device))
                alg.process_env_step(torch.randn(n, generator=g).to(device), d[t], {})
            st.saved_hidden_states_a = [s.to(dtype) for s in st.saved_hidden_states_a]
            st.saved_hidden_states_c = [s.to(dtype) for s in st.saved_hidden_states_c]
            alg.compute_returns(torch.randn(n, COBS, generator=g).to(device))
    finally:
        torch.set_default_dtype(prev)
    return alg


def twin(src, rnn, n, device, dtype, nmb, epochs, log_std=False, **ppo_kw):
    """A PPO on `device` / `dtype` holding copies of `src`'s policy and filled storage."""
    import torch

    dst = build(rnn, n, device, dtype, nmb, epochs, log_std, **ppo_kw)
    with torch.no_grad():
        for (ka, p), (kb, q) in zip(dst.actor_critic.named_parameters(), src.actor_critic.named_parameters()):
            assert ka == kb
            p.copy_(q)
        for name in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "returns", "advantages",
                     "actions_log_prob"):
            getattr(dst.storage, name).copy_(getattr(src.storage, name))
        for a, b in zip(dst.storage.saved_hidden_states_a + dst.storage.saved_hidden_states_c,
                        src.storage.saved_hidden_states_a + src.storage.saved_hidden_states_c):
            a.copy_(b)
    return dst


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
@pytest.mark.parametrize("n,options", [(16, False), (5, False), (16, True)], ids=["96-rows", "30-rows", "log-std-minibatch-norm"])
def test_one_optimizer_step_is_as_close_to_float64_as_the_autograd_form(rnn, n, options):
    """N = 16: 96 rows; N = 5: 30 rows, a partial block in the sequence kernels (64 envs) and in the MLP kernels (16 rows); `options`:
    a log-std policy with per-minibatch advantage normalisation (lt_ppo_loss_opts, lt_adv_stats)."""
    import torch

    from locotouch_amd.rl import tuned_gemms

    tuned_gemms.disable()  # both GPU forms on the library's default GEMM algorithms, as tests/test_hip_ppo_graph.py has them
    kw = dict(log_std=options, normalize_advantage_per_mini_batch=options, tuned_gemms=False)
    src = build(rnn, n, "cuda:0", torch.float32, 1, 1, **kw)
    ref = twin(src, rnn, n, "cpu", torch.float64, 1, 1, **kw)
    auto = twin(src, rnn, n, "cuda:0", torch.float32, 1, 1, fused_recurrent_update=True, **kw)
    direct = twin(src, rnn, n, "cuda:0", torch.float32, 1, 1, **KEYS, **kw)
    assert direct.direct_recurrent_update and not auto.direct_recurrent_update and auto.fused_recurrent_update
    assert direct._flat_adam is not None and auto._flat_adam is not None and ref._flat_adam is None
    r_ref, r_auto, r_direct = ref.update(), auto.update(), direct.update()
    torch.cuda.synchronize()
    assert direct._pair.last_backward == "fused" and float(direct._pair.saturated()) == 0.0
    for a, b in zip(r_direct[:3], r_auto[:3]):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (r_direct, r_auto)
    # the rule runs in f32 on the device and in f64 on the host: one rounding of 1e-3 and one of the product, 2^-24 each
    assert abs(direct.learning_rate - auto.learning_rate) <= 2.0 ** -22 * auto.learning_rate, (direct.learning_rate, auto.learning_rate)
    assert abs(ref.learning_rate - auto.learning_rate) <= 1e-12
    assert direct.optimizer.param_groups[0]["lr"] == direct.learning_rate
    lo, hi = direct._flat_adam.flat_g.data_ptr(), direct._flat_adam.flat_g.data_ptr() + 4 * direct._flat_adam.flat_g.numel()
    for (k, p64), p_auto, p_direct in zip(ref.actor_critic.named_parameters(), auto.actor_critic.parameters(), direct.actor_critic.parameters()):
        g64 = p64.grad
        e_auto = float((p_auto.grad.double().cpu() - g64).abs().max())
        e_direct = float((p_direct.grad.double().cpu() - g64).abs().max())
        top = float(g64.abs().max())
        print(f"\n[direct recurrent update] {rnn} N={n} {k}: max |g - g64|  direct {e_direct:.3e}  autograd form {e_auto:.3e}  max |g64| {top:.3e}")
        assert e_direct <= max(4.0 * e_auto, 1e-5 * top), (k, e_direct, e_auto, top)
        assert lo <= p_direct.grad.data_ptr() < hi  # written in place into the flat bucket
        # Adam's first step is lr * g / (|g| + eps): where |g| ~ eps = 1e-8 an error of 1e-9 is a visible fraction of lr
        torch.testing.assert_close(p_direct, p_auto, rtol=0, atol=2 * direct.learning_rate)
        assert float((p_direct.detach() - p_auto.detach()).abs().mean()) < 1e-6, k


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_a_whole_update_follows_the_autograd_form(rnn):
    import torch

    from locotouch_amd.rl import tuned_gemms

    tuned_gemms.disable()
    src = build(rnn, 16, "cuda:0", torch.float32, 2, 2, tuned_gemms=False)
    auto = twin(src, rnn, 16, "cuda:0", torch.float32, 2, 2, fused_recurrent_update=True, tuned_gemms=False)
    direct = twin(src, rnn, 16, "cuda:0", torch.float32, 2, 2, tuned_gemms=False, **KEYS)
    r_auto, r_direct = auto.update(), direct.update()
    torch.cuda.synchronize()
    print(f"\n[direct recurrent update] {rnn} 2 x 2 steps: direct {r_direct[:3]} lr {direct.learning_rate:.6e}   autograd form {r_auto[:3]} lr {auto.learning_rate:.6e}")
    assert abs(direct.learning_rate - auto.learning_rate) <= 1e-5 * auto.learning_rate  # the same decisions in all four steps
    for a, b in zip(r_direct[:3], r_auto[:3]):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (r_direct, r_auto)
    for (k, pa), pd in zip(auto.actor_critic.named_parameters(), direct.actor_critic.parameters()):
        torch.testing.assert_close(pd, pa, rtol=0, atol=4e-3, msg=lambda s: f"{k}: {s}")
    assert direct.storage.step == 0  # cleared, as every update leaves it


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_no_autograd_and_one_host_read(rnn, monkeypatch):
    import torch

    from locotouch_amd.rl import memory_seq
    from locotouch_amd.rl.storage import RolloutStorage
    from tests.test_hip_ppo_opts_train import count_scalar_reads

    direct = build(rnn, 16, "cuda:0", torch.float32, 2, 2, **KEYS)
    torch.cuda.synchronize()
    reads = {"tolist": 0}
    tolist = torch.Tensor.tolist

    def refuse(what):
        def f(*a, **k):
            raise AssertionError(f"{what} ran inside the direct recurrent update")
        return f

    def counted(self, *a, **k):
        reads["tolist"] += 1
        return tolist(self, *a, **k)

    monkeypatch.setattr(memory_seq._SeqHip, "apply", refuse("_SeqHip.apply"))
    monkeypatch.setattr(torch.Tensor, "backward", refuse("Tensor.backward"))
    monkeypatch.setattr(RolloutStorage, "recurrent_mini_batches", refuse("recurrent_mini_batches"))
    monkeypatch.setattr(torch.Tensor, "item", refuse("Tensor.item"))
    monkeypatch.setattr(torch.Tensor, "tolist", counted)
    scalars = count_scalar_reads(monkeypatch)  # float(t), bool(t), int(t): reads that the two above do not see
    out = direct.update()
    monkeypatch.undo()
    assert reads["tolist"] == 1 and scalars == []
    assert all(np.isfinite(v) for v in out[:3])


def test_with_the_key_off_the_whole_rollout_update_is_what_it_was():
    """Two `fused_recurrent_update`-only runs, the new code imported and a direct-form PPO alive and updated between them: same bits."""
    import torch

    src = build("lstm", 16, "cuda:0", torch.float32, 2, 2)
    a = twin(src, "lstm", 16, "cuda:0", torch.float32, 2, 2, fused_recurrent_update=True)
    direct = twin(src, "lstm", 16, "cuda:0", torch.float32, 2, 2, **KEYS)
    b = twin(src, "lstm", 16, "cuda:0", torch.float32, 2, 2, fused_recurrent_update=True, direct_recurrent_update=False)
    r_a = a.update()
    direct.update()
    r_b = b.update()
    torch.cuda.synchronize()
    assert r_a == r_b and a.learning_rate == b.learning_rate
    for p, q in zip(a.actor_critic.parameters(), b.actor_critic.parameters()):
        assert torch.equal(p, q)


def test_construction_refuses_on_the_gpu_what_the_form_does_not_serve():
    import torch

    from locotouch_amd.rl import PPO
    from locotouch_amd.rl.modules import ActorCriticRecurrent

    def policy(**kw):
        return ActorCriticRecurrent(OBS, COBS, kw.pop("act", ACT), **dict(dict(actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_hidden_size=H), **kw))

    for match, ac, kw in (("FlatAdam", policy(), dict(fused_adam=False)),
                          ("GRU", policy(rnn_type="gru"), {}),
                          ("2 layers", policy(rnn_num_layers=2), {}),
                          ("multiples of 4", policy(actor_hidden_dims=[30, 16]), {}),
                          ("ELU stacks", policy(activation="tanh"), {}),
                          ("does not serve the actor", policy(actor_hidden_dims=[520, 16]), {}),
                          ("action width is 17", policy(act=17), {}),
                          ("packed_forward", policy(), dict(packed_forward=False))):
        with pytest.raises(ValueError, match=r"^direct_recurrent_update: .*" + match):
            PPO(ac, device="cuda:0", **KEYS, **kw)
    frozen = policy()
    frozen.std.requires_grad_(False)
    with pytest.raises(ValueError, match=r"^direct_recurrent_update: std has no gradient"):
        PPO(frozen, device="cuda:0", **KEYS)

    class TwoRanks:
        world_size, rank, local_rank = 2, 0, 0

    with pytest.raises(ValueError, match=r"^direct_recurrent_update: dist.world_size is 2"):
        PPO(policy(), device="cuda:0", dist=TwoRanks(), **KEYS)
    assert PPO(policy(), device="cuda:0", **KEYS).direct_recurrent_update and torch.cuda.is_available()


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_learn_iteration_with_every_recurrent_switch_on(rnn, monkeypatch):
    import torch

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner, memory_seq

    task = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
    env = make(task, num_envs=64, device="cuda:0", seed=3, max_episode_length=3)  # episodes end inside the rollout
    cfg = train_cfg(task)
    cfg["policy"] = dict(class_name="ActorCriticRecurrent", init_noise_std=1.0, actor_hidden_dims=[128, 64], critic_hidden_dims=[128, 64],
                         activation="elu", rnn_type=rnn, rnn_hidden_size=64, rnn_num_layers=1)
    cfg["num_steps_per_env"] = 8
    cfg["algorithm"] = dict(cfg["algorithm"], num_mini_batches=2, num_learning_epochs=2)
    cfg["fused_recurrent_rollout"] = cfg["fused_recurrent_update"] = cfg["direct_recurrent_update"] = True
    if rnn == "gru":
        cfg["fused_gru_memories"] = True
    torch.manual_seed(11)
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    assert runner.alg.direct_recurrent_update and runner.alg.fused_recurrent_update and runner._make_fused() is not None
    calls = {"hip": 0}
    forward = memory_seq.hip_forward

    def counted(*a, **k):
        calls["hip"] += 1
        return forward(*a, **k)

    monkeypatch.setattr(memory_seq, "hip_forward", counted)
    before = [p.detach().clone() for p in runner.alg.actor_critic.parameters()]
    runner.learn(1)
    assert calls["hip"] == 4  # 2 epochs x 2 mini-batches
    rec = runner.history[-1]
    assert all(np.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    assert all(not torch.equal(p, q) for p, q in zip(runner.alg.actor_critic.parameters(), before))
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())
