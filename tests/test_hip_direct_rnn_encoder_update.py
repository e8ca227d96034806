"""`PPO(direct_rnn_encoder_update=True)` on the GPU (rl/ppo.py `_direct_rnn_encoder_update`): the whole-rollout update of an
`ActorCriticRNNEncoder` with no autograd graph, no padded trajectories and one host read, against the eager update on the GPU and a
float64 CPU run of it, from identical parameters and storage.  GRU and LSTM memories, on the plan of
tests/test_hip_direct_recurrent_update.py (its `build` / `twin`, T = 6, its dones pattern, its bounds): rows 14 + 10 wide, memories with
H = 64, encoders [16, 8] -> 8 + tanh.

What is pinned tightly is ONE optimizer step: the clipped gradients of every parameter against float64, with the GPU eager update's own
error as the yardstick.  A whole update is held to that file's statistical bounds (PPO is a discontinuous map of its parameters)."""
import numpy as np
import pytest

from .test_recurrent_update_form import ACT, T, dones_pattern

pytestmark = pytest.mark.gpu
FLAT, TAIL, H = 14, 10, 64
D = FLAT + TAIL
KEY = dict(direct_rnn_encoder_update=True)
CELLS = ("gru", "lstm")


def policy(cell, act=ACT, **kw):
    from locotouch_amd.rl import ActorCriticRNNEncoder

    args = dict(actor_flatten_obs_end_idx=FLAT, actor_encoder_obs_start_idx=-TAIL, actor_encoder_hidden_dims=[16, 8], actor_encoder_embedding_dim=8,
                actor_hidden_dims=[32, 16], critic_flatten_obs_end_idx=FLAT, critic_encoder_obs_start_idx=-TAIL, critic_encoder_hidden_dims=[16, 8],
                critic_encoder_embedding_dim=8, critic_hidden_dims=[32, 16], encoder_rnn_type=cell, encoder_rnn_hidden_size=H,
                encoder_rnn_num_layers=1, encoder_activation="elu", encoder_final_activation="tanh", activation="elu", init_noise_std=1.0)
    args.update(kw)
    return ActorCriticRNNEncoder(D, D, act, **args)


def build(cell, n, device, dtype, nmb, epochs, **ppo_kw):
    """A PPO whose storage the eager loop of the class filled (the GRU with biases of order 1, as tests/test_gru_update_form.py has them)."""
    import torch

    from locotouch_amd.rl import PPO

    torch.manual_seed(5)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        ac = policy(cell)
        g = torch.Generator().manual_seed(9)
        with torch.no_grad():
            for mem in (ac.memory_a, ac.memory_c) if cell == "gru" else ():
                mem.rnn.weight_ih_l0.mul_(4.0)
                mem.rnn.bias_ih_l0.copy_(torch.randn(3 * H, generator=g))
                mem.rnn.bias_hh_l0.copy_(torch.randn(3 * H, generator=g))
        alg = PPO(ac, num_learning_epochs=epochs, num_mini_batches=nmb, schedule="adaptive", desired_kl=0.01, entropy_coef=0.01,
                  learning_rate=1e-3, device=device, **ppo_kw)
        alg.init_storage(n, T, [D], [D], [ACT])
        st = alg.storage
        for name in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "values", "returns", "advantages",
                     "actions_log_prob"):
            setattr(st, name, getattr(st, name).to(dtype))
        d = dones_pattern(max(n, 8))[:, :n].to(device)
        with torch.no_grad():
            for t in range(T):
                alg.act(torch.randn(n, D, generator=g).to(device), torch.randn(n, D, generator=g).to(device))
                alg.process_env_step(torch.randn(n, generator=g).to(device), d[t], {})
            st.saved_hidden_states_a = [s.to(dtype) for s in st.saved_hidden_states_a]
            st.saved_hidden_states_c = [s.to(dtype) for s in st.saved_hidden_states_c]
            alg.compute_returns(torch.randn(n, D, generator=g).to(device))
    finally:
        torch.set_default_dtype(prev)
    return alg


def twin(src, cell, n, device, dtype, nmb, epochs, **ppo_kw):
    """A PPO on `device` / `dtype` holding copies of `src`'s policy and filled storage."""
    import torch

    dst = build(cell, n, device, dtype, nmb, epochs, **ppo_kw)
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


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("n", [16, 5], ids=["96-rows", "30-rows"])
def test_one_optimizer_step_is_as_close_to_float64_as_the_eager_update(cell, n):
    """N = 16: 96 rows; N = 5: 30 rows, a partial block in the sequence kernels, the encoder kernels and the MLP kernels."""
    import torch

    from locotouch_amd.rl import tuned_gemms

    tuned_gemms.disable()  # both GPU forms on the library's default GEMM algorithms, as tests/test_hip_ppo_graph.py has them
    kw = dict(tuned_gemms=False)
    src = build(cell, n, "cuda:0", torch.float32, 1, 1, **kw)
    ref = twin(src, cell, n, "cpu", torch.float64, 1, 1, **kw)
    eager = twin(src, cell, n, "cuda:0", torch.float32, 1, 1, **kw)
    direct = twin(src, cell, n, "cuda:0", torch.float32, 1, 1, **KEY, **kw)
    assert direct.direct_rnn_encoder_update and not eager.direct_rnn_encoder_update
    assert direct._flat_adam is not None and eager._flat_adam is not None and ref._flat_adam is None
    r_ref, r_eager, r_direct = ref.update(), eager.update(), direct.update()
    torch.cuda.synchronize()
    assert direct._pair.last_backward == "fused" and float(direct._pair.saturated()) == 0.0
    print(f"\n[direct rnn-encoder update] {cell} N={n} losses: direct {r_direct[:3]}  eager {r_eager[:3]}  f64 {r_ref[:3]}")
    for a, b in zip(r_direct[:3], r_eager[:3]):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (r_direct, r_eager)
    # the rule runs in f32 on the device and in f64 on the host: one rounding of 1e-3 and one of the product, 2^-24 each
    assert abs(direct.learning_rate - eager.learning_rate) <= 2.0 ** -22 * eager.learning_rate, (direct.learning_rate, eager.learning_rate)
    assert abs(ref.learning_rate - eager.learning_rate) <= 1e-12
    assert direct.optimizer.param_groups[0]["lr"] == direct.learning_rate
    lo, hi = direct._flat_adam.flat_g.data_ptr(), direct._flat_adam.flat_g.data_ptr() + 4 * direct._flat_adam.flat_g.numel()
    for (k, p64), p_eager, p_direct in zip(ref.actor_critic.named_parameters(), eager.actor_critic.parameters(), direct.actor_critic.parameters()):
        g64 = p64.grad
        e_eager = float((p_eager.grad.double().cpu() - g64).abs().max())
        e_direct = float((p_direct.grad.double().cpu() - g64).abs().max())
        top = float(g64.abs().max())
        print(f"\n[direct rnn-encoder update] {cell} N={n} {k}: max |g - g64|  direct {e_direct:.3e}  eager update {e_eager:.3e}  max |g64| {top:.3e}")
        assert e_direct <= max(4.0 * e_eager, 1e-5 * top), (k, e_direct, e_eager, top)
        assert lo <= p_direct.grad.data_ptr() < hi  # written in place into the flat bucket
        # Adam's first step is lr * g / (|g| + eps): where |g| ~ eps = 1e-8 an error of 1e-9 is a visible fraction of lr
        torch.testing.assert_close(p_direct, p_eager, rtol=0, atol=2 * direct.learning_rate)


@pytest.mark.parametrize("cell", CELLS)
def test_a_whole_update_follows_the_eager_update(cell):
    import torch

    from locotouch_amd.rl import tuned_gemms

    tuned_gemms.disable()
    src = build(cell, 16, "cuda:0", torch.float32, 2, 2, tuned_gemms=False)
    eager = twin(src, cell, 16, "cuda:0", torch.float32, 2, 2, tuned_gemms=False)
    direct = twin(src, cell, 16, "cuda:0", torch.float32, 2, 2, tuned_gemms=False, **KEY)
    r_eager, r_direct = eager.update(), direct.update()
    torch.cuda.synchronize()
    print(f"\n[direct rnn-encoder update] {cell} 2 x 2 steps: direct {r_direct[:3]} lr {direct.learning_rate:.6e}   eager {r_eager[:3]} lr {eager.learning_rate:.6e}")
    assert abs(direct.learning_rate - eager.learning_rate) <= 1e-5 * eager.learning_rate  # the same decisions in all four steps
    for a, b in zip(r_direct[:3], r_eager[:3]):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (r_direct, r_eager)
    for (k, pe), pd in zip(eager.actor_critic.named_parameters(), direct.actor_critic.parameters()):
        torch.testing.assert_close(pd, pe, rtol=0, atol=4e-3, msg=lambda s: f"{k}: {s}")
    assert direct.storage.step == 0  # cleared, as every update leaves it


@pytest.mark.parametrize("cell", CELLS)
def test_no_autograd_and_one_host_read(cell, monkeypatch):
    import torch

    from locotouch_amd.rl import memory_seq
    from locotouch_amd.rl.storage import RolloutStorage
    from tests.test_hip_ppo_opts_train import count_scalar_reads

    direct = build(cell, 16, "cuda:0", torch.float32, 2, 2, **KEY)
    torch.cuda.synchronize()
    reads = {"tolist": 0}
    tolist = torch.Tensor.tolist

    def refuse(what):
        def f(*a, **k):
            raise AssertionError(f"{what} ran inside the direct rnn-encoder update")
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


def test_with_the_key_off_update_is_the_eager_one(monkeypatch):
    import torch

    from locotouch_amd.rl import PPO

    src = build("gru", 16, "cuda:0", torch.float32, 2, 2)
    a = twin(src, "gru", 16, "cuda:0", torch.float32, 2, 2)
    b = twin(src, "gru", 16, "cuda:0", torch.float32, 2, 2, direct_rnn_encoder_update=False)
    calls = []
    eager = PPO._eager_update
    monkeypatch.setattr(PPO, "_eager_update", lambda self: (calls.append(self), eager(self))[1])
    monkeypatch.setattr(PPO, "_direct_rnn_encoder_update", lambda self: pytest.fail("the direct form ran with the key off"))
    r_a, r_b = a.update(), b.update()
    torch.cuda.synchronize()
    assert calls == [a, b] and r_a == r_b and a.learning_rate == b.learning_rate
    for p, q in zip(a.actor_critic.parameters(), b.actor_critic.parameters()):
        assert torch.equal(p, q)


def test_construction_refuses_on_the_gpu_what_the_form_does_not_serve():
    from locotouch_amd.rl import PPO

    none = dict(critic_flatten_obs_end_idx=None, critic_encoder_obs_start_idx=None, critic_encoder_hidden_dims=None, critic_encoder_embedding_dim=None)
    for match, ac, kw in (("FlatAdam", policy("gru"), dict(fused_adam=False)),
                          ("packed_forward", policy("gru"), dict(packed_forward=False)),
                          ("the critic has no encoder", policy("gru", **none), {}),
                          ("2 layers", policy("lstm", encoder_rnn_num_layers=2), {}),
                          ("hidden size 96", policy("gru", encoder_rnn_hidden_size=96), {}),
                          (r"dims\[2\] must be", policy("gru", actor_encoder_embedding_dim=12), {}),
                          ("ELU stacks", policy("gru", activation="tanh"), {}),
                          ("action width is 17", policy("gru", act=17), {})):
        with pytest.raises(ValueError, match=r"^direct_rnn_encoder_update: .*" + match):
            PPO(ac, device="cuda:0", **KEY, **kw)
    frozen = policy("gru")
    frozen.actor_encoder.model[0].bias.requires_grad_(False)
    assert PPO(frozen, device="cuda:0", **KEY).direct_rnn_encoder_update  # (a frozen parameter asks for no gradient)
    for cell in CELLS:
        assert PPO(policy(cell), device="cuda:0", **KEY).direct_rnn_encoder_update
    # the keys of the other kinds stay refused for this class, with or without the new one
    with pytest.raises(ValueError, match=r"^fused_recurrent_update: the policy is an ActorCriticRNNEncoder"):
        PPO(policy("gru"), device="cuda:0", fused_recurrent_update=True, **KEY)


def test_bf16_observation_rows_are_refused_at_the_first_update():
    import torch

    alg = build("gru", 16, "cuda:0", torch.float32, 1, 1, **KEY)
    st = alg.storage
    st.observations, st.privileged_observations = st.observations.to(torch.bfloat16), st.privileged_observations.to(torch.bfloat16)
    with pytest.raises(ValueError, match=r"^direct_rnn_encoder_update: bf16 observation rows"):
        alg.update()


@pytest.mark.parametrize("case", ["gru64", "lstm64"])
def test_learn_iteration_with_both_keys_on(case, monkeypatch):
    import torch

    from locotouch_amd.rl import memory_seq
    from locotouch_amd.rl.storage import RolloutStorage

    from .test_hip_rnn_encoder_policy import make_runner

    def refuse(*a, **k):
        raise AssertionError("recurrent_mini_batches ran with direct_rnn_encoder_update on")

    runner = make_runner(case, direct_rnn_encoder_update=True)
    assert runner.alg.direct_rnn_encoder_update and runner._make_fused() is not None
    calls = {"hip": 0}
    forward = memory_seq.hip_forward

    def counted(*a, **k):
        calls["hip"] += 1
        return forward(*a, **k)

    monkeypatch.setattr(memory_seq, "hip_forward", counted)
    monkeypatch.setattr(RolloutStorage, "recurrent_mini_batches", refuse)
    named = list(runner.alg.actor_critic.named_parameters())
    before = [p.detach().clone() for _, p in named]
    runner.learn(1)
    assert calls["hip"] == 4  # 2 epochs x 2 mini-batches
    rec = runner.history[-1]
    assert all(np.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    assert all(bool(torch.isfinite(p).all()) for _, p in named)
    for group in ("memory_a.", "actor_encoder.", "memory_c.", "critic_encoder.", "actor.", "critic."):  # the update reaches every part
        assert any(k.startswith(group) and not torch.equal(p, q) for (k, p), q in zip(named, before)), group
