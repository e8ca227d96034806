"""An `ActorCriticEncoder` behind `fused_encoder_policy` on the HIP env at 64 envs: the fused rollout step (csrc/lt_encoder.hip in
front of the policy + value launch, three launches per step), its capture into one hipGraph, the update without an autograd graph
(rl/ppo.py `_direct_encoder_update`) and a learn() iteration with a checkpoint round trip.  The shape is the reference's teacher cfg:
rows of 348 columns, head 270, the last 78 through 256 -> 128 -> 64 -> 64 (ELU, tanh behind it), a critic without an encoder.

Bounds.  The fused step's mu and values: the rule of tests/test_hip_encoder.py - against float64 on the same rows, at most the larger
of twice the eager f32 modules' error and one f32 ulp of the array's magnitude.  One optimizer step's gradients: the rule and margin of
tests/test_hip_direct_recurrent_update.py - against a float64 CPU run, at most the larger of 4 x the f32 autograd form's error and
1e-5 of the gradient's magnitude."""
import copy
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
T = 4
ENCODER_POLICY = dict(class_name="ActorCriticEncoder", init_noise_std=1.0, actor_flatten_obs_end_idx=270, actor_encoder_obs_start_idx=270,
                      actor_encoder_hidden_dims=[256, 128, 64], actor_encoder_embedding_dim=64, actor_hidden_dims=[128, 64],
                      critic_hidden_dims=[128, 64], encoder_activation="elu", encoder_final_activation="tanh", activation="elu")


def _ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


def make_runner(n=64, tmp=None, key=True, policy=None, **cfg_over):
    import torch

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    env = make(TASK, num_envs=n, device="cuda:0", seed=3, max_episode_length=3)  # episodes end inside the rollout
    cfg = train_cfg(TASK)
    cfg["policy"] = dict(ENCODER_POLICY, **(policy or {}))
    cfg["num_steps_per_env"] = T
    cfg["algorithm"] = dict(cfg["algorithm"], num_mini_batches=2, num_learning_epochs=2)
    if key:
        cfg["fused_encoder_policy"] = True
    cfg.update(cfg_over)
    torch.manual_seed(11)
    runner = OnPolicyRunner(env, cfg, log_dir=tmp, device="cuda:0")
    with torch.no_grad():
        runner.alg.actor_critic.std.copy_(torch.linspace(0.3, 1.4, 12))
    return runner


def test_one_fused_step_matches_float64_as_closely_as_the_eager_modules():
    import torch

    from locotouch_amd.rl import FusedRollout

    runner = make_runner()
    ac, st = runner.alg.actor_critic, runner.alg.storage
    assert st.observations.shape[-1] == 348 and ac.actor[0].in_features == 334 and not ac.critic_with_encoder
    fused = runner._make_fused()
    assert isinstance(fused, FusedRollout) and fused.encoders is not None and fused.actor_mlp is not None and fused.launches_per_step == 3
    fused.begin()
    rows0, crows0 = runner.env.obs_policy.clone(), runner.env.obs_critic.clone()
    fused.rollout(1)
    torch.cuda.synchronize()
    rows, crows = st.observations[0], st.privileged_observations[0]
    assert torch.equal(rows, rows0) and torch.equal(crows, crows0)  # the storage keeps the raw rows
    ac64 = copy.deepcopy(ac).double()
    with torch.no_grad():
        want = (ac64.act_inference(rows.double()), ac64.evaluate(crows.double()))
        eager = (ac.act_inference(rows), ac.evaluate(crows))
    for name, got, e, w in (("mu", st.mu[0], eager[0], want[0]), ("values", st.values[0], eager[1], want[1])):
        err_k, err_e = float((got.double() - w).abs().max()), float((e.double() - w).abs().max())
        bound = max(2.0 * err_e, _ulp(float(w.abs().max())))
        print(f"\n[encoder policy step] {name}: max |err| vs f64  fused {err_k:.3e}  eager modules {err_e:.3e}  bound {bound:.3e}")
        assert err_k <= bound, (name, err_k, err_e, bound)
    std = ac.std.detach()
    assert torch.equal(st.sigma[0], std.expand(64, 12))
    lp = torch.distributions.Normal(st.mu[0].double(), std.double().expand(64, 12)).log_prob(st.actions[0].double()).sum(-1, keepdim=True)
    torch.testing.assert_close(st.actions_log_prob[0].double(), lp, rtol=1e-4, atol=1e-4)


def storage_snapshot(runner):
    st, env = runner.alg.storage, runner.env
    keys = ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "actions_log_prob")
    snap = {k: getattr(st, k).clone() for k in keys}
    snap.update(env_obs=env.obs_policy.clone(), env_critic_obs=env.obs_critic.clone(), env_reward=env.reward_buf.clone(),
                env_dones=env.dones_buf.clone(), counters=env.counters[[0, 3]].clone())
    return snap


def test_captured_rollout_replays_to_the_directly_launched_one():
    """Twin runners (same seeds): a warm rollout each, then a second 4-step rollout - launched directly on one, captured into ONE hipGraph
    on one stream and replayed on the other - from the same env state and counters."""
    import torch

    a, b = make_runner(), make_runner()
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
    assert bool(sa["dones"][:T - 1].any()) and not torch.equal(sa["mu"][0], sa["mu"][1])
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_a_step_is_three_launches():
    import torch
    from torch.profiler import ProfilerActivity, profile

    runner = make_runner()
    fused = runner._make_fused()
    fused.begin()
    fused.rollout(T)  # warm

    def kernels_of(steps):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fused.rollout(steps)
            torch.cuda.synchronize()
        dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return [k for k in dev if "memcpy" not in k.lower() and "memset" not in k.lower()]

    two, four = kernels_of(2), kernels_of(4)
    print("\nkernels of a 2-step rollout:", [k.split("<")[0].split("(anonymous namespace)::")[-1][:40] for k in two])
    assert sum("lt_encoder_kernel" in k for k in two) == 2 and sum("lt_encoder_kernel" in k for k in four) == 4
    assert len(four) - len(two) == 2 * 3 == 2 * fused.launches_per_step, (len(two), len(four))


# ---- the update ---------------------------------------------------------------------------------------------------------------------------
OBS, COBS, ACT, N_ENVS, STEPS = 30, 20, 5, 16, 6
UPDATE_POLICIES = {
    # the actor's encoder alone, tanh behind it: the stacks' rows are 22 + 8 = 30 and 20 columns wide
    "actor-encoder-tanh": dict(actor_flatten_obs_end_idx=22, actor_encoder_obs_start_idx=-8, actor_encoder_hidden_dims=[16, 8],
                               actor_encoder_embedding_dim=8, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16],
                               encoder_activation="elu", encoder_final_activation="tanh"),
    # both encoders, no final activation, a single Linear for the critic's: rows of 30 and 10 + 8 = 18 columns
    "both-encoders": dict(actor_flatten_obs_end_idx=22, actor_encoder_obs_start_idx=-8, actor_encoder_hidden_dims=[16],
                          actor_encoder_embedding_dim=8, actor_hidden_dims=[32, 16], critic_flatten_obs_end_idx=10,
                          critic_encoder_obs_start_idx=-10, critic_encoder_hidden_dims=[], critic_encoder_embedding_dim=8,
                          critic_hidden_dims=[32, 16], encoder_activation="elu", encoder_final_activation=None),
}


def build(kind, device, dtype, nmb, epochs, **ppo_kw):
    """A PPO whose storage the eager ActorCriticEncoder loop filled from seeded rows."""
    import torch

    from locotouch_amd.rl import PPO
    from locotouch_amd.rl.modules import ActorCriticEncoder

    torch.manual_seed(5)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        ac = ActorCriticEncoder(OBS, COBS, ACT, **UPDATE_POLICIES[kind])
        g = torch.Generator().manual_seed(9)
        alg = PPO(ac, num_learning_epochs=epochs, num_mini_batches=nmb, schedule="adaptive", desired_kl=0.01, entropy_coef=0.01,
                  learning_rate=1e-3, device=device, **ppo_kw)
        alg.init_storage(N_ENVS, STEPS, [OBS], [COBS], [ACT])
        st = alg.storage
        for name in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "values", "returns", "advantages",
                     "actions_log_prob"):
            setattr(st, name, getattr(st, name).to(dtype))
        with torch.no_grad():
            for t in range(STEPS):
                alg.act(torch.randn(N_ENVS, OBS, generator=g).to(device=device, dtype=dtype), torch.randn(N_ENVS, COBS, generator=g).to(device=device, dtype=dtype))
                alg.process_env_step(torch.randn(N_ENVS, generator=g).to(device=device, dtype=dtype), (torch.rand(N_ENVS, generator=g) < 0.2).to(device), {})
            alg.compute_returns(torch.randn(N_ENVS, COBS, generator=g).to(device=device, dtype=dtype))
    finally:
        torch.set_default_dtype(prev)
    return alg


def twin(src, kind, device, dtype, nmb, epochs, **ppo_kw):
    """A PPO on `device` / `dtype` holding copies of `src`'s policy and filled storage."""
    import torch

    dst = build(kind, device, dtype, nmb, epochs, **ppo_kw)
    with torch.no_grad():
        for (ka, p), (kb, q) in zip(dst.actor_critic.named_parameters(), src.actor_critic.named_parameters()):
            assert ka == kb
            p.copy_(q)
        for name in ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "returns", "advantages",
                     "actions_log_prob"):
            getattr(dst.storage, name).copy_(getattr(src.storage, name))
    return dst


def float64_step(ref):
    """One optimizer step's clipped gradients in float64 autograd on the CPU: the reference's op chain (loco_rl/loco_rl/algorithms/
    ppo.py:216-319) on the whole storage as ONE minibatch (a mean over the rows: their order does not matter), left in `.grad`.
    (`RolloutStorage.mini_batches` hands out f32 observation rows whatever the storage holds, so the chain is written out here.)"""
    import torch

    ac, st = ref.actor_critic, ref.storage
    f = lambda t: t.flatten(0, 1).double()  # noqa: E731
    ac.act(f(st.observations))
    log_prob = ac.get_actions_log_prob(f(st.actions))
    value = ac.evaluate(f(st.privileged_observations))
    entropy = ac.entropy
    ratio = torch.exp(log_prob - torch.squeeze(f(st.actions_log_prob)))
    a = torch.squeeze(f(st.advantages))
    surrogate = torch.max(-a * ratio, -a * torch.clamp(ratio, 1.0 - ref.clip_param, 1.0 + ref.clip_param)).mean()
    old, returns = f(st.values), f(st.returns)
    clipped = old + (value - old).clamp(-ref.clip_param, ref.clip_param)
    value_loss = torch.max((value - returns).pow(2), (clipped - returns).pow(2)).mean()
    loss = surrogate + ref.value_loss_coef * value_loss - ref.entropy_coef * entropy.mean()
    ac.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(ac.parameters(), ref.max_grad_norm)
    return value_loss.item(), surrogate.item(), entropy.mean().item()


@pytest.mark.parametrize("kind", list(UPDATE_POLICIES))
def test_one_optimizer_step_is_as_close_to_float64_as_the_autograd_form(kind):
    import torch

    from locotouch_amd.rl import tuned_gemms

    tuned_gemms.disable()  # both GPU forms on the library's default GEMM algorithms, as tests/test_hip_ppo_graph.py has them
    src = build(kind, "cuda:0", torch.float32, 1, 1, tuned_gemms=False)
    ref = twin(src, kind, "cpu", torch.float64, 1, 1, tuned_gemms=False)
    auto = twin(src, kind, "cuda:0", torch.float32, 1, 1, tuned_gemms=False)
    direct = twin(src, kind, "cuda:0", torch.float32, 1, 1, tuned_gemms=False, fused_encoder_policy=True)
    assert direct.fused_encoder_policy and not auto.fused_encoder_policy
    assert direct._flat_adam is not None and auto._flat_adam is not None and ref._flat_adam is None
    r_ref, r_auto, r_direct = float64_step(ref), auto.update(), direct.update()
    torch.cuda.synchronize()
    for a, b, c in zip(r_direct[:3], r_auto[:3], r_ref):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)) and abs(b - c) <= 1e-5 * max(1.0, abs(c)), (r_direct, r_auto, r_ref)
    # the rule runs in f32 on the device and in f64 on the host: one rounding of 1e-3 and one of the product, 2^-24 each
    assert abs(direct.learning_rate - auto.learning_rate) <= 2.0 ** -22 * auto.learning_rate, (direct.learning_rate, auto.learning_rate)
    assert direct.optimizer.param_groups[0]["lr"] == direct.learning_rate
    lo, hi = direct._flat_adam.flat_g.data_ptr(), direct._flat_adam.flat_g.data_ptr() + 4 * direct._flat_adam.flat_g.numel()
    seen = set()
    for (k, p64), p_auto, p_direct in zip(ref.actor_critic.named_parameters(), auto.actor_critic.parameters(), direct.actor_critic.parameters()):
        g64 = p64.grad
        e_auto = float((p_auto.grad.double().cpu() - g64).abs().max())
        e_direct = float((p_direct.grad.double().cpu() - g64).abs().max())
        top = float(g64.abs().max())
        print(f"\n[direct encoder update] {kind} {k}: max |g - g64|  direct {e_direct:.3e}  autograd form {e_auto:.3e}  max |g64| {top:.3e}")
        assert e_direct <= max(4.0 * e_auto, 1e-5 * top), (k, e_direct, e_auto, top)
        assert lo <= p_direct.grad.data_ptr() < hi  # written in place into the flat bucket
        # Adam's first step is lr * g / (|g| + eps): where |g| ~ eps = 1e-8 an error of 1e-9 is a visible fraction of lr
        torch.testing.assert_close(p_direct, p_auto, rtol=0, atol=2 * direct.learning_rate)
        seen.add(k.split(".")[0])
    assert {"actor_encoder", "actor", "critic", "std"} <= seen and ("critic_encoder" in seen) == (kind == "both-encoders")


def test_no_autograd_and_one_host_read(monkeypatch):
    import torch

    from tests.test_hip_ppo_opts_train import count_scalar_reads

    direct = build("actor-encoder-tanh", "cuda:0", torch.float32, 2, 2, fused_encoder_policy=True)
    before = [p.detach().clone() for p in direct.actor_critic.parameters()]
    torch.cuda.synchronize()
    reads = {"tolist": 0}
    tolist = torch.Tensor.tolist

    def refuse(what):
        def f(*a, **k):
            raise AssertionError(f"{what} ran inside the direct encoder update")
        return f

    def counted(self, *a, **k):
        reads["tolist"] += 1
        return tolist(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "backward", refuse("Tensor.backward"))
    monkeypatch.setattr(torch.Tensor, "item", refuse("Tensor.item"))
    monkeypatch.setattr(torch.Tensor, "tolist", counted)
    scalars = count_scalar_reads(monkeypatch)  # float(t), bool(t), int(t): reads that the two above do not see
    out = direct.update()
    monkeypatch.undo()
    assert reads["tolist"] == 1 and scalars == []
    assert all(np.isfinite(v) for v in out[:3]) and direct.storage.step == 0
    assert all(not torch.equal(p, q) and bool(torch.isfinite(p).all()) for p, q in zip(direct.actor_critic.parameters(), before))


def test_construction_refuses_on_the_gpu_what_the_form_does_not_serve():
    from locotouch_amd.rl import PPO
    from locotouch_amd.rl.modules import ActorCritic, ActorCriticEncoder

    def policy(**kw):
        return ActorCriticEncoder(OBS, COBS, kw.pop("act", ACT), **dict(UPDATE_POLICIES["actor-encoder-tanh"], **kw))

    for match, ac, kw in (("FlatAdam", policy(), dict(fused_adam=False)),
                          (r"actor_encoder: .*dims\[2\] must be", policy(actor_encoder_embedding_dim=6), {}),
                          (r"actor_encoder: .*dims\[0\] must be", policy(actor_encoder_hidden_dims=[520, 8]), {}),
                          ("actor_encoder: .*serves ELU", policy(encoder_activation="relu"), {}),
                          ("actor_encoder: .*SELU", policy(encoder_final_activation="selu"), {}),
                          ("ELU stacks", policy(activation="tanh"), {}),
                          ("does not serve the actor", policy(actor_hidden_dims=[520, 16]), {}),
                          ("action width is 17", policy(act=17), {}),
                          ("packed_forward", policy(), dict(packed_forward=False)),
                          ("not an ActorCriticEncoder", ActorCritic(OBS, COBS, ACT), {})):
        with pytest.raises(ValueError, match=r"^fused_encoder_policy: .*" + match):
            PPO(ac, device="cuda:0", fused_encoder_policy=True, **kw)
    assert PPO(policy(), device="cuda:0", fused_encoder_policy=True).fused_encoder_policy


def test_learn_with_the_key_and_a_checkpoint_round_trip(tmp_path, monkeypatch):
    import os

    import torch

    from locotouch_amd.rl import PPO, FusedRollout

    calls = {"rollout": 0, "update": 0}
    rollout, update = FusedRollout.rollout, PPO._direct_encoder_update

    def counted_rollout(self, *a, **k):
        calls["rollout"] += 1
        return rollout(self, *a, **k)

    def counted_update(self, *a, **k):
        calls["update"] += 1
        return update(self, *a, **k)

    monkeypatch.setattr(FusedRollout, "rollout", counted_rollout)
    monkeypatch.setattr(PPO, "_direct_encoder_update", counted_update)
    runner = make_runner(tmp=str(tmp_path))
    before = {k: p.detach().clone() for k, p in runner.alg.actor_critic.named_parameters()}
    runner.learn(2)
    assert calls == {"rollout": 2, "update": 2}
    rec = runner.history[-1]
    assert all(np.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    after = dict(runner.alg.actor_critic.named_parameters())
    assert all(not torch.equal(after[k], before[k]) for k in before if k.startswith("actor_encoder")) and any(k.startswith("actor_encoder") for k in before)
    assert all(bool(torch.isfinite(p).all()) for p in after.values())
    ck = os.path.join(str(tmp_path), "model_1.pt")
    assert os.path.exists(ck)
    twin_runner = make_runner()
    twin_runner.load(ck)
    for (k, p), q in zip(runner.alg.actor_critic.named_parameters(), twin_runner.alg.actor_critic.parameters()):
        assert torch.equal(p, q), k


def test_what_keeps_the_eager_loop():
    import torch

    from locotouch_amd.rl import FusedRollout

    off = make_runner(key=False)
    assert off._make_fused() is None and not off.alg.fused_encoder_policy  # opt-in: off, the class collects in the eager loop as before
    with pytest.raises(ValueError, match="does not serve ActorCriticEncoder"):
        FusedRollout(off.env, off.alg)
    norm = make_runner(empirical_normalization=True)
    assert norm._make_fused() is None
    with pytest.raises(ValueError, match=r"^fused_encoder_policy: empirical_normalization"):
        FusedRollout(norm.env, norm.alg, obs_normalizer=norm.obs_normalizer, critic_obs_normalizer=norm.critic_obs_normalizer, fused_encoder_policy=True)
    # an embedding width lt_encoder_validate refuses: PPO names it with the key; without it the rollout refuses it and the runner keeps the loop
    with pytest.raises(ValueError, match=r"^fused_encoder_policy: actor_encoder: .*dims\[3\] must be"):
        make_runner(policy=dict(actor_encoder_embedding_dim=60))
    odd = make_runner(key=False, policy=dict(actor_encoder_embedding_dim=60))
    with pytest.raises(ValueError, match=r"^fused_encoder_policy: .*dims\[3\] must be"):
        FusedRollout(odd.env, odd.alg, fused_encoder_policy=True)
    wide = make_runner(key=False, policy=dict(actor_hidden_dims=[520, 64]))
    with pytest.raises(ValueError, match=r"^fused_encoder_policy: the actor or the critic stack is outside lt_mlp's limits"):
        FusedRollout(wide.env, wide.alg, fused_encoder_policy=True)
    bf16 = make_runner(key=False)
    st = bf16.alg.storage
    st.observations, st.privileged_observations = st.observations.to(torch.bfloat16), st.privileged_observations.to(torch.bfloat16)
    with pytest.raises(ValueError, match=r"^fused_encoder_policy: bf16 observation rows"):
        FusedRollout(bf16.env, bf16.alg, fused_encoder_policy=True)
