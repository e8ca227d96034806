"""An `ActorCriticRNNEncoder` behind the runner cfg key `fused_rnn_encoder_policy` on the HIP env at 64 envs: four launches per step (the
memories' strided step, the encoder on their output - include/lt_rnn_encoder.h -, the policy + value launch, the env step) and the
cell's finish behind the last.  The storage it fills is checked for SELF-CONSISTENCY against float64 torch on the modules' own
parameters, in the manner of tests/test_hip_gru_recurrent_rollout.py and with its tolerances; `mu` and the values by the rule of
tests/test_hip_encoder_policy.py (at most the larger of twice the eager f32 modules' error and one f32 ulp of the array's magnitude)."""
import os

import numpy as np
import pytest

from .test_hip_encoder_policy import _ulp
from .test_hip_gru_recurrent_rollout import cell64 as gru64
from .test_hip_recurrent_rollout import TOL, TOL_LP, cell64 as lstm64, mlp64

pytestmark = pytest.mark.gpu

TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
T = 4
SMALL = dict(actor_encoder_hidden_dims=[32, 16], actor_encoder_embedding_dim=16, critic_encoder_hidden_dims=[32, 16], critic_encoder_embedding_dim=16,
             encoder_rnn_hidden_size=64)
REFERENCE = dict(actor_encoder_hidden_dims=[256, 128, 64], actor_encoder_embedding_dim=64, critic_encoder_hidden_dims=[256, 128, 64],
                 critic_encoder_embedding_dim=64, encoder_rnn_hidden_size=256)  # the shape of the reference's teacher cfg
CASES = {"gru64": dict(SMALL, encoder_rnn_type="gru"), "lstm64": dict(SMALL, encoder_rnn_type="lstm"), "reference": dict(REFERENCE, encoder_rnn_type="gru")}
POLICY = dict(class_name="ActorCriticRNNEncoder", init_noise_std=1.0, actor_flatten_obs_end_idx=270, actor_encoder_obs_start_idx=270,
              actor_hidden_dims=[128, 64], critic_flatten_obs_end_idx=270, critic_encoder_obs_start_idx=270, critic_hidden_dims=[128, 64],
              encoder_rnn_num_layers=1, encoder_activation="elu", encoder_final_activation="tanh", activation="elu")


def make_runner(case="gru64", n=64, tmp=None, key=True, policy=None, **cfg_over):
    import torch

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    env = make(TASK, num_envs=n, device="cuda:0", seed=3, max_episode_length=3)  # episodes end inside the rollout
    cfg = train_cfg(TASK)
    cfg["policy"] = {**POLICY, **CASES[case], **(policy or {})}
    cfg["num_steps_per_env"] = T
    cfg["algorithm"] = dict(cfg["algorithm"], num_mini_batches=2, num_learning_epochs=2)
    if key:
        cfg["fused_rnn_encoder_policy"] = True
    cfg.update(cfg_over)
    torch.manual_seed(11)
    runner = OnPolicyRunner(env, cfg, log_dir=tmp, device="cuda:0")
    with torch.no_grad():
        ac = runner.alg.actor_critic
        ac.std.copy_(torch.linspace(0.3, 1.4, 12))
        for mem in (ac.memory_a, getattr(ac, "memory_c", None)):  # biases of order 0.3: where they stand in a cell is not a rounding matter
            if mem is not None:
                mem.rnn.bias_hh_l0.copy_(0.3 * torch.randn_like(mem.rnn.bias_hh_l0))
    return runner


def enc64(enc, x):
    import torch

    for m in enc.model:
        if hasattr(m, "weight"):
            x = x @ m.weight.double().t() + m.bias.double()
        elif isinstance(m, torch.nn.ELU):
            x = torch.nn.functional.elu(x)
        else:
            assert isinstance(m, torch.nn.Tanh)
            x = torch.tanh(x)
    return x


def state_of(mem):
    """The module's state tensors as a tuple: (h, c), or (h,)."""
    return mem.hidden_states if isinstance(mem.hidden_states, tuple) else (mem.hidden_states,)


def storage_snapshot(runner):
    st = runner.alg.storage
    keys = ("observations", "privileged_observations", "actions", "mu", "sigma", "rewards", "dones", "values", "actions_log_prob")
    snap = {k: getattr(st, k).clone() for k in keys}
    ac = runner.alg.actor_critic
    for name, saved, mem in (("a", st.saved_hidden_states_a, ac.memory_a), ("c", st.saved_hidden_states_c, ac.memory_c)):
        for j, s in enumerate(saved):
            snap[f"saved_{name}{j}"] = s.clone()
        for j, s in enumerate(state_of(mem)):
            snap[f"state_{name}{j}"] = s.clone()
    return snap


@pytest.mark.parametrize("case", list(CASES))
def test_rollout_storage_is_self_consistent_against_float64(case):
    import torch

    from locotouch_amd.rl import FusedRollout

    n = 64
    runner = make_runner(case)
    ac, alg, env = runner.alg.actor_critic, runner.alg, runner.env
    lstm = CASES[case]["encoder_rnn_type"] == "lstm"
    ns, hid = (2 if lstm else 1), CASES[case]["encoder_rnn_hidden_size"]
    fused = runner._make_fused()
    assert isinstance(fused, FusedRollout) and fused.actor_mlp is not None and fused.encoders is not None
    assert fused.launches_per_step == 4  # the memories' step, the encoders, policy + value, env step
    assert fused.recurrent and fused.gru == (not lstm)
    fused.begin()
    assert all(s.shape == (1, n, hid) and torch.count_nonzero(s) == 0 for m in (ac.memory_a, ac.memory_c) for s in state_of(m))
    rows0, crows0 = env.obs_policy.clone(), env.obs_critic.clone()
    fused.rollout(T)
    torch.cuda.synchronize()
    st = alg.storage
    assert torch.equal(st.observations[0], rows0) and torch.equal(st.privileged_observations[0], crows0)  # the storage keeps the raw rows
    assert st.observations.shape[-1] == 348 and ac.memory_a.rnn.input_size == 78
    dones = st.dones[:, :, 0] != 0
    assert bool(dones[:T - 1].any()), "no episode ended at a step t < T - 1: no reset was carried into a following step"
    assert bool((~dones[:T - 1]).any())
    std = ac.std.detach()
    final = [tuple(s.clone() for s in state_of(m)) for m in (ac.memory_a, ac.memory_c)]  # what `finish` left in the modules
    nets = ((ac.memory_a, ac.actor_encoder, ac.actor, st.observations, st.saved_hidden_states_a, st.mu, "mu"),
            (ac.memory_c, ac.critic_encoder, ac.critic, st.privileged_observations, st.saved_hidden_states_c, st.values, "values"))
    for k, (mem, enc, stack, rows, saved, got, name) in enumerate(nets):
        assert len(saved) == ns and all(s.shape == (T, 1, n, hid) for s in saved)
        assert all(torch.count_nonzero(s[0]) == 0 for s in saved)  # the rollout started from zeros
        err_k = err_e = mag = 0.0
        for t in range(T):
            x = rows[t][:, 270:]
            pre = [s[t, 0] for s in saved]
            new64 = lstm64(mem.rnn, x, *pre) if lstm else (gru64(mem.rnn, x, pre[0]),)
            keep = (~dones[t]).unsqueeze(1)
            for j in range(ns):
                nxt = saved[j][t + 1, 0] if t < T - 1 else final[k][j][0]
                torch.testing.assert_close(nxt.double(), torch.where(keep, new64[j], torch.zeros_like(new64[j])), **TOL)
                assert torch.count_nonzero(nxt[dones[t]]) == 0  # a reset is an exact zero
            want = mlp64(stack, torch.cat([rows[t][:, :270].double(), enc64(enc, new64[0])], dim=1)).detach()
            # the eager f32 modules on the same rows from the same state
            with torch.inference_mode():
                mem.hidden_states = tuple(s[t].clone() for s in saved) if lstm else saved[0][t].clone()
                eager = ac.act_inference(rows[t]) if k == 0 else ac.evaluate(rows[t])
            err_k = max(err_k, float((got[t].double() - want).abs().max()))
            err_e = max(err_e, float((eager.double() - want).abs().max()))
            mag = max(mag, float(want.abs().max()))
        bound = max(2.0 * err_e, _ulp(mag))
        print(f"\n[rnn-encoder rollout {case}] {name}: max |err| vs f64  fused {err_k:.3e}  eager modules {err_e:.3e}  bound {bound:.3e}")
        assert err_k <= bound, (name, err_k, err_e, bound)
        # the modules' state after finish: where(dones[T - 1], 0, raw state of the last step), exactly
        for j in range(ns):
            raw = fused._hc[(T - 1) & 1][k][j][:n]
            assert torch.equal(final[k][j][0], torch.where((~dones[T - 1]).unsqueeze(1), raw, torch.zeros_like(raw)))
    for t in range(T):
        assert torch.equal(st.sigma[t], std.expand(n, 12))
        lp = torch.distributions.Normal(st.mu[t].double(), std.double().expand(n, 12)).log_prob(st.actions[t].double()).sum(-1, keepdim=True)
        torch.testing.assert_close(st.actions_log_prob[t].double(), lp, **TOL_LP)
    # the storage serves the eager update's batches
    raw = next(iter(st.recurrent_mini_batches(2, 1)))
    first = raw[9][0][0] if lstm else raw[9][0]
    assert torch.is_tensor(first) and first.shape[0] == 1 and first.shape[2] == hid
    # one further EAGER step from the state the rollout left
    for m, s in zip((ac.memory_a, ac.memory_c), final):
        m.hidden_states = tuple(x.clone() for x in s) if lstm else s[0].clone()
    with torch.inference_mode():
        ac.act(env.obs_policy)
        value = ac.evaluate(env.obs_critic)
    for mem, enc, stack, rows, s, got in ((ac.memory_a, ac.actor_encoder, ac.actor, env.obs_policy, final[0], ac.action_mean),
                                          (ac.memory_c, ac.critic_encoder, ac.critic, env.obs_critic, final[1], value)):
        pre = [x[0] for x in s]
        h64 = (lstm64(mem.rnn, rows[:, 270:], *pre) if lstm else (gru64(mem.rnn, rows[:, 270:], pre[0]),))[0]
        torch.testing.assert_close(got.double(), mlp64(stack, torch.cat([rows[:, :270].double(), enc64(enc, h64)], dim=1)), **TOL)


@pytest.mark.parametrize("case", ["gru64", "lstm64"])
def test_captured_rollout_replays_to_the_same_storage(case):
    """Two twin runners (same seeds): a warm rollout each, then a second rollout - launched directly on one, captured into a hipGraph
    and replayed on the other - from the same env state, counters and memory state."""
    import torch

    a, b = make_runner(case), make_runner(case)
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


@pytest.mark.parametrize("case", ["gru64", "lstm64"])
def test_learn_iteration_with_the_eager_update(case, tmp_path, monkeypatch):
    import torch

    from locotouch_amd.rl import FusedRollout
    from locotouch_amd.rl.storage import RolloutStorage

    ns = 2 if case == "lstm64" else 1
    calls = {"rollout": 0, "batches": 0}
    rollout, batches = FusedRollout.rollout, RolloutStorage.recurrent_mini_batches

    def counted_rollout(self, *a, **k):
        calls["rollout"] += 1
        return rollout(self, *a, **k)

    def counted_batches(self, *a, **k):
        assert len(self.saved_hidden_states_a) == ns and len(self.saved_hidden_states_c) == ns
        for b in batches(self, *a, **k):
            calls["batches"] += 1
            yield b

    monkeypatch.setattr(FusedRollout, "rollout", counted_rollout)
    monkeypatch.setattr(RolloutStorage, "recurrent_mini_batches", counted_batches)
    runner = make_runner(case, tmp=str(tmp_path))
    before = [p.detach().clone() for p in runner.alg.actor_critic.parameters()]
    runner.learn(1)
    assert calls["rollout"] == 1 and calls["batches"] == 4  # 2 epochs x 2 mini-batches read the slots the kernels filled
    rec = runner.history[-1]
    assert all(np.isfinite(rec[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/entropy"))
    named = list(runner.alg.actor_critic.named_parameters())
    assert all(bool(torch.isfinite(p).all()) for _, p in named)
    for group in ("memory_a.", "actor_encoder.", "memory_c.", "critic_encoder.", "actor.", "critic."):  # the update reaches every part
        assert any(k.startswith(group) and not torch.equal(p, q) for (k, p), q in zip(named, before)), group
    ck = os.path.join(str(tmp_path), "model_0.pt")
    assert os.path.exists(ck)
    twin = make_runner(case)
    twin.load(ck)
    for (k, p), q in zip(named, twin.alg.actor_critic.parameters()):
        assert torch.equal(p, q), k


def test_what_keeps_the_eager_loop_and_what_the_key_refuses():
    import torch

    from locotouch_amd.rl import PPO, ActorCriticRNNEncoder, FusedRollout
    from locotouch_amd.rl.fused import rollout_unsupported

    from .test_hip_recurrent_rollout import make_runner as make_recurrent_runner

    off = make_runner(key=False)
    assert off._make_fused() is None  # opt-in: off, the class collects in the eager loop
    with pytest.raises(ValueError, match="does not serve ActorCriticRNNEncoder without fused_rnn_encoder_policy"):
        FusedRollout(off.env, off.alg)
    assert isinstance(FusedRollout(off.env, off.alg, fused_rnn_encoder_policy=True), FusedRollout)
    key = r"^fused_rnn_encoder_policy: "
    # another policy class
    other = make_recurrent_runner(64, switch=False)
    with pytest.raises(ValueError, match=key + "the policy is a ActorCriticRecurrent, not an ActorCriticRNNEncoder"):
        FusedRollout(other.env, other.alg, fused_rnn_encoder_policy=True)
    # a critic without an encoder
    none = dict(critic_flatten_obs_end_idx=None, critic_encoder_obs_start_idx=None, critic_encoder_hidden_dims=None, critic_encoder_embedding_dim=None)
    with pytest.raises(ValueError, match=key + "the critic has no encoder"):
        make_runner(policy=none)._make_fused()
    # multi-layer memories, a hidden size outside {64, 128, ..., 512}
    with pytest.raises(ValueError, match=key + r"memory_a must be a single-layer.*it has 2 layers"):
        make_runner(policy=dict(encoder_rnn_num_layers=2))._make_fused()
    with pytest.raises(ValueError, match=key + "memory_a: hidden size 96 is not a multiple of 64"):
        make_runner(policy=dict(encoder_rnn_hidden_size=96))._make_fused()
    # a stack outside lt_mlp's limits, use_packed_mlp=False
    with pytest.raises(ValueError, match=key + "the actor or the critic stack is outside lt_mlp's limits"):
        make_runner(policy=dict(actor_hidden_dims=[520, 64]))._make_fused()
    with pytest.raises(ValueError, match=key + r"the actor or the critic stack is outside lt_mlp's limits.*use_packed_mlp is off"):
        FusedRollout(off.env, off.alg, use_packed_mlp=False, fused_rnn_encoder_policy=True)
    # an encoder width lt_rnn_encoder.h refuses
    with pytest.raises(ValueError, match=key + r".*dims\[2\] must be"):
        make_runner(policy=dict(actor_encoder_embedding_dim=12))._make_fused()
    # normalisers
    with pytest.raises(ValueError, match=key + "empirical_normalization"):
        make_runner(empirical_normalization=True)._make_fused()
    # bf16 rows
    bf16 = make_runner(key=False)
    st = bf16.alg.storage
    st.observations, st.privileged_observations = st.observations.to(torch.bfloat16), st.privileged_observations.to(torch.bfloat16)
    with pytest.raises(ValueError, match=key + "bf16 observation rows"):
        FusedRollout(bf16.env, bf16.alg, fused_rnn_encoder_policy=True)
    # I + H > 1248, and a non-CUDA device: the statement of support itself, on a PPO no env stands behind
    kw = dict(POLICY, **CASES["gru64"])
    kw.pop("class_name")
    wide = dict(kw, actor_flatten_obs_end_idx=100, actor_encoder_obs_start_idx=-800, critic_flatten_obs_end_idx=100, critic_encoder_obs_start_idx=-800,
                encoder_rnn_hidden_size=512)
    alg = PPO(ActorCriticRNNEncoder(1300, 1300, 12, **wide), device="cuda:0")
    alg.init_storage(64, T, [1300], [1300], [12])
    assert rollout_unsupported(alg, fused_rnn_encoder_policy=True) == "fused_rnn_encoder_policy: memory_a: input size + hidden size exceeds 1248"
    cpu = PPO(ActorCriticRNNEncoder(348, 348, 12, **kw), device="cpu")
    cpu.init_storage(64, T, [348], [348], [12])
    assert rollout_unsupported(cpu, fused_rnn_encoder_policy=True).startswith("fused_rnn_encoder_policy: the device is 'cpu'")
    # the key with another class is refused where the runner is built
    with pytest.raises(ValueError, match=key + "the policy is a ActorCriticRecurrent"):
        make_recurrent_runner(64, switch=False, fused_rnn_encoder_policy=True)
