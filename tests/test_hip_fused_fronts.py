"""`FusedRollout` across its kinds of policy (rl/fused.py: one front per kind) at 64 envs, 8 steps, [128, 64] stacks: the policy + value
launch alone repeats the bits of the step that ran last for every kind, and the runner and the constructor refuse the same cases in the
words of the one support function."""
import pytest

from .test_hip_encoder_policy import make_runner as make_encoder_runner
from .test_hip_gru_recurrent_rollout import make_runner as make_gru_runner
from .test_hip_recurrent_rollout import TASK, T
from .test_hip_recurrent_rollout import make_runner as make_lstm_runner

pytestmark = pytest.mark.gpu

N = 64


def make_plain_runner(**cfg_over):
    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    env = make(TASK, num_envs=N, device="cuda:0", seed=3, max_episode_length=3)
    cfg = train_cfg(TASK)
    cfg["policy"] = dict(class_name="ActorCritic", init_noise_std=1.0, actor_hidden_dims=[128, 64], critic_hidden_dims=[128, 64], activation="elu")
    cfg["num_steps_per_env"] = T
    cfg.update(cfg_over)
    torch.manual_seed(11)
    return OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")


RUNNERS = {"plain": make_plain_runner, "normalisers": lambda: make_plain_runner(empirical_normalization=True), "lstm": lambda: make_lstm_runner(N),
           "gru": lambda: make_gru_runner(N), "encoder": lambda: make_encoder_runner(N, num_steps_per_env=T)}


@pytest.mark.parametrize("kind", list(RUNNERS))
def test_policy_value_launch_repeats_the_last_step_bit_for_bit(kind):
    """begin(); rollout(T); then `policy_value_launch(T - 1)`: mu, values and actions of slot T - 1 come out bit-equal.  The launch does
    not advance the Philox counter (include/lt_env.h: key = *step_counter + step_offset) and reads the same packed weights, so with the
    same rows the bits must repeat.  The same rows: the slot's (plain), or the ones the front's launch of step T - 1 left (memory:
    the h buffers, encoder: its output rows).  A normaliser front's rows are by then those of the slot BEHIND step T - 1 (the launch
    behind the env step wrote them), so this case first puts back the rows step T - 1 read: (raw slot - mean) * inv through snapshot
    T - 1, in f32 - bit for bit what lt_obs_norm_update writes (tests/test_hip_obs_norm.py::test_rollout_semantics holds
    `last_critic_obs` to exactly this expression)."""
    import torch

    runner = RUNNERS[kind]()
    fused, st = runner._make_fused(), runner.alg.storage
    assert fused is not None and fused.actor_mlp is not None and fused.launches_per_step == {"plain": 2, "normalisers": 4}.get(kind, 3)
    fused.begin()
    fused.rollout(T)
    want = [x[T - 1].clone() for x in (st.mu, st.values, st.actions)]
    if kind == "normalisers":
        for w, rows in enumerate((st.observations, st.privileged_observations)):
            snap = fused.snapshots(w)[T - 1]
            fused.norm_rows[w].copy_((rows[T - 1] - snap[0]) * snap[1])
    for x in (st.mu, st.values, st.actions):
        x[T - 1].zero_()
    fused.policy_value_launch(T - 1)
    torch.cuda.synchronize()
    for name, w, got in zip(("mu", "values", "actions"), want, (st.mu, st.values, st.actions)):
        assert bool(w.abs().sum() > 0) and torch.equal(got[T - 1], w), (kind, name)


def _lstm_with_normalisation():
    r = make_lstm_runner(N, empirical_normalization=True)
    return r, dict(obs_normalizer=r.obs_normalizer, critic_obs_normalizer=r.critic_obs_normalizer)


def _gru_without_its_key():
    return make_gru_runner(N, key=False), {}


def _encoder_without_its_key():
    return make_encoder_runner(N, key=False), {}


def _encoder_with_normalisation():
    r = make_encoder_runner(N, empirical_normalization=True)
    return r, dict(obs_normalizer=r.obs_normalizer, critic_obs_normalizer=r.critic_obs_normalizer, fused_encoder_policy=True)


def _bf16_rows_with_normalisation():
    import torch

    r = make_plain_runner(empirical_normalization=True)
    d = r.env.num_obs
    r.alg.init_storage(N, T, [d], [d], [12], obs_dtype=torch.bfloat16)
    return r, dict(obs_normalizer=r.obs_normalizer, critic_obs_normalizer=r.critic_obs_normalizer)


@pytest.mark.parametrize("case", [_lstm_with_normalisation, _gru_without_its_key, _encoder_without_its_key, _encoder_with_normalisation,
                                  _bf16_rows_with_normalisation], ids=lambda f: f.__name__.strip("_"))
def test_runner_and_rollout_refuse_the_same_cases(case):
    from locotouch_amd.rl import FusedRollout
    from locotouch_amd.rl.fused import rollout_unsupported

    runner, kw = case()
    why = rollout_unsupported(runner.alg, **kw)
    assert isinstance(why, str) and why
    assert runner._make_fused() is None
    with pytest.raises(ValueError) as e:
        FusedRollout(runner.env, runner.alg, **kw)
    assert str(e.value).endswith(why), (str(e.value), why)


@pytest.mark.parametrize("both", [True, False], ids=["both_normalisers", "one_normaliser"])
def test_bf16_rows_off_the_packed_path_are_refused_before_the_normalisers(both):
    """Two refusals could fire: bf16 rows need the packed MLP path, and normalisers are not served on bf16 rows (or: one normaliser alone).
    The first is the one that fires, as it always did; the support function, which knows no env, names the second."""
    from locotouch_amd.rl import FusedRollout
    from locotouch_amd.rl.fused import rollout_unsupported

    runner, kw = _bf16_rows_with_normalisation()
    if not both:
        del kw["critic_obs_normalizer"]
    assert "bf16" in rollout_unsupported(runner.alg, **kw) if both else "both" in rollout_unsupported(runner.alg, **kw)
    with pytest.raises(ValueError, match="^bf16 observation rows need the packed MLP path"):
        FusedRollout(runner.env, runner.alg, use_packed_mlp=False, **kw)
