"""Which update `PPO.update()` runs (rl/ppo.py `_update_form`): for a policy class, its keys and a storage of 8 envs x 4 steps, the
name of the method the resolution hands back.  No update runs here; the expected names are what the chain of calls that `update()`,
`_eager_update` and `_fused_update` used to make ended in."""
import pytest
import torch

from locotouch_amd.rl import PPO, ActorCritic, ActorCriticEncoder, ActorCriticRecurrent, ActorCriticRNNEncoder
from locotouch_amd.rl.symmetry import mirror_go1
from tests.rl_synth import policy_case
from tests.rnn_encoder_synth import rnn_encoder_case

N, T, D, A = 8, 4, 14, 4
ONE_ROW = dict(normalize_advantage_per_mini_batch=True, num_mini_batches=N * T)  # minibatches of one row: their std is NaN in the reference


def user_mirror(obs=None, actions=None, env=None, is_critic=False):
    """A `data_augmentation_func` that is not this package's `mirror_go1`: [original; negated]."""
    return (None if obs is None else torch.cat((obs, -obs)), None if actions is None else torch.cat((actions, -actions)))


def symmetry(func):
    return dict(use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=0.5, data_augmentation_func=func)


def plain():
    return ActorCritic(D, D, A, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu")


def recurrent():
    return ActorCriticRecurrent(D, D, A, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_type="lstm", rnn_hidden_size=64)


def encoder():
    case = policy_case("encoder")
    return ActorCriticEncoder(*case["args"], **case["kwargs"])


def rnn_encoder():
    case = rnn_encoder_case("gru")
    return ActorCriticRNNEncoder(*case["args"], **case["kwargs"])


def form(ac, device, width=D, **ppo_kw):
    alg = PPO(ac, device=device, **ppo_kw)
    alg.init_storage(N, T, [width], [width], [A])
    return alg._update_form().__name__


@pytest.mark.parametrize("policy, ppo_kw, name", [
    (plain, {}, "_eager_update"),
    (plain, ONE_ROW, "_eager_update"),
    (recurrent, {}, "_eager_update"),
    (recurrent, dict(fused_recurrent_update=True), "_recurrent_update"),
    (plain, dict(symmetry_cfg=symmetry(user_mirror)), "_symmetry_update"),
    (encoder, {}, "_eager_update"),
    (rnn_encoder, {}, "_eager_update"),
], ids=["plain", "plain-one-row", "recurrent", "recurrent-fused_recurrent_update", "plain-symmetry-user-function", "encoder", "rnn-encoder"])
def test_the_form_on_the_cpu(policy, ppo_kw, name):
    assert form(policy(), "cpu", **ppo_kw) == name


def gpu_encoder():
    from tests.test_hip_encoder_policy import ENCODER_POLICY

    return ActorCriticEncoder(348, 348, A, **{k: v for k, v in ENCODER_POLICY.items() if k != "class_name"})


def gpu_rnn_encoder():
    from tests.test_hip_direct_rnn_encoder_update import policy

    return policy("gru", act=A)


@pytest.mark.gpu
@pytest.mark.parametrize("policy, width, ppo_kw, name", [
    (plain, D, {}, "_direct_update"),
    (plain, D, dict(fused_adam=False), "_fused_update"),
    (plain, D, dict(direct_update=False), "_fused_update"),
    (plain, D, dict(fused_loss=False), "_eager_update"),
    (plain, D, ONE_ROW, "_eager_update"),
    (plain, D, dict(symmetry_cfg=symmetry(mirror_go1)), "_direct_update"),
    (plain, D, dict(symmetry_cfg=symmetry(user_mirror)), "_symmetry_update"),
    (recurrent, D, {}, "_eager_update"),
    (gpu_encoder, 348, dict(fused_encoder_policy=True), "_direct_encoder_update"),
    (recurrent, D, dict(fused_recurrent_update=True), "_recurrent_update"),
    (recurrent, D, dict(fused_recurrent_update=True, direct_recurrent_update=True), "_direct_recurrent_update"),
    (gpu_rnn_encoder, 24, dict(direct_rnn_encoder_update=True), "_direct_rnn_encoder_update"),
], ids=["plain", "plain-fused_adam-off", "plain-direct_update-off", "plain-fused_loss-off", "plain-one-row", "symmetry-mirror_go1",
        "symmetry-user-function", "recurrent", "fused_encoder_policy", "fused_recurrent_update", "direct_recurrent_update",
        "direct_rnn_encoder_update"])
def test_the_form_on_the_gpu(policy, width, ppo_kw, name):
    assert form(policy(), "cuda:0", width=width, **ppo_kw) == name
