"""The opt-in key `fused_encoder_policy` on a machine without a GPU: what it needs is refused by name at construction, and with the key
off an `ActorCriticEncoder` updates exactly as it did - the op chain of the reference's PPO, written out here with plain torch."""
import pytest
import torch

from locotouch_amd.rl import PPO
from locotouch_amd.rl.fused import FusedRollout
from locotouch_amd.rl.modules import ActorCriticEncoder
from tests.rl_synth import policy_case


def policy(case=None):
    case = case or policy_case("encoder")
    return ActorCriticEncoder(*case["args"], **case["kwargs"])


def test_ppo_refuses_the_key_on_a_cpu_device():
    with pytest.raises(ValueError, match=r"^fused_encoder_policy: the device is 'cpu': its kernels run on a GPU only"):
        PPO(policy(), device="cpu", fused_encoder_policy=True)
    assert not PPO(policy(), device="cpu").fused_encoder_policy and not PPO(policy(), device="cpu", fused_encoder_policy=False).fused_encoder_policy


def test_ppo_refuses_the_key_with_symmetry_recurrent_keys_and_several_ranks():
    sym = dict(use_data_augmentation=True, data_augmentation_func=lambda obs=None, actions=None, env=None, is_critic=False: (obs, actions))
    with pytest.raises(ValueError, match=r"^fused_encoder_policy: symmetry_cfg is not served"):
        PPO(policy(), device="cpu", fused_encoder_policy=True, symmetry_cfg=sym)
    for key in ("fused_recurrent_update", "direct_recurrent_update", "fused_gru_memories"):
        with pytest.raises(ValueError, match=r"^fused_encoder_policy: the recurrent keys"):
            PPO(policy(), device="cpu", fused_encoder_policy=True, **{key: True})

    class TwoRanks:
        world_size, rank, local_rank = 2, 0, 0

    with pytest.raises(ValueError, match=r"^fused_encoder_policy: dist.world_size is 2"):
        PPO(policy(), device="cpu", fused_encoder_policy=True, dist=TwoRanks())


def test_fused_rollout_refuses_the_key_on_a_cpu_device():
    alg = PPO(policy(), device="cpu")
    case = policy_case("encoder")
    alg.init_storage(case["N"], case["T"], [case["D"]], [case["D"]], [case["A"]])
    with pytest.raises(ValueError, match=r"^fused_encoder_policy: the device is 'cpu': its kernels run on a GPU only"):
        FusedRollout(object(), alg, fused_encoder_policy=True)
    with pytest.raises(TypeError, match="LocoTouchVecEnv"):  # without the key: the refusal it always had
        FusedRollout(object(), alg)


def filled(case, **ppo_kw):
    """A PPO on the CPU whose storage the eager loop filled from the seeded case."""
    torch.manual_seed(case["seed"])
    alg = PPO(policy(case), device="cpu", **case["ppo"], **ppo_kw)
    alg.init_storage(case["N"], case["T"], [case["D"]], [case["D"]], [case["A"]])
    with torch.no_grad():
        for t in range(case["T"]):
            alg.act(case["obs"][t], case["cobs"][t])
            alg.process_env_step(case["rewards"][t].clone(), case["dones"][t], {})
        alg.compute_returns(case["last_cobs"])
    return alg


def test_with_the_key_off_the_update_is_the_op_chain_it_was():
    case = policy_case("encoder")
    alg, twin = filled(case), filled(case, fused_encoder_policy=False)
    ac, cfg = twin.actor_critic, case["ppo"]
    for p, q in zip(alg.actor_critic.parameters(), ac.parameters()):
        assert torch.equal(p, q)
    before = {k: p.detach().clone() for k, p in alg.actor_critic.named_parameters()}
    torch.manual_seed(99)
    got = alg.update()
    # the reference's update (loco_rl/loco_rl/algorithms/ppo.py:216-337) on the twin, op by op
    torch.manual_seed(99)
    opt = torch.optim.Adam(ac.parameters(), lr=cfg["learning_rate"])
    lr, sums, flat, enc_in = cfg["learning_rate"], [0.0, 0.0, 0.0], ac.actor_flatten_obs_dim, ac.actor_encoder_obs_dim
    for b in twin.storage.mini_batches(cfg["num_mini_batches"], cfg["num_learning_epochs"]):
        mean = ac.actor(torch.cat([b.obs[..., :flat], ac.actor_encoder(b.obs[..., -enc_in:])], dim=-1))
        dist = torch.distributions.Normal(mean, ac.std.expand_as(mean))
        log_prob = dist.log_prob(b.actions).sum(dim=-1)
        value = ac.critic(b.critic_obs)
        mu, sigma, entropy = dist.mean, dist.stddev, dist.entropy().sum(dim=-1)
        with torch.inference_mode():
            kl = torch.sum(torch.log(sigma / b.sigma + 1.0e-5) + (torch.square(b.sigma) + torch.square(b.mu - mu)) / (2.0 * torch.square(sigma)) - 0.5, dim=-1)
            kl_mean = float(torch.mean(kl))
        if kl_mean > cfg["desired_kl"] * 2.0:
            lr = max(1e-5, lr / 1.5)
        elif cfg["desired_kl"] / 2.0 > kl_mean > 0.0:
            lr = min(1e-2, lr * 1.5)
        for group in opt.param_groups:
            group["lr"] = lr
        ratio = torch.exp(log_prob - torch.squeeze(b.log_prob))
        a = torch.squeeze(b.advantages)
        surrogate = torch.max(-a * ratio, -a * torch.clamp(ratio, 1.0 - cfg["clip_param"], 1.0 + cfg["clip_param"])).mean()
        clipped = b.values + (value - b.values).clamp(-cfg["clip_param"], cfg["clip_param"])
        value_loss = torch.max((value - b.returns).pow(2), (clipped - b.returns).pow(2)).mean()
        loss = surrogate + cfg["value_loss_coef"] * value_loss - cfg["entropy_coef"] * entropy.mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ac.parameters(), cfg["max_grad_norm"])
        opt.step()
        for k, v in enumerate((value_loss, surrogate, entropy.mean())):
            sums[k] += v.item()
    n = cfg["num_mini_batches"] * cfg["num_learning_epochs"]
    assert got[:3] == tuple(s / n for s in sums) and alg.learning_rate == lr
    for (name, p), q in zip(alg.actor_critic.named_parameters(), ac.parameters()):
        assert torch.equal(p, q), name
        assert not torch.equal(p, before[name]), name  # (the encoder's parameters among them)
    assert any(name.startswith("actor_encoder") for name in before)
