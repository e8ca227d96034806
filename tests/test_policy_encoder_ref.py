"""tests/policy_encoder_ref.py, the float64 oracle of include/lt_policy_encoder.h, held to the modules it restates: in double, on the
CPU, `ActorCriticRNNEncoder.act_inference` and `ActorCriticEncoder.act_inference` behind an `EmpiricalNormalization` in evaluation
mode, over four steps with `reset(dones)` between them - NULL, all zero, mixed, all one, the masks of the GPU test."""
import pytest
import torch

from locotouch_amd.rl.modules import ActorCriticEncoder, ActorCriticRNNEncoder
from locotouch_amd.rl.normalizer import EmpiricalNormalization
from tests.policy_encoder_ref import operands_of, policy_encoder_ref

N, OBS, FLAT, TAIL, ACTIONS, H = 9, 40, 6, 33, 5, 64
TOL = 1e-12  # the same float64 arithmetic, grouped by torch's kernels in another way


def _module(form, final):
    torch.manual_seed(17)
    kw = dict(actor_flatten_obs_end_idx=FLAT, actor_encoder_obs_start_idx=-TAIL, actor_encoder_hidden_dims=[24, 16], actor_encoder_embedding_dim=8,
              actor_hidden_dims=[32, 16], critic_flatten_obs_end_idx=FLAT, critic_encoder_obs_start_idx=-TAIL, critic_encoder_hidden_dims=[16],
              critic_encoder_embedding_dim=8, critic_hidden_dims=[16], encoder_final_activation=final)
    if form == "plain":
        return ActorCriticEncoder(OBS, OBS, ACTIONS, **kw).double().eval()
    return ActorCriticRNNEncoder(OBS, OBS, ACTIONS, encoder_rnn_type=form, encoder_rnn_hidden_size=H, **kw).double().eval()


def _normalizer(gen):
    nz = EmpiricalNormalization(OBS).double()
    for _ in range(3):
        nz(torch.randn(64, OBS, generator=gen, dtype=torch.float64) * 3.0 + 1.5)
    return nz.eval()


@pytest.mark.parametrize("with_norm", [False, True], ids=["plain-rows", "normalised"])
@pytest.mark.parametrize("form, final", [("lstm", None), ("gru", "tanh"), ("plain", "tanh"), ("plain", None)])
def test_restatement_follows_act_inference_over_four_steps_with_resets(form, final, with_norm):
    gen = torch.Generator().manual_seed(5)
    ac = _module(form, final)
    nz = _normalizer(gen) if with_norm else None
    encoder, actor, memory = operands_of(ac)
    assert (memory is None) == (form == "plain") and encoder[3] == final and len(encoder[0]) == 3 and len(actor[0]) == 3
    norm = (nz._mean, nz._std, nz.eps) if with_norm else None
    mixed = torch.rand(N, generator=gen) < 0.4
    mixed[0], mixed[-1] = True, False
    masks = [None, torch.zeros(N, dtype=torch.bool), mixed, torch.ones(N, dtype=torch.bool)]
    state = (torch.zeros(N, H, dtype=torch.float64), torch.zeros(N, H, dtype=torch.float64))
    with torch.no_grad():
        for t, done in enumerate(masks):
            obs = torch.randn(N, OBS, generator=gen, dtype=torch.float64) * (3.0 if with_norm else 1.0) + (1.5 if with_norm else 0.0)
            if done is not None:
                ac.reset(done)
            want = ac.act_inference(nz(obs) if with_norm else obs)
            got = policy_encoder_ref(obs, FLAT, TAIL, encoder, actor, memory, state if memory else None, done, norm)
            assert got["actions"].shape == (N, ACTIONS) and got["embedding"].shape == (N, 8)
            assert float((got["actions"] - want).abs().max()) < TOL, t
            if memory is not None:
                hs = ac.get_hidden_states()[0]
                hs = hs if form == "lstm" else (hs,)
                assert float((got["h"] - hs[0][0]).abs().max()) < TOL, t
                if form == "lstm":
                    assert float((got["c"] - hs[1][0]).abs().max()) < TOL, t
                else:
                    assert got["c"] is None
                if done is not None and bool(done.all()):  # every row restarted: the state behind the step does not depend on the one before
                    fresh = policy_encoder_ref(obs, FLAT, TAIL, encoder, actor, memory, (torch.zeros(N, H), torch.zeros(N, H)), None, norm)
                    assert torch.equal(fresh["h"], got["h"])
                state = (got["h"], got["c"] if form == "lstm" else state[1])
            else:
                assert got["h"] is None and got["c"] is None
                ac.reset(done)  # a no-op of the plain class


def test_the_head_is_normalised_with_the_heads_statistics_and_the_tail_with_the_tails():
    """Planted statistics: a restatement that normalised the tail with the head's columns (or not at all) would differ."""
    gen = torch.Generator().manual_seed(9)
    ac = _module("plain", None)
    encoder, actor, _ = operands_of(ac)
    mean, std = torch.arange(OBS, dtype=torch.float64) * 0.25, 0.5 + torch.arange(OBS, dtype=torch.float64) * 0.125
    obs = torch.randn(N, OBS, generator=gen, dtype=torch.float64) * 4.0
    with torch.no_grad():
        want = ac.act_inference((obs - mean) / (std + 1e-2))
        got = policy_encoder_ref(obs, FLAT, TAIL, encoder, actor, norm=(mean, std, 1e-2))
        plain = policy_encoder_ref(obs, FLAT, TAIL, encoder, actor)
    assert float((got["actions"] - want).abs().max()) < TOL
    assert float((plain["actions"] - want).abs().max()) > 1e-3
