"""Seeded inputs for tools/gen_golden_rnn_encoder.py / tests/test_rnn_encoder_policy_cpu.py: the rollout data of
tests/rl_synth.py::policy_case("encoder") (14-wide rows, 8 envs x 10 steps, dones inside) with the constructor arguments of an
`ActorCriticRNNEncoder` whose two networks both have an encoder.  `args` / `kwargs` are the same for the reference and this package."""
from tests.rl_synth import policy_case

CELLS = ("gru", "lstm")


def rnn_encoder_case(cell: str):
    """Flatten end 9, encoder start -5: head columns 0-8, the memory reads columns 9-13; hidden size 24; encoders [16, 8] -> 6 + tanh."""
    assert cell in CELLS
    case = dict(policy_case("encoder"))
    case["kwargs"] = dict(actor_flatten_obs_end_idx=9, actor_encoder_obs_start_idx=-5, actor_encoder_hidden_dims=[16, 8],
                          actor_encoder_embedding_dim=6, actor_hidden_dims=[32, 16], critic_flatten_obs_end_idx=9,
                          critic_encoder_obs_start_idx=-5, critic_encoder_hidden_dims=[16, 8], critic_encoder_embedding_dim=6,
                          critic_hidden_dims=[32, 16], encoder_rnn_type=cell, encoder_rnn_hidden_size=24, encoder_rnn_num_layers=1,
                          encoder_activation="elu", encoder_final_activation="tanh", activation="elu", init_noise_std=1.0)
    return case
