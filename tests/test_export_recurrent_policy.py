"""`export_policy_as_jit` for recurrent policies (compat/runtime.py::_PolicyExport): the TorchScript file carries a plain nn.LSTM / nn.GRU
with its state in registered buffers, steps it one row at a time and has an exported `reset()`.  Against the module's own
`act_inference(normalizer(x))` on the CPU: both sides are the same library ops, so `assert_close` with its float32 defaults."""
import pytest
import torch

STEPS, RESET_AT = 6, 3


def make_policy(rnn_type, obs_dim, with_norm, seed):
    from locotouch_amd.rl.modules import ActorCriticRecurrent
    from locotouch_amd.rl.normalizer import EmpiricalNormalization

    torch.manual_seed(seed)
    ac = ActorCriticRecurrent(obs_dim, obs_dim + 3, 12, actor_hidden_dims=(32, 16), critic_hidden_dims=(16,), rnn_type=rnn_type,
                              rnn_hidden_size=64).eval()
    norm = None
    if with_norm:  # non-trivial statistics: columns of different scale and offset, gathered by the module's own update
        norm = EmpiricalNormalization(obs_dim)
        scale = torch.logspace(-2, 2, obs_dim)
        for _ in range(3):
            norm(torch.randn(50, obs_dim) * scale + scale)
        norm.eval()
        assert float((norm._mean.abs() > 1e-3).float().mean()) > 0.9 and float((norm._std - 1).abs().max()) > 1.0
    return ac, norm


@pytest.mark.parametrize("with_norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("obs_dim", [5, 33])
@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_exported_file_reproduces_act_inference_over_a_chain_with_a_reset(tmp_path, rnn_type, obs_dim, with_norm):
    from locotouch_amd.compat.runtime import export_policy_as_jit

    ac, norm = make_policy(rnn_type, obs_dim, with_norm, seed=obs_dim)
    path = export_policy_as_jit(ac, norm, path=str(tmp_path / "exported"), filename="policy.pt")
    assert path == str(tmp_path / "exported" / "policy.pt") and (tmp_path / "exported" / "policy.pt").is_file()
    mod = torch.jit.load(path)
    buffers = dict(mod.named_buffers())
    assert buffers["hidden_state"].shape == (1, 1, 64) and ("cell_state" in buffers) == (rnn_type == "lstm")
    if rnn_type == "lstm":
        assert buffers["cell_state"].shape == (1, 1, 64)
    scale = torch.logspace(-2, 2, obs_dim) if with_norm else torch.ones(obs_dim)
    with torch.no_grad():
        for t in range(STEPS):
            x = torch.randn(1, obs_dim) * scale + (scale if with_norm else 0.0)
            if t == RESET_AT:
                mod.reset()
                ac.reset()
            want = ac.act_inference(norm(x) if norm is not None else x)
            got = mod(x)
            assert got.shape == (1, 12)
            torch.testing.assert_close(got, want)
            if t == RESET_AT - 1:
                assert float(buffers["hidden_state"].abs().max()) > 0.0  # the state is carried in the buffer ...
        h = ac.get_hidden_states()[0]
        torch.testing.assert_close(buffers["hidden_state"], h[0] if rnn_type == "lstm" else h)  # ... and is the module's own


def test_the_exported_module_is_built_from_plain_library_layers():
    from locotouch_amd.compat.runtime import _PolicyExport

    for rnn_type, cls in (("lstm", torch.nn.LSTM), ("gru", torch.nn.GRU)):
        ac, _ = make_policy(rnn_type, 5, False, seed=1)
        mod = _PolicyExport(ac, None)
        assert type(mod.rnn) is cls and all(type(m) is torch.nn.Linear for m in mod.actor if isinstance(m, torch.nn.Linear))
        for k, v in ac.memory_a.rnn.state_dict().items():
            assert torch.equal(mod.rnn.state_dict()[k], v)


def test_feed_forward_export_keeps_its_shape():
    from locotouch_amd.compat.runtime import _PolicyExport
    from locotouch_amd.rl.modules import ActorCritic

    mod = _PolicyExport(ActorCritic(7, 9, 12, actor_hidden_dims=(16,), critic_hidden_dims=(16,)), None)
    assert not hasattr(mod, "rnn") and not dict(mod.named_buffers()) and isinstance(mod.normalizer, torch.nn.Identity)
    x = torch.randn(4, 7)
    torch.testing.assert_close(torch.jit.script(mod.eval())(x), mod.actor(x))
