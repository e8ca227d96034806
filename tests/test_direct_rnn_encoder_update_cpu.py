"""The PPO key `direct_rnn_encoder_update` where no GPU is needed: what it refuses at construction (each a ValueError that starts with
the key's name), the runner's forwarding, the binding of include/lt_rnn_encoder_train.h, and the float64 statement of the encoder's
backward pass (tests/rnn_encoder_backward_ref.py) - held to autograd on an `MLP` of rl/models.py for every pair of activations, and
shown to reject each of its planted mutations.  CPU only."""
import ctypes

import pytest
import torch

from locotouch_amd import _abi
from locotouch_amd.rl import PPO, ActorCritic, ActorCriticEncoder, ActorCriticRecurrent, ActorCriticRNNEncoder, OnPolicyRunner
from locotouch_amd.rl.models import MLP
from tests import rnn_encoder_backward_ref as R
from tests.rnn_encoder_synth import rnn_encoder_case

KEY = r"^direct_rnn_encoder_update: "


# ---- refusals and forwarding ----
def test_the_key_is_refused_on_the_cpu():
    case = rnn_encoder_case("gru")
    with pytest.raises(ValueError, match=KEY + "the device is 'cpu'"):
        PPO(ActorCriticRNNEncoder(*case["args"], **case["kwargs"]), device="cpu", direct_rnn_encoder_update=True)
    off = PPO(ActorCriticRNNEncoder(*case["args"], **case["kwargs"]), device="cpu")
    assert off.direct_rnn_encoder_update is False  # default off


OTHERS = {"ActorCritic": lambda: ActorCritic(14, 14, 4, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16]),
          "ActorCriticRecurrent": lambda: ActorCriticRecurrent(14, 14, 4, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_hidden_size=64),
          "ActorCriticEncoder": lambda: ActorCriticEncoder(14, 14, 4, 9, -5, [16, 8], 8, [32, 16], critic_hidden_dims=[32, 16])}


@pytest.mark.parametrize("name", list(OTHERS))
def test_the_key_is_refused_for_the_three_other_classes(name):
    with pytest.raises(ValueError, match=KEY + f"the policy is a {name}, not an ActorCriticRNNEncoder"):
        PPO(OTHERS[name](), device="cpu", direct_rnn_encoder_update=True)


def test_the_key_is_refused_for_a_critic_without_an_encoder():
    case = rnn_encoder_case("gru")
    kw = dict(case["kwargs"], critic_flatten_obs_end_idx=None, critic_encoder_obs_start_idx=None, critic_encoder_hidden_dims=None,
              critic_encoder_embedding_dim=None)
    with pytest.raises(ValueError, match=KEY + "the critic has no encoder"):
        PPO(ActorCriticRNNEncoder(*case["args"], **kw), device="cpu", direct_rnn_encoder_update=True)


def test_more_than_one_rank_is_refused_before_anything_is_broadcast():
    class TwoRanks:
        world_size, rank, local_rank = 2, 0, 0

    case = rnn_encoder_case("lstm")
    with pytest.raises(ValueError, match=KEY + "dist.world_size is 2"):
        PPO(ActorCriticRNNEncoder(*case["args"], **case["kwargs"]), device="cpu", dist=TwoRanks(), direct_rnn_encoder_update=True)


def test_the_runner_forwards_the_key_and_names_another_class():
    from tests.distill_synth import ScriptedEnv
    from tests.test_rnn_encoder_policy_cpu import runner_cfg

    env = ScriptedEnv(6, form="tuple")
    with pytest.raises(ValueError, match=KEY + "the device is 'cpu'"):  # PPO's refusal: the key reached it
        OnPolicyRunner(env, runner_cfg(env, direct_rnn_encoder_update=True), log_dir=None, device="cpu")
    r = OnPolicyRunner(env, runner_cfg(env, direct_rnn_encoder_update=False), log_dir=None, device="cpu")
    assert r.alg.direct_rnn_encoder_update is False and r.alg_cfg["direct_rnn_encoder_update"] is False
    cfg = runner_cfg(env, direct_rnn_encoder_update=True)
    cfg["policy"] = dict(class_name="ActorCritic", actor_hidden_dims=[32], critic_hidden_dims=[32], activation="elu", init_noise_std=1.0)
    with pytest.raises(ValueError, match=KEY + "the policy is a ActorCritic, not an ActorCriticRNNEncoder"):
        OnPolicyRunner(env, cfg, log_dir=None, device="cpu")


def test_train_script_has_the_flag():
    import inspect

    from locotouch_amd.scripts import train

    src = inspect.getsource(train)
    assert '"--direct_rnn_encoder_update"' in src and 'cfg["direct_rnn_encoder_update"] = True' in src


# ---- the header ----
def test_header_is_bound_by_one_row_and_refuses_on_the_host():
    rows = [r for r in _abi.HEADERS if r[1] == "lt_rnn_encoder_train.h"]
    assert len(rows) == 1 and rows[0][0] == "RNN_ENCODER_TRAIN"
    assert set(_abi.RNN_ENCODER_TRAIN_SIGNATURES) == {"lt_rnn_encoder_forward_train", "lt_rnn_encoder_backward", "lt_rnn_encoder_backward_launches"}
    assert _abi.RNN_ENCODER_TRAIN_VALUE_QUERIES == {"lt_rnn_encoder_backward_launches"}
    assert _abi.CONSTS["LT_ABI_VERSION"] == 21
    net_p, grad_p = ctypes.POINTER(_abi.LtRnnEncoderNet), ctypes.POINTER(_abi.LtRnnEncoderGrad)  # the net is lt_rnn_encoder.h's own structure
    assert _abi.RNN_ENCODER_TRAIN_SIGNATURES["lt_rnn_encoder_forward_train"] == (ctypes.c_int, [net_p, net_p, ctypes.c_int, ctypes.c_void_p])
    assert _abi.RNN_ENCODER_TRAIN_SIGNATURES["lt_rnn_encoder_backward"] == (ctypes.c_int, [grad_p, grad_p, ctypes.c_int, ctypes.c_void_p])
    assert _abi.RNN_ENCODER_TRAIN_CONSTS["LT_RNN_ENCODER_TRAIN_MAX_LAYERS"] == _abi.RNN_ENCODER_CONSTS["LT_RNN_ENCODER_MAX_LAYERS"]
    lib = _abi.load()
    g = _abi.LtRnnEncoderGrad()
    g.flat_dim, g.enc_in, g.num_layers, g.activation, g.final_activation = 270, 256, 2, _abi.CONSTS["LT_ACT_ELU"], _abi.CONSTS["LT_ACT_TANH"]
    g.dims[0], g.dims[1] = 64, 64
    assert lib.lt_rnn_encoder_backward_launches(ctypes.byref(g), None) == 1
    assert lib.lt_rnn_encoder_backward_launches(ctypes.byref(g), ctypes.byref(g)) == 1
    g.dims[1] = 12
    assert lib.lt_rnn_encoder_backward_launches(ctypes.byref(g), None) == _abi.CONSTS["LT_EINVAL"]
    msg = lib.lt_last_error().decode()
    assert msg.startswith("lt_rnn_encoder_backward_launches: invalid argument: actor.dims[1] must be"), msg
    with pytest.raises(RuntimeError, match=r"lt_rnn_encoder_backward: invalid argument: n must be"):
        _abi.call("lt_rnn_encoder_backward", g, None, 0, None)


# ---- the float64 statement against autograd ----
def autograd(case):
    """([dz_l], dh, [dW_l], [db_l]) by autograd through an `MLP` of rl/models.py holding the case's parameters, in float64."""
    ws, bs = case["weights"], case["biases"]
    mlp = MLP(ws[0].shape[1], [w.shape[0] for w in ws[:-1]], ws[-1].shape[0], activation=case["act"], final_layer_activation=case["final"]).double()
    linears = [m for m in mlp.model if hasattr(m, "weight")]
    with torch.no_grad():
        for m, w, b in zip(linears, ws, bs):
            m.weight.copy_(w)
            m.bias.copy_(b)
    h = case["h"].clone().requires_grad_(True)
    x, pres = h, []
    for m in mlp.model:
        x = m(x)
        if hasattr(m, "weight"):
            x.retain_grad()
            pres.append(x)
    (x * case["g"]).sum().backward()
    return [p.grad for p in pres], h.grad, [m.weight.grad for m in linears], [m.bias.grad for m in linears]


def judge(case, mutate=None):
    """The arrays on which the (possibly mutated) statement departs from autograd by more than 1e-9 of the array's magnitude."""
    acts, pre, emb = R.forward(case["weights"], case["biases"], case["h"], case["act"], case["final"])
    dzs, dh = R.backward(case["weights"], acts, pre, emb, case["g"], case["act"], case["final"], mutate=mutate)
    want_dz, want_dh, want_dw, want_db = autograd(case)
    ins = [case["h"], *acts]
    got = {"dh": dh, **{f"dz[{l}]": d for l, d in enumerate(dzs)}, **{f"dW[{l}]": d.t() @ x for l, (d, x) in enumerate(zip(dzs, ins))},
           **{f"db[{l}]": d.sum(0) for l, d in enumerate(dzs)}}
    want = {"dh": want_dh, **{f"dz[{l}]": d for l, d in enumerate(want_dz)}, **{f"dW[{l}]": d for l, d in enumerate(want_dw)},
            **{f"db[{l}]": d for l, d in enumerate(want_db)}}
    return sorted(k for k in want if float((got[k] - want[k]).abs().max()) > 1e-9 * max(1.0, float(want[k].abs().max())))


@pytest.mark.parametrize("final", R.FINALS, ids=lambda f: f"final-{f}")
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("enc_in,dims", [(24, [16, 16, 16]), (5, [8]), (64, [24, 8])], ids=["24-16-16-16", "5-8", "64-24-8"])
def test_statement_equals_autograd_on_an_mlp(enc_in, dims, act, final):
    case = R.case(enc_in, dims, act, final, n=19)
    acts, pre, _ = R.forward(case["weights"], case["biases"], case["h"], act, final)
    assert bool((pre > 0).any()) and bool((pre < 0).any())  # both branches of the final activation
    assert all(bool((a > 0).any()) and bool((a < 0).any() if act != "relu" else (a == 0).any()) for a in acts)
    assert judge(case) == []


# mutation -> the (hidden, final) activations on which it bites
MUTANTS = {"elu_derivative_of_relu": ("relu", None), "relu_derivative_of_tanh": ("tanh", None), "tanh_derivative_of_elu": ("elu", None),
           "final_elu_from_emb_where_pre_belongs": ("elu", "elu"), "final_tanh_from_pre_where_emb_belongs": ("elu", "tanh"),
           "weight_transposed": ("elu", "tanh"), "a_layer_dropped": ("elu", "tanh"), "final_activation_skipped": ("elu", "tanh"),
           "dh_from_dz1": ("elu", "tanh"), "hidden_derivative_skipped": ("elu", "tanh")}


def test_every_mutation_has_a_case():
    assert set(MUTANTS) == set(R.MUTATIONS) and len(MUTANTS) >= 8


@pytest.mark.parametrize("mutation", list(MUTANTS))
def test_planted_mutation_is_rejected(mutation):
    act, final = MUTANTS[mutation]
    case = R.case(24, [16, 16, 16], act, final, n=19)  # square layers: a transposed or dropped weight still has a shape that fits
    assert judge(case) == []
    bad = judge(case, mutate=mutation)
    print(f"\n[rnn encoder backward ref] {mutation}: rejected on {bad}")
    assert bad, mutation
    if mutation == "dh_from_dz1":
        assert "dh" in bad and "dz[0]" not in bad
