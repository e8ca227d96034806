"""csrc/lt_policy.hip (`lt_policy_step`: the memory step `lt_policy_memory_kernel<Cell>` + the actor launch), its Python front
rl/fused_policy.py::FusedRecurrentPolicy, `OnPolicyRunner.get_inference_policy(fused=True)` and `scripts/play.py --fused_policy`.

What is asked of the kernel:
  * the new state has THE BITS the rollout kernel (`lt_memory_step` / `lt_memory_gru_step`) writes for its actor network on the same
    inputs: playing a checkpoint reproduces the memory state the rollout computed;
  * the actions are `lt_mlp_forward` on that state, nothing more;
  * against a float64 cell the state's largest error is at most TWICE that of the eager f32 composition (`PolicyMemory` in inference
    mode on the GPU) on the same inputs - the rule of tests/test_hip_memory_step.py: the same exact f32 products summed in another
    order - and the actions' error against the float64 network is below 2e-5 * scale, the bound tests/test_hip_parity.py
    ::test_fused_mlp_matches_torch holds the MLP kernel to (scale = max |reference| + 1);
  * the same with the observation normaliser folded in, on statistics of mixed scale.
The measured figures are printed."""
import copy
import functools
import os
import subprocess
import sys
import types

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"

# n, I, H, row stride (None: I).  I below one k block; rows that are not 16-byte aligned (I = 270, 33); a tail tile (n = 17, 37, 80 % 16
# = 0 is the full one); the widest H; and a column slice [3, 36) of rows of 61 floats
SHAPES = [(1, 5, 64, None), (17, 270, 128, None), (37, 33, 512, None), (80, 64, 256, None), (17, 33, 128, 61)]
CELLS = ("lstm", "gru")
STEPS = 4  # dones in front of step t: NULL, all zero, mixed, all one
ACTIONS = 12
ACTION_TOL = 2e-5


def cell64(cell, x, h, c, p):
    """nn.LSTM's (i, f, g, o) / nn.GRU's (r, z, n; b_hn inside r * (...)) cell in float64: (h', c' or None)."""
    import torch

    w_ih, w_hh, b_ih, b_hh = (p[k].double() for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
    if cell == "lstm":
        i, f, g, o = (x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh).chunk(4, dim=1)
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c2), c2
    (ir, iz, i_n), (hr, hz, hn) = (x @ w_ih.t() + b_ih).chunk(3, dim=1), (h @ w_hh.t() + b_hh).chunk(3, dim=1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(i_n + r * hn)
    return (1 - z) * n + z * h, None


@functools.lru_cache(maxsize=None)
def make_case(cell, n, i, h, stride, norm):
    """Weights, STEPS observation batches, the first state, the masks, an actor and (norm) a normaliser of mixed-scale statistics."""
    import torch
    from locotouch_amd.rl.modules import build_mlp
    from locotouch_amd.rl.normalizer import EmpiricalNormalization

    gen = torch.Generator(device="cpu").manual_seed(1000 * n + i + h + (7 if cell == "gru" else 0))
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(DEV)  # noqa: E731
    g, k = (4 if cell == "lstm" else 3), 1.0 / h ** 0.5
    p = dict(cell=cell, n=n, I=i, H=h, w_ih=r(g * h, i, scale=2 * k), w_hh=r(g * h, h, scale=2 * k), b_ih=r(g * h, scale=0.3),
             b_hh=r(g * h, scale=0.3), h0=torch.tanh(r(n, h)), c0=r(n, h), norm=None)
    wide, off = (stride, 3) if stride else (i, 0)
    col = torch.tensor([1e-2, 1.0, 1e3])[torch.arange(i) % 3].to(DEV) if norm else torch.ones(i, device=DEV)
    mean, std = (col * r(i), col * (0.5 + torch.rand(i, generator=gen).to(DEV))) if norm else (torch.zeros(i, device=DEV), col)
    p["x"] = []
    for _ in range(STEPS):
        rows = r(n, wide)
        rows[:, off:off + i] = mean + std * rows[:, off:off + i]
        p["x"].append(rows[:, off:off + i])  # a view: read in place through the row stride
    if norm:
        nz = EmpiricalNormalization(i).to(DEV).eval()
        nz._mean.copy_(mean[None])
        nz._std.copy_(std[None])
        nz._var.copy_(std[None] ** 2)
        p["norm"] = nz
    mixed = (torch.rand(n, generator=gen) < 0.4).to(torch.uint8)
    if n > 1:
        mixed[0], mixed[-1] = 1, 0
    p["dones"] = [d if d is None else d.to(DEV) for d in (None, torch.zeros(n, dtype=torch.uint8), mixed, torch.ones(n, dtype=torch.uint8))]
    torch.manual_seed(5)
    p["actor"] = build_mlp(h, [64, 32], ACTIONS, "elu").to(DEV)
    with torch.no_grad():
        for q in p["actor"].parameters():
            q.mul_(2.0)  # livelier activations than the default init
    return p


def policy_desc(p, mlp):
    from locotouch_amd import _abi

    d = _abi.LtPolicyDesc()
    d.rnn_type = _abi.LT_POLICY_RNN_LSTM if p["cell"] == "lstm" else _abi.LT_POLICY_RNN_GRU
    d.rnn_layers, d.rnn_hidden, d.obs_dim, d.actor = 1, p["H"], p["I"], mlp.desc
    return d


def policy_memory(p):
    from locotouch_amd import _abi

    m = _abi.LtPolicyMemory(p["w_ih"].data_ptr(), p["w_hh"].data_ptr(), p["b_ih"].data_ptr(), p["b_hh"].data_ptr())
    if p["norm"] is not None:
        p["_stats"] = (p["norm"]._mean.reshape(-1).contiguous(), p["norm"]._std.reshape(-1).contiguous())
        m.norm_mean, m.norm_std, m.norm_eps = p["_stats"][0].data_ptr(), p["_stats"][1].data_ptr(), p["norm"].eps
    return m


def policy_step(p, mlp, x, dones, h, c):
    """One lt_policy_step into fresh NaN buffers: (h', c' or None, actions)."""
    import torch
    from locotouch_amd import _abi

    n = x.shape[0]
    lstm = p["cell"] == "lstm"
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    h2, c2, act = nan(n, p["H"]), nan(n, p["H"]) if lstm else None, nan(n, ACTIONS)
    _abi.call("lt_policy_step", policy_desc(p, mlp), policy_memory(p), mlp.packed, x, x.stride(0) if n > 1 else p["I"], dones, h,
              c if lstm else None, h2, c2, n, act, _abi.stream(torch.device(DEV)))
    return h2, c2, act


@functools.lru_cache(maxsize=None)
def policy_chain(cell, n, i, h, stride, norm):
    """STEPS steps of lt_policy_step, free-running from (h0, c0): [(h', c', actions)] per step.  Computed once per case."""
    import torch
    from locotouch_amd.rl.mlp import PackedMLP

    p = make_case(cell, n, i, h, stride, norm)
    mlp = PackedMLP(p["actor"])
    out, state = [], (p["h0"], p["c0"])
    for t in range(STEPS):
        out.append(policy_step(p, mlp, p["x"][t], p["dones"][t], *state))
        state = out[-1][:2]
    torch.cuda.synchronize()
    return out


def rollout_chain(p, xs):
    """The same chain through the ROLLOUT kernel (both networks of its launch get this memory): [(h', c')] of its actor per step."""
    import torch
    from locotouch_amd import _abi

    n, h, lstm = p["n"], p["H"], p["cell"] == "lstm"
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    stream = _abi.stream(torch.device(DEV))
    w = [p[k].data_ptr() for k in ("w_ih", "w_hh", "b_ih", "b_hh")]
    out, src = [], [(p["h0"], p["c0"])] * 2
    for t in range(STEPS):
        x = xs[t].contiguous()
        dst = [(nan(n, h), nan(n, h)) for _ in range(2)]
        saved = [(nan(n, h), nan(n, h)) for _ in range(2)]
        if lstm:
            nets = [_abi.LtMemoryNet(x.data_ptr(), p["I"], *w, s[0].data_ptr(), s[1].data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                                     v[0].data_ptr(), v[1].data_ptr()) for s, d, v in zip(src, dst, saved)]
            _abi.call("lt_memory_step", nets[0], nets[1], p["dones"][t], n, h, stream)
        else:
            nets = [_abi.LtMemoryGruNet(x.data_ptr(), p["I"], *w, s[0].data_ptr(), d[0].data_ptr(), v[0].data_ptr()) for s, d, v in zip(src, dst, saved)]
            _abi.call("lt_memory_gru_step", nets[0], nets[1], p["dones"][t], n, h, stream)
        torch.cuda.synchronize()  # (x and the slots live until the launch is done)
        out.append(dst[0])
        src = dst
    return out


@pytest.fixture(scope="module", autouse=True)
def release_cached_cases():
    """The cases and chains above stay on the device for the tests of this file alone: behind the last one they are dropped and the
    caching allocator's free blocks returned, so that the files that follow start from the memory state they would have without this one."""
    yield
    import gc

    import torch

    make_case.cache_clear()
    policy_chain.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def case_id(v):
    return "x".join(str(e) for e in v if e is not None) if isinstance(v, tuple) else str(v)


# ---- 1, 2: the bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
@pytest.mark.parametrize("cell", CELLS)
def test_state_has_the_bits_of_the_rollout_kernel_and_the_actions_those_of_the_actor_launch(cell, shape):
    import torch
    from locotouch_amd.rl.mlp import PackedMLP

    p = make_case(cell, *shape, False)
    got = policy_chain(cell, *shape, False)
    want = rollout_chain(p, p["x"])
    mlp = PackedMLP(p["actor"])
    for t in range(STEPS):
        h2, c2, act = got[t]
        assert not torch.isnan(h2).any() and not torch.isnan(act).any(), (t, "an element was not written")
        assert torch.equal(h2, want[t][0]), (t, float((h2 - want[t][0]).abs().max()))
        if cell == "lstm":
            assert not torch.isnan(c2).any() and torch.equal(c2, want[t][1]), (t, float((c2 - want[t][1]).abs().max()))
        assert torch.equal(act, mlp(h2)), t  # composition adds nothing


# ---- 3, 4: against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
@pytest.mark.parametrize("cell", CELLS)
def test_step_chain_against_float64_is_as_close_as_the_eager_composition(cell, shape, norm):
    import torch
    from locotouch_amd.rl.modules import PolicyMemory

    n, i, h, _ = shape
    p = make_case(cell, *shape, norm)
    got = policy_chain(cell, *shape, norm)
    mem = PolicyMemory(i, type=cell, num_layers=1, hidden_size=h).to(DEV).eval()
    actor64 = copy.deepcopy(p["actor"]).double()
    with torch.no_grad():
        for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
            getattr(mem.rnn, {"w_ih": "weight_ih_l0", "w_hh": "weight_hh_l0", "b_ih": "bias_ih_l0", "b_hh": "bias_hh_l0"}[name]).copy_(p[name])
        err_kernel = err_eager = err_act = scale = 0.0
        state = (p["h0"], p["c0"])  # the RAW f32 state the kernel's step t reads: the input of every reference below
        for t in range(STEPS):
            d = p["dones"][t]
            keep = torch.ones(n, 1, device=DEV, dtype=torch.bool) if d is None else (d == 0).unsqueeze(1)
            hm, cm = (torch.where(keep, s, torch.zeros_like(s)) for s in state)
            x = p["x"][t]
            nz = p["norm"]
            x64 = x.double() if nz is None else (x.double() - nz._mean.double()) / (nz._std.double() + nz.eps)
            h64, c64 = cell64(cell, x64, hm.double(), cm.double(), p)
            # the eager composition: the torch normaliser in evaluation mode, PolicyMemory in inference mode, f32 on the GPU
            mem.hidden_states = (hm[None].clone(), cm[None].clone()) if cell == "lstm" else hm[None].clone()
            mem((x if nz is None else nz(x)).contiguous())
            he, ce = mem.hidden_states if cell == "lstm" else (mem.hidden_states, None)
            kh, kc, ka = got[t]
            err_kernel = max(err_kernel, float((kh.double() - h64).abs().max()))
            err_eager = max(err_eager, float((he[0].double() - h64).abs().max()))
            if cell == "lstm":
                err_kernel = max(err_kernel, float((kc.double() - c64).abs().max()))
                err_eager = max(err_eager, float((ce[0].double() - c64).abs().max()))
            a64 = actor64(h64)
            err_act = max(err_act, float((ka.double() - a64).abs().max()))
            scale = max(scale, float(a64.abs().max()) + 1.0)
            state = (kh, kc if cell == "lstm" else p["c0"])
    print(f"\nlt_policy_step {cell} n={n} I={i} H={h} stride={shape[3]} norm={norm}: state max |err| vs f64  kernel {err_kernel:.3e}  "
          f"eager composition {err_eager:.3e};  actions {err_act:.3e} (bound {ACTION_TOL * scale:.3e})")
    assert err_eager > 0.0
    assert err_kernel <= 2.0 * err_eager, (err_kernel, err_eager)
    assert err_act < ACTION_TOL * scale, (err_act, scale)


# ---- 5: row independence and repeatability ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS)
def test_a_row_has_the_same_bits_alone_last_of_17_and_on_a_second_run(cell):
    import torch
    from locotouch_amd.rl.mlp import PackedMLP

    shape = (37, 33, 512, None)
    p = make_case(cell, *shape, False)
    mlp = PackedMLP(p["actor"])
    t, r = 2, 20  # the mixed mask; row 20 stands in the second row tile of the 37
    full = policy_step(p, mlp, p["x"][t], p["dones"][t], p["h0"], p["c0"])
    again = policy_step(p, mlp, p["x"][t], p["dones"][t], p["h0"], p["c0"])
    for lo in (r, r - 16):  # alone (n = 1), and last of n = 17
        part = policy_step(p, mlp, p["x"][t][lo:r + 1], p["dones"][t][lo:r + 1], p["h0"][lo:r + 1], p["c0"][lo:r + 1])
        torch.cuda.synchronize()
        for a, b, c in zip(full, part, again):
            if a is not None:
                assert torch.equal(a[r], b[-1]), lo
                assert torch.equal(a, c)
    for a, b in zip(policy_chain.__wrapped__(cell, *shape, False), policy_chain(cell, *shape, False)):  # the whole chain, run again
        assert all(x is None or torch.equal(x, y) for x, y in zip(a, b))


# ---- 6: the front -----------------------------------------------------------------------------------------------------------------------
def make_module(cell, obs_dim=33, hidden=64, layers=1):
    import torch
    from locotouch_amd.rl.modules import ActorCriticRecurrent

    torch.manual_seed(3)
    return ActorCriticRecurrent(obs_dim, obs_dim + 7, ACTIONS, actor_hidden_dims=[64, 32], critic_hidden_dims=[32], rnn_type=cell,
                                rnn_hidden_size=hidden, rnn_num_layers=layers).to(DEV).eval()


def states(hs, cell):
    return list(hs) if cell == "lstm" else [hs]


@pytest.mark.parametrize("cell, with_norm", [("lstm", True), ("gru", False), ("gru", True)])
def test_front_follows_act_inference_through_masks_and_resets(cell, with_norm):
    import torch
    from locotouch_amd.rl.fused_policy import FusedRecurrentPolicy
    from locotouch_amd.rl.normalizer import EmpiricalNormalization

    n, i = 37, 33
    ac = make_module(cell, i)
    gen = torch.Generator(device="cpu").manual_seed(21)
    nz = None
    if with_norm:
        nz = EmpiricalNormalization(i).to(DEV)
        for _ in range(3):
            nz(torch.randn(64, i, generator=gen).to(DEV) * 3.0 + 1.5)
        nz.eval()
    ac64 = copy.deepcopy(ac).cpu().double()
    nz64 = copy.deepcopy(nz).cpu().double() if nz is not None else (lambda x: x)
    fused = FusedRecurrentPolicy.for_actor_critic(ac, nz)
    assert fused.launches == 2 and fused.eval() is fused and fused.train() is fused and fused.get_hidden_states() is None
    mask = lambda: torch.rand(n, generator=gen) < 0.3  # noqa: E731
    events = {2: [mask()], 5: [mask()], 6: [None], 8: [mask(), mask()], 10: [mask()]}  # in front of step t; 8: two masks, no step between
    err_fused = err_eager = 0.0

    def compare_states():
        nonlocal err_fused, err_eager
        hf, he, h64 = (states(x, cell) for x in (fused.get_hidden_states(), ac.get_hidden_states()[0], ac64.get_hidden_states()[0]))
        for f, e, w in zip(hf, he, h64):
            assert f.shape == e.shape == (1, n, 64)
            err_fused = max(err_fused, float((f.double().cpu() - w).abs().max()))
            err_eager = max(err_eager, float((e.double().cpu() - w).abs().max()))

    with torch.no_grad():
        for t in range(12):
            for m in events.get(t, []):
                for pol in (fused, ac, ac64):
                    pol.reset(None if m is None else (m.to(DEV) if pol is not ac64 else m))
                if m is None:
                    assert fused.get_hidden_states() is None and float(ac.get_hidden_states()[0][0].abs().max()) == 0.0
                else:
                    compare_states()  # with the reset pending in the front, applied in the module
                    hf = states(fused.get_hidden_states(), cell)[0][0]
                    assert float(hf[m.to(DEV)].abs().max()) == 0.0 and float(hf[~m.to(DEV)].abs().max()) > 0.0
            obs = torch.randn(n, i, generator=gen) * 3.0 + 1.5 if with_norm else torch.randn(n, i, generator=gen)
            a_f = fused(obs.to(DEV))
            a_e = ac.act_inference(nz(obs.to(DEV)) if nz is not None else obs.to(DEV))
            ac64.act_inference(nz64(obs.double()))
            assert a_f.shape == (n, ACTIONS)
            scale = float(a_e.abs().max()) + 1.0
            assert float((a_f - a_e).abs().max()) < ACTION_TOL * scale, t
            compare_states()
    print(f"\nFusedRecurrentPolicy {cell} norm={with_norm}: state max |err| vs f64  fused {err_fused:.3e}  eager {err_eager:.3e}")
    assert err_eager > 0.0 and err_fused <= 2.0 * err_eager, (err_fused, err_eager)


def test_front_refuses_what_is_not_served_and_refresh_picks_up_new_parameters():
    import torch
    from locotouch_amd.rl.fused_policy import FusedRecurrentPolicy
    from locotouch_amd.rl.modules import ActorCritic
    from locotouch_amd.rl.normalizer import EmpiricalNormalization

    with pytest.raises(ValueError, match="rnn_layers must be"):
        FusedRecurrentPolicy.for_actor_critic(make_module("lstm", layers=2))
    with pytest.raises(ValueError, match="rnn_hidden must be"):
        FusedRecurrentPolicy.for_actor_critic(make_module("gru", hidden=96))
    with pytest.raises(ValueError, match="obs_dim must be"):
        FusedRecurrentPolicy.for_actor_critic(make_module("gru", obs_dim=1249 - 64))
    with pytest.raises(ValueError, match="actor_critic must be a plain ActorCriticRecurrent"):
        FusedRecurrentPolicy.for_actor_critic(ActorCritic(33, 40, ACTIONS, actor_hidden_dims=[64], critic_hidden_dims=[32]).to(DEV))
    n, i = 5, 33
    ac, nz = make_module("lstm", i), EmpiricalNormalization(i).to(DEV).eval()
    fused = FusedRecurrentPolicy.for_actor_critic(ac, nz)
    obs = torch.randn(n, i, device=DEV)
    with torch.no_grad():
        before = fused(obs)
        for q in ac.parameters():
            q.add_(0.02)  # the memory's parameters are read in place, the actor is packed
        nz._mean.add_(0.3)
        nz._std.mul_(1.7)
        fused.reset()
        stale = fused(obs)
        fused.refresh()
        fused.reset()
        ac.reset()
        fresh, want = fused(obs), ac.act_inference(nz(obs))
    scale = float(want.abs().max()) + 1.0
    assert float((fresh - want).abs().max()) < ACTION_TOL * scale
    assert float((stale - want).abs().max()) > 100 * ACTION_TOL * scale and float((before - want).abs().max()) > 100 * ACTION_TOL * scale
    with pytest.raises(ValueError, match="unit column stride"):
        fused(torch.randn(i, n, device=DEV).t())
    with pytest.raises(TypeError):
        fused(obs.double())


# ---- 7, 8: runner and play ---------------------------------------------------------------------------------------------------------------
def make_runner(cell, with_norm, n=37):
    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    env = make(TASK, num_envs=n, device=DEV, seed=3, max_episode_length=6)  # episodes end inside the 20 steps
    cfg = train_cfg(TASK)
    cfg["policy"] = dict(class_name="ActorCriticRecurrent", init_noise_std=1.0, actor_hidden_dims=[128, 64], critic_hidden_dims=[128, 64],
                         activation="elu", rnn_type=cell, rnn_hidden_size=64, rnn_num_layers=1)
    cfg["empirical_normalization"] = with_norm
    torch.manual_seed(11)
    runner = OnPolicyRunner(env, cfg, log_dir=None, device=DEV)
    if with_norm:  # statistics of a few env steps under random actions
        runner.train_mode()
        with torch.no_grad():
            obs, _ = env.get_observations()
            for _ in range(4):
                runner.obs_normalizer(obs)
                obs = env.step(torch.randn(n, env.num_actions, device=DEV))[0]
    return runner, cfg


@pytest.mark.parametrize("cell, with_norm", [("lstm", False), ("gru", True)])
def test_runner_serves_the_front_on_request_and_the_eager_policy_otherwise(cell, with_norm):
    import torch
    from locotouch_amd.rl.fused_policy import FusedRecurrentPolicy

    runner, _ = make_runner(cell, with_norm)
    ac, env = runner.alg.actor_critic, runner.env
    eager = runner.get_inference_policy(device=DEV)
    if with_norm:  # what it returned before: the lambda around the normaliser ...
        assert type(eager) is types.FunctionType and eager.__name__ == "<lambda>"
    else:          # ... or the module's own bound method
        assert eager.__self__ is ac and eager.__func__ is type(ac).act_inference
    assert type(runner.get_inference_policy()) is type(eager)
    fused = runner.get_inference_policy(device=DEV, fused=True)
    assert isinstance(fused, FusedRecurrentPolicy) and fused.actor_critic is ac
    assert fused.normalizer is (runner.obs_normalizer if with_norm else None)
    ac.reset()
    finished = 0
    with torch.inference_mode():
        obs, _ = env.get_observations()
        for t in range(20):
            a_e, a_f = eager(obs), fused(obs)
            scale = float(a_e.abs().max()) + 1.0
            assert float((a_f - a_e).abs().max()) < ACTION_TOL * scale, t
            obs, _, dones, _ = env.step(a_e)
            finished += int((dones != 0).sum())
            ac.reset(dones)
            fused.reset(dones)
    assert finished > 0  # the masks were exercised


def test_play_script_serves_and_exports_a_recurrent_checkpoint(tmp_path):
    """scripts/play.py --fused_policy --export on a saved recurrent checkpoint, in a fresh child process."""
    import torch
    from locotouch_amd.scripts.train import dump_params

    runner, cfg = make_runner("gru", True)
    run = tmp_path / "run"
    run.mkdir()
    runner.save(str(run / "model_0.pt"))
    dump_params(str(run), {}, cfg)
    del runner
    cmd = [sys.executable, "-m", "locotouch_amd.scripts.play", "--task", TASK, "--num_envs", "37", "--device", DEV, "--fused_policy", "--export",
           "--steps", "20", "--checkpoint", str(run / "model_0.pt")]
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "[play] step 20:" in r.stdout and "Exported policy to" in r.stdout, r.stdout[-2000:]
    mod = torch.jit.load(str(run / "exported" / "policy.pt"))
    assert dict(mod.named_buffers())["hidden_state"].shape == (1, 1, 64)
    out = mod(torch.zeros(1, runner_obs_dim(cfg, run)))
    assert out.shape == (1, ACTIONS) and bool(torch.isfinite(out).all())
    mod.reset()


def runner_obs_dim(cfg, run):
    import torch

    sd = torch.load(str(run / "model_0.pt"), map_location="cpu", weights_only=True)["model_state_dict"]
    return sd["memory_a.rnn.weight_ih_l0"].shape[1]
