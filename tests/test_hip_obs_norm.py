"""Observation normalisation on the fused rollout path (csrc/lt_obs_norm.hip, include/lt_obs_norm.h, rl/fused.py, rl/runner.py).

The kernels are pinned to the reference's golden of EmpiricalNormalization (tests/golden/rl_extra.npz `norm_*`), to the recurrence in
float64 and to the torch class they replace; the rollout is pinned to the recurrence rerun on its own raw rows.

Bound of the float64 comparisons (`_assert_ratio`): per column, the kernel's error is at most 2x the error of the torch class in
float32 on the same batches on the GPU (the factor is for a different summation order), with an absolute floor of one f32 ulp of the
column's magnitude, max |x| over all batches - for mean, std and y alike.  A rollout's snapshot stores 1 / (std + eps), not std: the
rule is applied to that number as it is stored, against the same number formed from the torch class's `_std` in f32, with one f32 ulp
of ITS magnitude as the floor (the precision of the format it is kept in; std itself is not kept).
"""
import copy
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
EPS = 1e-2


def _ulp(x):
    """One f32 ulp at magnitude x (float64 array)."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def _rec64(mean, var, count, x, until):
    """One `update` of EmpiricalNormalization (rl/normalizer.py) in float64 on the CPU: (mean, var, count)."""
    if until is not None and count >= until:
        return mean, var, count
    n = x.shape[0]
    count = count + n
    w = n / count
    x = x.double().cpu()
    bm, bv = x.mean(0), x.var(0, unbiased=False)
    shift = bm - mean
    mean2 = mean + w * shift
    return mean2, var + w * (bv - var + shift * (bm - mean2)), count


def _assert_ratio(what, err_k, err_t, floor):
    bound = np.maximum(2.0 * err_t, floor)
    worst = int(np.argmax(err_k - bound))
    print(f"    {what:5s} kernel max {err_k.max():.3e}  torch-f32 max {err_t.max():.3e}  worst column {worst}: "
          f"kernel {err_k[worst]:.3e} torch {err_t[worst]:.3e} floor {floor[worst]:.3e}")
    assert (err_k <= bound).all(), (what, worst, err_k[worst], err_t[worst], floor[worst])


def _mixed_batches(n, d, nb, seed):
    """Columns by index mod 4: N(0,1); constant; mean 1e3 and spread 1e-2; N(0,1) jumping by 10 from batch to batch."""
    import torch

    g = torch.Generator().manual_seed(seed)
    kind = torch.arange(d) % 4
    const = 0.7 * (1.0 + torch.arange(d, dtype=torch.float32))
    for b in range(nb):
        x = torch.randn(n, d, generator=g)
        x = torch.where(kind == 1, const.expand(n, d), x)
        x = torch.where(kind == 2, 1.0e3 + 1.0e-2 * x, x)
        x = torch.where(kind == 3, x + 10.0 * b, x)
        yield x


def _run_mixed(n, d, nb=30, seed=5):
    """Kernel and torch class on the same batches against the f64 recurrence: per-column maxima of the errors, final buffers."""
    import torch
    from locotouch_amd.rl import EmpiricalNormalization
    from locotouch_amd.rl.fused import normalize_rows

    dev = "cuda:0"
    ker, tor = EmpiricalNormalization([d]).to(dev), EmpiricalNormalization([d]).to(dev)
    mean, var, count = torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64), 0
    err = {k: np.zeros(d) for k in ("mean_k", "mean_t", "std_k", "std_t", "y_k", "y_t")}
    xmag, inv_max = np.zeros(d), np.zeros(d)
    for x in _mixed_batches(n, d, nb, seed):
        xg = x.to(dev)
        y_k = normalize_rows(ker, xg)
        with torch.no_grad():
            y_t = tor(xg)
        mean, var, count = _rec64(mean, var, count, x, None)
        std = var.sqrt()
        y64 = (xg.double() - mean.to(dev)) / (std.to(dev) + EPS)
        for tag, nm, y in (("k", ker, y_k), ("t", tor, y_t)):
            err["mean_" + tag] = np.maximum(err["mean_" + tag], (nm._mean[0].double().cpu() - mean).abs().numpy())
            err["std_" + tag] = np.maximum(err["std_" + tag], (nm._std[0].double().cpu() - std).abs().numpy())
            err["y_" + tag] = np.maximum(err["y_" + tag], (y.double() - y64).abs().amax(0).cpu().numpy())
        xmag = np.maximum(xmag, x.abs().amax(0).double().numpy())
        inv_max = np.maximum(inv_max, (1.0 / (std + EPS)).numpy())
    assert int(ker.count) == int(tor.count) == n * nb
    return err, _ulp(xmag), inv_max, ker


def test_kernels_reproduce_the_reference_golden():
    """The batches of tests/rl_synth.extra_inputs through the kernels, then once in evaluation mode, against the golden the reference's
    class wrote - the tolerances of tests/test_rl_extra.py::test_empirical_normalization_matches_reference, including the batch at
    which `until` stops the updates."""
    import torch
    from locotouch_amd.rl import EmpiricalNormalization
    from locotouch_amd.rl.fused import normalize_rows
    from tests.rl_synth import extra_inputs

    x = extra_inputs()
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "rl_extra.npz"))
    nz = EmpiricalNormalization(shape=[x["norm_batches"].shape[-1]], until=x["norm_until"]).to("cuda:0")
    bufs = [b.data_ptr() for b in (nz._mean, nz._var, nz._std, nz.count)]
    ys = [normalize_rows(nz, b.to("cuda:0").contiguous()).cpu() for b in x["norm_batches"]]
    nz.eval()
    ys.append(normalize_rows(nz, x["norm_batches"][0].to("cuda:0").contiguous()).cpu())
    assert bufs == [b.data_ptr() for b in (nz._mean, nz._var, nz._std, nz.count)]  # written in place
    np.testing.assert_allclose(torch.stack(ys).numpy(), g["norm_y"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(nz.mean.cpu().numpy(), g["norm_mean"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(nz.std.cpu().numpy(), g["norm_std"], rtol=1e-6, atol=1e-7)
    assert int(nz.count) == int(g["norm_count"]) and nz.count.dtype == torch.int64 and int(nz.count) >= x["norm_until"]


@pytest.mark.parametrize("n,d", [(1, 7), (37, 270), (4096, 348), (4100, 348), (32768, 348), (405, 1024)])
def test_kernels_against_float64(n, d):
    """30 consecutive batches with columns of mixed scales (`_mixed_batches`): mean, std and y per column against the recurrence in
    float64 on the CPU, bounded by the torch class's own f32 error (module docstring)."""
    print(f"\n  (n, d) = ({n}, {d})")
    err, ulp, inv_max, _ = _run_mixed(n, d)
    _assert_ratio("mean", err["mean_k"], err["mean_t"], ulp)
    _assert_ratio("std", err["std_k"], err["std_t"], ulp)
    _assert_ratio("y", err["y_k"], err["y_t"], ulp)


def test_two_runs_give_the_same_bits():
    import torch

    a, b = _run_mixed(4096, 348)[3], _run_mixed(4096, 348)[3]
    for name in ("_mean", "_var", "_std", "count"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_apply_serves_blocks_that_straddle_snapshots():
    """lt_obs_norm_apply with rows_per_snap not a multiple of its 64-row blocks, in place: bit-equal to (x - mean) * inv in torch
    (one subtraction, one multiplication, each rounded once: nothing to reorder)."""
    import torch
    from locotouch_amd import _abi

    torch.manual_seed(0)
    for rps, d in ((37, 270), (100, 348), (5, 7)):
        x = torch.randn(4 * rps, d, device="cuda:0")
        snaps = torch.randn(4, 3 * d, device="cuda:0")  # stride wider than a snapshot
        want = (x.view(4, rps, d) - snaps[:, None, :d]) * snaps[:, None, d:2 * d]
        _abi.call("lt_obs_norm_apply", x, 4 * rps, d, snaps, 3 * d, rps, x, _abi.stream("cuda:0"))
        assert torch.equal(x.view(4, rps, d), want), (rps, d)


def _rollout_setup(n, T, packed=True, seed=3):
    import torch
    from locotouch_amd.env import LocoTouchVecEnv
    from locotouch_amd.rl import PPO, ActorCritic, EmpiricalNormalization, FusedRollout
    from tests.rl_synth import POLICY_CFG, PPO_CFG

    env = LocoTouchVecEnv(TASK, num_envs=n, device="cuda:0", seed=seed)
    torch.manual_seed(1)
    alg = PPO(ActorCritic(env.num_obs, env.num_obs, 12, **POLICY_CFG), device="cuda:0", **PPO_CFG)
    alg.init_storage(n, T, [env.num_obs], [env.num_obs], [12])
    norms = [EmpiricalNormalization([env.num_obs], until=1.0e8).to("cuda:0") for _ in range(2)]
    fr = FusedRollout(env, alg, use_packed_mlp=packed, obs_normalizer=norms[0], critic_obs_normalizer=norms[1])
    return env, alg, norms, fr


@pytest.mark.parametrize("n,packed,training", [(4096, True, True), (37, True, True), (64, False, True), (4096, True, False)],
                         ids=["rows-in-storage", "arena-rows", "torch-modules", "eval-mode"])
def test_rollout_semantics(n, packed, training):
    """After rollout(T) and before normalize_storage(): the snapshots are the recurrence rerun in f64 on the raw slots 1..T-1 and the
    env's rows from the statistics before the rollout (bound: module docstring); mu and values of EVERY slot are the f64 networks
    (tests/mlp_ref.py) on the f64-normalised raw rows, within tests/test_hip_mlp_f64.py's rule plus the propagated input allowance
    (computed below).  After normalize_storage(): the slots are (raw - mean_t) * inv_t in f32 BIT FOR BIT (one subtraction and one
    multiplication, each rounded once, in the kernel as in torch), the env's rows are untouched and slot 0 of the next rollout is
    those raw rows.  `use_packed_mlp=False` is the path of a policy shape outside lt_mlp's limits (`_step_torch`)."""
    import torch
    from tests import mlp_ref as R
    from tests.parity_util import F64_RATIO, F64_ULPS

    T = 6
    env, alg, norms, fr = _rollout_setup(n, T, packed)
    st = alg.storage
    assert fr.rows_in_storage == (n % 16 == 0) and (fr.actor_mlp is not None) == packed
    assert fr.launches_per_step == (2 if packed else 11) + 2
    fr.begin()
    assert [int(m.count) for m in norms] == [n, n]
    if not training:
        for m in norms:
            m.eval()
        assert fr.launches_per_step == 3
        fr.begin()  # evaluation mode: normalises, merges nothing
        assert [int(m.count) for m in norms] == [n, n]
    before = [(m._mean[0].double().cpu(), m._var[0].double().cpu(), int(m.count)) for m in norms]
    twins = copy.deepcopy(norms)  # the torch class in f32 from the same statistics: the yardstick of the bound
    fr.rollout(T)
    torch.cuda.synchronize()
    raw = (st.observations.clone(), st.privileged_observations.clone())
    arena = (env.obs_policy.clone(), env.obs_critic.clone())
    assert [int(m.count) for m in norms] == [n * (1 + T * training)] * 2
    for w in range(2):
        snaps = fr.snapshots(w).clone()
        batches = [raw[w][t] for t in range(1, T)] + [arena[w]]
        mean, var, count = before[w]
        xmag = torch.stack([b.abs().amax(0) for b in batches + [raw[w][0]]]).amax(0).double().cpu().numpy()
        ulp = _ulp(xmag)
        assert torch.equal(snaps[0, 0], twins[w]._mean[0])  # slot 0: the statistics before the rollout
        assert torch.allclose(snaps[0, 1], 1.0 / (twins[w]._std[0] + EPS), rtol=2.0 ** -22, atol=0)
        em_k, em_t, ei_k, ei_t, inv_mag = (np.zeros_like(xmag) for _ in range(5))
        net = (alg.actor_critic.actor, alg.actor_critic.critic)[w]
        got = (st.mu, st.values)[w]
        worst = {}
        for t in range(T + 1):  # slot t: the statistics behind batch t (slot 0: those before the rollout)
            if t >= 1 and training:
                mean, var, count = _rec64(mean, var, count, batches[t - 1], 1.0e8)
                with torch.no_grad():
                    twins[w].update(batches[t - 1])
            inv64 = 1.0 / (var.sqrt() + EPS)
            inv_t = 1.0 / (twins[w]._std[0] + EPS)  # what the torch class divides by, as the f32 number the snapshot would hold
            em_k = np.maximum(em_k, (snaps[t, 0].double().cpu() - mean).abs().numpy())
            em_t = np.maximum(em_t, (twins[w]._mean[0].double().cpu() - mean).abs().numpy())
            ei_k = np.maximum(ei_k, (snaps[t, 1].double().cpu() - inv64).abs().numpy())
            ei_t = np.maximum(ei_t, (inv_t.double().cpu() - inv64).abs().numpy())
            inv_mag = np.maximum(inv_mag, inv64.numpy())
            if t == T:
                break
            # mu / values of slot t against the f64 network on the f64-normalised raw rows (tests/test_hip_mlp_f64.py's rule: e_hip <=
            # F64_RATIO e_f32 + F64_ULPS f32 ulps of the field), widened by what check 3 allows the input rows to be off by - per
            # column max(2 x the torch class's error in y, one ulp of the column) - propagated through the f64 network to first order:
            # max over rows and outputs of sum_c |d out / d y_c| delta_c
            x = raw[w][t]
            y64 = (x.double() - mean.to(x.device)) / (var.sqrt().to(x.device) + EPS)
            with torch.no_grad():
                y_t = (x - twins[w]._mean) / (twins[w]._std + EPS)
            delta = torch.maximum(2.0 * (y_t.double() - y64).abs().amax(0), torch.as_tensor(ulp, device=x.device))
            yg = y64.clone().requires_grad_(True)
            with torch.enable_grad():
                ref = R.forward64(net, yg)[0]
                prop = 0.0
                for k in range(ref.shape[1]):
                    grad, = torch.autograd.grad(ref[:, k].sum(), yg, retain_graph=k + 1 < ref.shape[1])
                    prop = max(prop, float((grad.abs() @ delta).max()))
            ref = ref.detach()
            e_hip, e_f32 = R.err(got[t], ref), R.err(R.forward32(net, y64.float())[0], ref)
            allowed = F64_RATIO * e_f32[0] + F64_ULPS * 2.0 ** -24 * e_hip[1] + prop
            if not worst or e_hip[0] / allowed > worst["e_hip"] / worst["allowed"]:
                worst = dict(t=t, e_hip=e_hip[0], e_f32=e_f32[0], prop=prop, allowed=allowed, top=e_hip[1])
            assert e_hip[0] <= allowed, (w, t, e_hip, e_f32, prop)
        print(f"\n  network {w}: worst slot {worst['t']}: |out - f64| {worst['e_hip']:.3e}, torch f32 {worst['e_f32']:.3e}, propagated input "
              f"allowance {worst['prop']:.3e}, allowed {worst['allowed']:.3e}, |f64| {worst['top']:.3e}")
        _assert_ratio("mean", em_k, em_t, ulp)
        _assert_ratio("inv", ei_k, ei_t, _ulp(inv_mag))
    fr.normalize_storage()
    torch.cuda.synchronize()
    for w, rows in enumerate((st.observations, st.privileged_observations)):
        s = fr.snapshots(w)
        assert torch.equal(rows, (raw[w] - s[:T, 0].unsqueeze(1)) * s[:T, 1].unsqueeze(1)), w
        assert torch.isfinite(rows).all()
    assert torch.equal(env.obs_policy, arena[0]) and torch.equal(env.obs_critic, arena[1])
    assert torch.equal(fr.last_critic_obs, (arena[1] - fr.snapshots(1)[T, 0]) * fr.snapshots(1)[T, 1])
    carried = fr.snapshots(0)[T].clone()
    fr.rollout(T)
    torch.cuda.synchronize()
    assert torch.equal(st.observations[0], arena[0]) and torch.equal(st.privileged_observations[0], arena[1])
    assert torch.equal(fr.snapshots(0)[0], carried)  # slot 0 is not merged a second time
    assert [int(m.count) for m in norms] == [n * (1 + 2 * T * training)] * 2


def test_captured_rollout_replays_the_plain_one_bit_for_bit():
    """A plain and a hipGraph-captured-and-replayed 24-step rollout from the same env state and seed: raw rows, snapshots, mu,
    values and statistics bit-equal (one linear graph: the normaliser's launches sit on the rollout's stream)."""
    import torch

    n, T = 4096, 24
    res = []
    for captured in (False, True):
        env, alg, norms, fr = _rollout_setup(n, T)
        fr.begin()
        if captured:
            # capture without running: what a capture pass leaves in the statistics does not matter, the graph is replayed once on
            # state restored to the start
            state = (env._arena_aligned.clone(), [copy.deepcopy(m.state_dict()) for m in norms], fr.norm_rows[0].clone(),
                     fr.norm_rows[1].clone(), fr._carry.clone(), [w.clone() for w in fr._norm_ws])  # (the workspaces hold the f64 state)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                fr.rollout(T)  # warm-up off the default stream, as torch's capture wants
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fr.rollout(T)
            env._arena_aligned.copy_(state[0])
            for m, sd in zip(norms, state[1]):
                for k, v in sd.items():
                    getattr(m, k).copy_(v)  # in place: the graph holds these pointers
            fr.norm_rows[0].copy_(state[2]); fr.norm_rows[1].copy_(state[3]); fr._carry.copy_(state[4])
            for w, saved in zip(fr._norm_ws, state[5]):
                w.copy_(saved)
            g.replay()
        else:
            fr.rollout(T)
        torch.cuda.synchronize()
        st = alg.storage
        res.append([st.observations.clone(), st.privileged_observations.clone(), fr._snaps.clone(), st.mu.clone(), st.values.clone(),
                    st.actions.clone(), env.obs_policy.clone()] + [getattr(m, k).clone() for m in norms for k in ("_mean", "_var", "_std", "count")])
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), i
    assert int(res[0][-1]) == n * (1 + T)


@pytest.mark.parametrize("n", [64, 4096])
def test_runner_trains_on_the_fused_path_with_normalisation(n, tmp_path):
    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import FusedRollout, OnPolicyRunner

    cfg = dict(train_cfg(TASK), empirical_normalization=True)
    runner = OnPolicyRunner(make(TASK, num_envs=n, device="cuda:0", seed=1), cfg, log_dir=str(tmp_path), device="cuda:0")
    fused = runner._make_fused()
    assert isinstance(fused, FusedRollout) and fused.normalizers == (runner.obs_normalizer, runner.critic_obs_normalizer)
    assert fused.launches_per_step == 4
    K, T = 2, runner.num_steps_per_env
    runner.learn(K)
    assert all(np.isfinite(r["Loss/value_function"]) and np.isfinite(r["Loss/surrogate"]) for r in runner.history)
    for nm in (runner.obs_normalizer, runner.critic_obs_normalizer):
        assert int(nm.count) == n * (1 + T * K)
    loaded = torch.load(os.path.join(str(tmp_path), f"model_{K - 1}.pt"), weights_only=True)
    d = runner.env.num_obs
    for key in ("obs_norm_state_dict", "critic_obs_norm_state_dict"):
        sd = loaded[key]
        assert sorted(sd) == ["_mean", "_std", "_var", "count"] and sd["count"].dtype == torch.int64
        assert all(tuple(sd[k].shape) == (1, d) for k in ("_mean", "_std", "_var"))
    runner2 = OnPolicyRunner(make(TASK, num_envs=n, device="cuda:0", seed=2), cfg, log_dir=None, device="cuda:0")
    runner2.load(os.path.join(str(tmp_path), f"model_{K - 1}.pt"))
    for a, b in ((runner.obs_normalizer, runner2.obs_normalizer), (runner.critic_obs_normalizer, runner2.critic_obs_normalizer)):
        for k in ("_mean", "_var", "_std", "count"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
    x = runner.env.obs_policy.clone()
    policy = runner.get_inference_policy(device="cuda:0")
    with torch.inference_mode():
        assert torch.equal(policy(x), runner.alg.actor_critic.actor(runner.obs_normalizer(x)))
    # without the switch: the same two launches per step as before
    off = OnPolicyRunner(make(TASK, num_envs=64, device="cuda:0", seed=1), train_cfg(TASK), log_dir=None, device="cuda:0")._make_fused()
    assert isinstance(off, FusedRollout) and off.normalizers is None and off.launches_per_step == 2


def test_unserved_cases_keep_the_eager_path():
    """bf16 observation rows and more than one rank: FusedRollout refuses normalisers on bf16 storage, the runner keeps its eager loop."""
    import types

    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import EmpiricalNormalization, FusedRollout, OnPolicyRunner

    n = 64
    cfg = dict(train_cfg(TASK), empirical_normalization=True)
    runner = OnPolicyRunner(make(TASK, num_envs=n, device="cuda:0", seed=1), cfg, log_dir=None, device="cuda:0")
    d = runner.env.num_obs
    assert isinstance(runner._make_fused(), FusedRollout)
    dist = runner.dist
    runner.dist = types.SimpleNamespace(world_size=2)
    assert runner._make_fused() is None
    runner.dist = dist
    runner.alg.init_storage(n, runner.num_steps_per_env, [d], [d], [12], obs_dtype=torch.bfloat16)
    assert runner._make_fused() is None
    made = []
    init = FusedRollout.__init__
    FusedRollout.__init__ = lambda self, *a, **k: (made.append(1), init(self, *a, **k))[1]
    try:
        runner.learn(1)  # the eager loop with the torch normaliser, on bf16 storage
    finally:
        FusedRollout.__init__ = init
    assert not made and runner.alg.storage.observations.dtype == torch.bfloat16
    rec = runner.history[-1]
    assert np.isfinite(rec["Loss/value_function"]) and np.isfinite(rec["Loss/surrogate"])
    for nm in (runner.obs_normalizer, runner.critic_obs_normalizer):
        assert int(nm.count) == n * (1 + runner.num_steps_per_env) and bool(torch.isfinite(nm._mean).all() and torch.isfinite(nm._std).all())
    norms = [EmpiricalNormalization([d]).to("cuda:0") for _ in range(2)]
    with pytest.raises(ValueError, match="(?s)normalis.*bf16"):
        FusedRollout(runner.env, runner.alg, obs_normalizer=norms[0], critic_obs_normalizer=norms[1])
    with pytest.raises(ValueError, match="both"):
        FusedRollout(runner.env, runner.alg, obs_normalizer=norms[0])


def test_two_ranks_with_normalisation_train_on_the_eager_path(tmp_path):
    """Two ranks on one card over gloo (spawned as tests/test_hip_dist.py spawns its ranks), switch on: each rank trains one
    iteration on the eager loop with its own statistics (count == N (1 + T) per rank), no FusedRollout is constructed
    (tests/_obs_norm_dist_child.py makes its constructor raise), and the replicas' parameters stay equal."""
    import socket
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   LT_DIST_BACKEND="gloo", LT_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(repo, "tests", "_obs_norm_dist_child.py"), str(tmp_path)], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    res = [json.load(open(os.path.join(str(tmp_path), f"obs_norm_rank{r}.json"))) for r in range(2)]
    for r in res:
        assert r["counts"] == [64 * (1 + r["steps"])] * 2 and r["finite"] and all(np.isfinite(v) for v in r["losses"])
    assert res[0]["params"] == res[1]["params"]


def test_statistics_written_by_something_else_are_adopted():
    """The recurrence runs on f64 copies of mean and var in the workspace, used only while the f32 buffers hold what the kernels last
    wrote (include/lt_obs_norm.h).  Here the torch class merges one batch between two kernel calls (as a loaded checkpoint would
    replace the buffers): the next kernel call must continue from the f32 buffers as they now are - compared with the f64 recurrence
    restarted from exactly those values, to half an ulp of the result (one rounding of the f64 state)."""
    import torch
    from locotouch_amd.rl import EmpiricalNormalization
    from locotouch_amd.rl.fused import normalize_rows

    n, d = 512, 270
    nz = EmpiricalNormalization([d]).to("cuda:0")
    batches = list(_mixed_batches(n, d, 5, seed=11))
    for x in batches[:3]:
        normalize_rows(nz, x.to("cuda:0"))
    with torch.no_grad():
        nz.update(batches[3].to("cuda:0"))  # rebinds `_std`, rewrites `_mean` / `_var`: the f64 copies are stale now
    mean, var, count = nz._mean[0].double().cpu(), nz._var[0].double().cpu(), int(nz.count)
    normalize_rows(nz, batches[4].to("cuda:0"))
    mean, var, count = _rec64(mean, var, count, batches[4], None)
    assert int(nz.count) == count == 5 * n
    em = (nz._mean[0].double().cpu() - mean).abs().numpy()
    std = var.clamp_min(0.0).sqrt()  # (the kernel takes the root of max(var, 0): a constant column's var may round below zero)
    es = (nz._std[0].double().cpu() - std).abs().numpy()
    assert (em <= 0.51 * _ulp(mean.numpy())).all(), float((em / _ulp(mean.numpy())).max())
    assert (es <= 0.51 * _ulp(std.numpy())).all(), float(es.max())


def test_update_consumes_the_normalised_rows():
    """One optimizer step of PPO._direct_update on the storage that rollout() filled and normalize_storage() rewrote, against the
    autograd form (`direct_update=False`) on a second storage that holds the same rollout with its observation rows normalised in
    TORCH from the raw rows and the per-slot snapshots - the one-step tolerances of
    tests/test_hip_ppo_graph.py::test_direct_update_without_host_reads_equals_the_autograd_form."""
    import torch
    from locotouch_amd.env import LocoTouchVecEnv
    from locotouch_amd.rl import PPO, ActorCritic, EmpiricalNormalization, FusedRollout, tuned_gemms
    from tests.rl_synth import POLICY_CFG, PPO_CFG

    tuned_gemms.disable()
    n, T = 1024, 24
    env = LocoTouchVecEnv(TASK, num_envs=n, device="cuda:0", seed=3)
    d = env.num_obs
    cfg = dict(PPO_CFG, num_learning_epochs=1, num_mini_batches=1, tuned_gemms=False)
    algs = []
    for direct in (True, False):
        torch.manual_seed(0)
        alg = PPO(ActorCritic(d, d, 12, **POLICY_CFG), device="cuda:0", direct_update=direct, **cfg)
        alg.init_storage(n, T, [d], [d], [12])
        algs.append(alg)
    a, b = algs
    assert a.direct_update and not b.direct_update and a._flat_adam is not None and b._flat_adam is not None
    norms = [EmpiricalNormalization([d], until=1.0e8).to("cuda:0") for _ in range(2)]
    fr = FusedRollout(env, a, obs_normalizer=norms[0], critic_obs_normalizer=norms[1])
    fr.begin()
    fr.rollout(T)
    torch.cuda.synchronize()
    raw = (a.storage.observations.clone(), a.storage.privileged_observations.clone())
    fr.normalize_storage()
    with torch.inference_mode():
        a.compute_returns(fr.last_critic_obs)
    sa, sb = a.storage, b.storage
    for name in ("actions", "mu", "sigma", "rewards", "dones", "values", "actions_log_prob"):
        getattr(sb, name).copy_(getattr(sa, name))
    sb.step = sa.step
    for w, name in enumerate(("observations", "privileged_observations")):
        s = fr.snapshots(w)
        getattr(sb, name).copy_((raw[w] - s[:T, 0].unsqueeze(1)) * s[:T, 1].unsqueeze(1))
    with torch.inference_mode():
        b.compute_returns((env.obs_critic - fr.snapshots(1)[T, 0]) * fr.snapshots(1)[T, 1])
    assert not torch.equal(sa.observations, raw[0])  # the update below reads rewritten rows, not the raw ones
    outs = []
    for alg in (a, b):
        torch.manual_seed(11)
        outs.append(alg.update())
    for x, y in zip(outs[0][:3], outs[1][:3]):
        assert abs(x - y) <= 1e-6 * max(1.0, abs(y)), outs
    for (name, pa), pb in zip(a.actor_critic.named_parameters(), b.actor_critic.parameters()):
        assert float((pa.grad - pb.grad).abs().max()) <= 3e-6 * float(pb.grad.abs().max()), name
        torch.testing.assert_close(pa, pb, rtol=0, atol=2 * a.learning_rate)
        assert float((pa - pb).abs().mean()) < 1e-6, name


def test_learning_sanity_100_iterations(tmp_path):
    """100 PPO iterations, teacher task, 4096 envs, switch on.  No threshold on the return (normalisation changes the optimisation
    problem): finite losses and statistics, and the mean episode length behind the last iteration above the first one reported.
    OBS_NORM_PROGRESS_DIR: where to keep progress.jsonl (the curve under profiles/ was recorded that way)."""
    import torch
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    log_dir = os.environ.get("OBS_NORM_PROGRESS_DIR") or str(tmp_path)
    cfg = dict(train_cfg(TASK), empirical_normalization=True, save_interval=1000)
    runner = OnPolicyRunner(make(TASK, num_envs=4096, device="cuda:0", seed=1), cfg, log_dir=log_dir, device="cuda:0")
    runner.learn(100)
    h = runner.history
    assert len(h) == 100 and all(np.isfinite(r["Loss/value_function"]) and np.isfinite(r["Loss/surrogate"]) for r in h)
    for nm in (runner.obs_normalizer, runner.critic_obs_normalizer):
        assert all(bool(torch.isfinite(getattr(nm, k)).all()) for k in ("_mean", "_var", "_std"))
        assert int(nm.count) == 4096 * (1 + runner.num_steps_per_env * 100)
    lens = [r["Train/mean_episode_length"] for r in h if r["Train/mean_episode_length"] is not None]
    print("\n  episode length", lens[0], "->", lens[-1], " reward", h[0]["Train/mean_reward"], "->", h[-1]["Train/mean_reward"])
    print("  " + json.dumps({k: h[-1][k] for k in ("Loss/value_function", "Loss/surrogate", "Policy/mean_noise_std")}))
    assert h[-1]["Train/mean_episode_length"] is not None and lens[-1] > lens[0]
