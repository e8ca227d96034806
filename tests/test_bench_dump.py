"""`bench.py --dump-outputs DIR` (bench.py::dump_outputs): the last timed step's per-env outputs as float32 .npy files, all env
rows while they fit the 64 MB budget, else the same seeded row sample in every file.  CPU: a stand-in env and a real storage."""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NAMES = ["action_mean", "action_std", "actions", "actions_log_prob", "critic_obs", "dones", "obs", "rewards", "values"]


def _filled(n, t):
    from locotouch_amd.rl.storage import RolloutStorage

    st = RolloutStorage(n, 24, 348, 348, 12)
    row = torch.arange(n, dtype=torch.float32)
    st.actions[t] = row[:, None] + 0.5
    st.rewards[t, :, 0] = -row
    st.dones[t, :, 0] = (torch.arange(n) % 3 == 0).to(torch.uint8)
    env = types.SimpleNamespace(num_envs=n, obs_policy=row[:, None].expand(n, 348).clone(), obs_critic=torch.ones(n, 348))
    return env, st


def test_small_population_is_dumped_whole(tmp_path):
    import bench

    env, st = _filled(64, 5)
    rec = bench.dump_outputs(str(tmp_path), env, st, 5)
    assert sorted(f[:-4] for f in os.listdir(tmp_path)) == NAMES and rec["env_rows"] == "all" and rec["storage_slot"] == 5
    for name in NAMES:
        assert np.load(tmp_path / f"{name}.npy").dtype == np.float32
    np.testing.assert_array_equal(np.load(tmp_path / "actions.npy")[:, 0], np.arange(64) + 0.5)
    np.testing.assert_array_equal(np.load(tmp_path / "dones.npy")[:, 0], (np.arange(64) % 3 == 0).astype(np.float32))


def test_large_population_is_a_fixed_row_sample_within_64_mb(tmp_path):
    import bench

    env, st = _filled(32768, 23)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), env, st, 23)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64_000_000
    rows = np.load(tmp_path / "a" / "obs.npy")[:, 0]
    assert 20000 < len(rows) < 32768 and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "actions.npy")[:, 0], rows + 0.5)  # the same rows in every file
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rewards.npy")[:, 0], -rows)
    for name in NAMES:  # and the same sample from run to run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy"))
