#!/usr/bin/env python3
"""Golden-vector generator for PPO's `symmetry_cfg` branch: the REFERENCE's own `loco_rl` PPO.update() with this project's
`mirror_go1` as its data-augmentation function, on the seeded synthetic rollout of tests/rl_synth.py (64 envs x 24 steps, 348
columns, 12 actions - the sizes of rl_ppo_cfg1), in four modes: augmentation, mirror loss only, both, and both flags false (the
symmetry loss is then logged only).  Data only: what is stored are the five values update() returned, the learning rate and sums
over the parameters.  Runs only where the reference is checked out beside the repository (with the two in-memory stubs of SURVEY.md
Appendix E for the absent `git` / `isaaclab` modules).

    python tools/gen_golden_ppo_symmetry.py   # writes tests/golden/ppo_symmetry.npz
"""
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(os.environ.get("LOCOTOUCH_REFERENCE", os.path.join(os.path.dirname(REPO), "reference")), "loco_rl"))
sys.modules.setdefault("git", types.ModuleType("git"))
il, ilu = types.ModuleType("isaaclab"), types.ModuleType("isaaclab.utils")
ilu.configclass = lambda c: c
il.utils = ilu
sys.modules.update({"isaaclab": il, "isaaclab.utils": ilu})

import contextlib  # noqa: E402
import io  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from loco_rl.algorithms import PPO  # noqa: E402
from loco_rl.modules import ActorCritic  # noqa: E402

from locotouch_amd.rl.symmetry import mirror_go1  # noqa: E402
from tests.rl_synth import N_ACT, N_ENVS, N_OBS, N_STEPS, POLICY_CFG, PPO_CFG, synth_rollout  # noqa: E402
from tests.symmetry_synth import MODES, TeacherRows, symmetry_cfg  # noqa: E402


def run(mode):
    torch.set_num_threads(1)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        ac = ActorCritic(N_OBS, N_OBS, N_ACT, **POLICY_CFG)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (logging_only: "Symmetry not used for learning")
        alg = PPO(ac, device="cpu", symmetry_cfg=symmetry_cfg(mode, mirror_go1, TeacherRows()), **PPO_CFG)
    alg.init_storage(N_ENVS, N_STEPS, [N_OBS], [N_OBS], [N_ACT])
    data = synth_rollout(seed=123)
    for t in range(N_STEPS):
        alg.act(data["obs"][t], data["critic_obs"][t])
        alg.process_env_step(data["rewards"][t], data["dones"][t], {"time_outs": data["time_outs"][t]})
    alg.compute_returns(data["last_critic_obs"])
    v, s, e, rnd, sym = alg.update()
    assert rnd is None
    sd = alg.actor_critic.state_dict()
    return {f"{mode}/losses": np.array([v, s, e, sym], dtype=np.float64), f"{mode}/learning_rate": np.array(alg.learning_rate),
            f"{mode}/param_names": np.array(list(sd.keys())),
            f"{mode}/param_sum": np.array([p.double().sum().item() for p in sd.values()]),
            f"{mode}/param_abs_sum": np.array([p.double().abs().sum().item() for p in sd.values()]),
            f"{mode}/std": sd["std"].numpy(), f"{mode}/actor_last_bias": sd["actor.6.bias"].numpy()}


def main():
    out = {}
    for mode in MODES:
        out.update(run(mode))
        print(mode, "losses", out[f"{mode}/losses"], "lr", out[f"{mode}/learning_rate"])
    np.savez_compressed(os.path.join(REPO, "tests", "golden", "ppo_symmetry.npz"), **out)


if __name__ == "__main__":
    main()
