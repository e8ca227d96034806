"""Child process of tests/test_hip_obs_norm.py::test_two_ranks_with_normalisation_train_on_the_eager_path: one rank of a two-rank
training run with `empirical_normalization` on ONE card (gloo, as tests/_dist_child.py).  The runner must keep the eager loop: a
FusedRollout that is constructed anywhere fails the run."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locotouch_amd.agents import train_cfg  # noqa: E402
from locotouch_amd.env import make  # noqa: E402
from locotouch_amd.rl import Dist, FusedRollout, OnPolicyRunner  # noqa: E402

TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
N = 64


def main(out):
    dist = Dist.from_env()
    assert dist.world_size == 2
    torch.manual_seed(1)
    env = make(TASK, num_envs=N, device="cuda:0", seed=1, env_index_offset=dist.rank * N, cur_gate_external=1)
    cfg = dict(train_cfg(TASK), empirical_normalization=True)
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0", dist=dist)

    def refuse(self, *a, **k):
        raise AssertionError("a FusedRollout was constructed on a multi-rank run with normalisation")

    FusedRollout.__init__ = refuse
    assert runner._make_fused() is None
    runner.learn(1)
    rec = runner.history[-1]
    res = {"rank": dist.rank, "counts": [int(runner.obs_normalizer.count), int(runner.critic_obs_normalizer.count)],
           "steps": runner.num_steps_per_env, "losses": [rec["Loss/value_function"], rec["Loss/surrogate"]],
           "finite": bool(torch.isfinite(runner.obs_normalizer._mean).all() and torch.isfinite(runner.obs_normalizer._std).all()),
           "params": float(torch.cat([p.detach().flatten() for p in runner.alg.actor_critic.parameters()]).double().sum())}
    with open(os.path.join(out, f"obs_norm_rank{dist.rank}.json"), "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
