#!/usr/bin/env python3
"""Cost of the contact-force vectors: lt_step_kernel time (lt_env_step_profiled: HIP events around the step kernel alone) of the
same task with and without a bound vector buffer, alternating env by env in rounds so that clock and thermal drift hit both.

    python tools/contact_force_cost.py [--task teacher] [--envs 4096 32768] [--rounds 7] [--steps 20]

Prints one JSON line per population size: per-round medians of each variant, their medians and the relative cost.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TASKS = {"teacher": "Isaac-RandCylinderTransportTeacher-LocoTouch-v1", "locomotion": "Isaac-Locomotion-LocoTouch-v1"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="teacher", choices=sorted(TASKS))
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="profiled steps per variant and round")
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds must be at least 5")

    import torch

    from locotouch_amd.env import LocoTouchVecEnv

    for n in args.envs:
        envs = {v: LocoTouchVecEnv(TASKS[args.task], num_envs=n, device="cuda:0", seed=42, contact_force_vectors=v) for v in (False, True)}
        g = torch.Generator(device="cpu").manual_seed(0)
        acts = [(0.5 * torch.randn(n, 12, generator=g)).to("cuda:0") for _ in range(8)]
        for e in envs.values():
            for i in range(args.warmup):
                e.step_profiled(acts[i % len(acts)])
        per_round = {False: [], True: []}
        for r in range(args.rounds):
            for v in ((False, True) if r % 2 == 0 else (True, False)):
                ms = [envs[v].step_profiled(acts[i % len(acts)]) for i in range(args.steps)]
                per_round[v].append(statistics.median(ms))
        off, on = statistics.median(per_round[False]), statistics.median(per_round[True])
        print(json.dumps({"task": args.task, "envs": n, "rounds": args.rounds, "steps_per_round": args.steps,
                          "step_kernel_us_off": 1e3 * off, "step_kernel_us_on": 1e3 * on, "cost_rel": on / off - 1.0,
                          "round_medians_us_off": [round(1e3 * x, 2) for x in per_round[False]],
                          "round_medians_us_on": [round(1e3 * x, 2) for x in per_round[True]]}), flush=True)
        del envs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
