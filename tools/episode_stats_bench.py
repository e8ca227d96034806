"""What the episode statistics of `--episode_stats` cost per env step; writes profiles/episode_stats_<envs>.json.

    python tools/episode_stats_bench.py [--envs 4096] [--out FILE] [--no-trace] [--parent-json FILE]
    python tools/episode_stats_bench.py --legs plain --no-trace --out FILE      # on a checkout of the parent commit: the plain legs alone

The teacher env at 4096 envs, episode_stats.default_metrics (11 metrics + the length).  Three measurements, each in a fresh child process
with a time limit of its own (this driver never opens the GPU):
  kernels: the kernels' own time - lt_episode_stats_step_kernel beside lt_step_kernel - from one `rocprofv3 --kernel-trace --stats` run
           of `--mode trace` (the program after `--`, no counters in the run): 200 env steps with random actions, and one reduce.
  rollout: the per-step wall time of a fused 24-step rollout (rl.FusedRollout, eager launches, 10 rollouts per round) with and without
           `env.episode_stats`, alternating, median [min, max] of 7 rounds, each round ending in a device synchronise.
  play:    the per-step wall time of a 100-step play window (env.step with zero actions), the same two legs, the same way.
`--legs plain` measures the legs without the attribute alone and imports nothing of the unit, so the same file runs on a checkout of the
parent commit; `--parent-json` takes that run's output and says whether the plain intervals overlap.  No speed is promised.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
KERNELS = ("lt_episode_stats_step_kernel", "lt_episode_stats_reduce_kernel", "lt_step_kernel")
LEGS = ("plain", "episode_stats")
ROLLOUT, ROLLOUTS_PER_ROUND = 24, 10
POLICY_CFG = dict(init_noise_std=1.0, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu")


def stats(xs) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def setup(leg: str, envs: int, fused: bool):
    """(env, FusedRollout or None) of one leg; the plain leg imports nothing of the unit."""
    import torch

    from locotouch_amd.env import make

    env = make(TASK, num_envs=envs, device="cuda:0", seed=1)
    if leg == "episode_stats":
        from locotouch_amd.episode_stats import EpisodeStats

        env.episode_stats = EpisodeStats(env, skip_running=False)
    if not fused:
        return env, None
    from locotouch_amd.rl import PPO, ActorCritic, FusedRollout

    torch.manual_seed(1234)
    alg = PPO(ActorCritic(env.num_obs, env.num_obs, 12, **POLICY_CFG), device="cuda:0")
    alg.init_storage(envs, ROLLOUT, [env.num_obs], [env.num_obs], [12])
    return env, FusedRollout(env, alg)


def trace(envs: int, steps: int) -> dict:
    """`steps` env steps with the statistics attached and one summary: under the profiler this is the run whose kernel statistics are read."""
    import torch

    env, _ = setup("episode_stats", envs, fused=False)
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = (0.5 * torch.randn(8, envs, 12, generator=g)).to("cuda:0")
    for t in range(steps):
        env.step(acts[t % 8])
    summary = env.episode_stats.summary()
    torch.cuda.synchronize()
    return {"steps": steps, "envs": envs, "metrics": len(env.episode_stats.metrics) + 1, "episodes_finished": summary["length"]["episodes"]}


def wall(what: str, legs: list, envs: int, rounds: int, warmup: int, steps: int) -> dict:
    import torch

    fused = what == "rollout"
    made = {leg: setup(leg, envs, fused) for leg in legs}
    act = torch.zeros(envs, 12, device="cuda:0")
    times = {leg: [] for leg in legs}
    per_round = ROLLOUT * ROLLOUTS_PER_ROUND if fused else steps
    for r in range(warmup + rounds):
        for leg in legs:  # alternating: every leg sees the same machine
            env, rollout = made[leg]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if fused:
                for _ in range(ROLLOUTS_PER_ROUND):
                    rollout.rollout(ROLLOUT)
            else:
                for _ in range(steps):
                    env.step(act)
            torch.cuda.synchronize()
            if r >= warmup:
                times[leg].append((time.perf_counter() - t0) * 1e3 / per_round)
    return {"device": torch.cuda.get_device_name(0), "envs": envs, "steps_per_round": per_round, **{f"step_ms_{leg}": stats(times[leg]) for leg in legs}}


def child(mode: str, extra: list, timeout: int, profiler_dir: str | None = None) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode] + extra
    if profiler_dir is not None:
        exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if not os.path.exists(exe):
            return {"error": "rocprofv3 not found"}
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", profiler_dir, "-o", "trace", "--"] + cmd
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {"error": f"--mode {mode}: no result within {timeout} s"}
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        return {"error": f"--mode {mode}: exit {p.returncode}: {(p.stderr or p.stdout)[-500:]}"}
    return json.loads(line[-1][7:])


def kernel_stats(folder: str) -> dict:
    """Per kernel of KERNELS the row with the most calls (lt_step_kernel is a template: the instantiation the steady steps run, not one
    that ran once), with the instantiations found."""
    rows = {}
    for path in glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k not in row.get("Name", ""):
                    continue
                calls = int(row["Calls"])
                seen = rows.get(k, {}).get("instantiations", 0) + 1
                if calls > rows.get(k, {}).get("calls", 0):
                    rows[k] = {"calls": calls, "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                               "max_us": float(row["MaxNs"]) / 1e3}
                rows[k]["instantiations"] = seen
    return rows


def overlap(a: dict, b: dict) -> bool:
    return a["min"] <= b["max"] and b["min"] <= a["max"]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=None, help="default: profiles/episode_stats_<envs>.json")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100, help="env steps of one round of the play window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-steps", type=int, default=200)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated legs of the wall measurements: " + ", ".join(LEGS))
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--parent-json", default=None, help="the output of `--legs plain --no-trace` on a checkout of the parent commit")
    ap.add_argument("--mode", choices=["trace", "rollout", "play"], help="(internal) one measurement in this process; prints a RESULT line")
    args = ap.parse_args()
    legs = [leg for leg in args.legs.split(",") if leg]
    if args.mode == "trace":
        print("RESULT " + json.dumps(trace(args.envs, args.trace_steps)))
        return
    if args.mode in ("rollout", "play"):
        print("RESULT " + json.dumps(wall(args.mode, legs, args.envs, args.rounds, args.warmup, args.steps)))
        return
    out = args.out or os.path.join(REPO, "profiles", f"episode_stats_{args.envs}.json")
    res = {"task": TASK, "envs": args.envs, "setup": "episode_stats.default_metrics; rollout: eager FusedRollout of 24 steps; play: env.step, zero actions"}
    if args.no_trace:
        res["kernels"] = "not measured"
    else:
        tmp = tempfile.mkdtemp(prefix="episode_stats_prof_")
        run = child("trace", ["--envs", str(args.envs), "--trace-steps", str(args.trace_steps)], 300, profiler_dir=tmp)
        rows = kernel_stats(tmp) if "error" not in run else {}
        shutil.rmtree(tmp, ignore_errors=True)
        res["kernels"] = {**run, **(rows or {"error": run.get("error", "no row of the kernels in the kernel statistics")}),
                          "source": "rocprofv3 --kernel-trace --stats, one run, no counters"}
    common = ["--envs", str(args.envs), "--legs", ",".join(legs), "--rounds", str(args.rounds), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    for what in ("rollout", "play"):
        res[what] = child(what, common, 300)
        both = [res[what].get(f"step_ms_{leg}") for leg in LEGS]
        if all(both):
            res[what]["intervals_overlap"] = overlap(*both)
    if args.parent_json:
        parent = json.load(open(args.parent_json))
        res["parent_commit"] = {"note": "the plain legs, measured with this tool on a checkout of the parent commit"}
        for what in ("rollout", "play"):
            theirs, mine = (parent.get(what) or {}).get("step_ms_plain"), res[what].get("step_ms_plain")
            res["parent_commit"][what] = theirs
            if mine and theirs:
                res["parent_commit"][f"{what}_plain_intervals_overlap"] = overlap(mine, theirs)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
