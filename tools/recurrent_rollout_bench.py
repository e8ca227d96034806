"""What the rollout of a recurrent (LSTM) policy costs in the eager loop and on the fused path: writes profiles/recurrent_rollout_<n>.json.

Teacher task, `--envs` envs (4096), `ActorCriticRecurrent` with LSTM memories of H = 256 (I from the task), 24 steps per rollout; two legs,
a fresh process each:
  off  `fused_recurrent_rollout` off: the runner's reference-shaped eager loop (two clones of the state, two library GEMMs, two
       lt_lstm_forward(L = 1), torch MLPs and sampling, storage.add, reset(dones) - per step).  The code of this leg is the code of the
       commit before the switch existed.
  on   the switch on: lt_memory_step + policy/value + env step, three launches per step (rl/fused.py).
Per leg: `rollout_ms` - one 24-step rollout, host wall clock between two device synchronisations, median of `--rounds` rounds behind
`--warmup`, with min and max (the spread); `iteration_ms` - one whole PPO iteration (collection + learning time of `runner.learn`, which
ends in the update's host read), same statistics.  The `on` leg also times the rollout captured into one hipGraph (events).
The memory-step kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of its own (`--mode trace` under the profiler).

`--rnn_type gru`: GRU memories; the on leg then also sets `fused_gru_memories` (csrc/lt_memory_gru.hip), the off leg is the eager loop
through `nn.GRU`, and the file is profiles/recurrent_rollout_gru_<n>.json.

    python tools/recurrent_rollout_bench.py [--envs 4096] [--rounds 7] [--rnn_type lstm] [--out profiles/recurrent_rollout_4096.json]
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
HIDDEN = 256


def stats(xs: list[float]) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def make_runner(envs: int, on: bool, rnn_type: str = "lstm"):
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    cfg = dict(train_cfg(TASK), fused_recurrent_rollout=on)
    if rnn_type == "gru":
        cfg["fused_gru_memories"] = on
    cfg["policy"] = dict(cfg["policy"], class_name="ActorCriticRecurrent", rnn_type=rnn_type, rnn_hidden_size=HIDDEN, rnn_num_layers=1)
    return OnPolicyRunner(make(TASK, num_envs=envs, device="cuda:0", seed=1), cfg, log_dir=None, device="cuda:0")


def eager_rollout(runner, obs, critic_obs):
    """The rollout part of the runner's eager loop (rl/runner.py `learn`), without its episode statistics."""
    import torch

    env, alg = runner.env, runner.alg
    with torch.inference_mode():
        for _ in range(runner.num_steps_per_env):
            actions = alg.act(obs, critic_obs)
            obs, rewards, dones, infos = env.step(actions)
            critic_obs = infos["observations"]["critic"]
            alg.process_env_step(rewards, dones, infos)
    alg.storage.clear()
    return obs, critic_obs


def measure(mode: str, envs: int, rounds: int, warmup: int, rnn_type: str = "lstm") -> dict:
    import torch

    on = mode != "off"
    runner = make_runner(envs, on, rnn_type)
    T = runner.num_steps_per_env
    fused = runner._make_fused()
    assert (fused is not None) == on
    out = {"mode": mode, "steps": T, "launches_per_step": fused.launches_per_step if on else None}
    obs, extras = runner.env.get_observations()
    critic_obs = extras["observations"]["critic"]
    runner.train_mode()
    if on:
        fused.begin()
    times = []
    for r in range(warmup + rounds if mode != "trace" else 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if on:
            fused.rollout(T)
        else:
            obs, critic_obs = eager_rollout(runner, obs, critic_obs)
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    if mode == "trace":
        return out
    out["rollout_ms"] = stats(times)
    if on:  # the same rollout as one hipGraph, replayed
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fused.rollout(T)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fused.rollout(T)
        times = []
        for r in range(warmup + rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            if r >= warmup:
                times.append(a.elapsed_time(b))
        out["rollout_graph_ms"] = stats(times)
    runner.learn(warmup + rounds)
    recs = runner.history[warmup:]
    out["iteration_ms"] = stats([1e3 * (r["Perf/collection time"] + r["Perf/learning_time"]) for r in recs])
    out["collection_ms"] = stats([1e3 * r["Perf/collection time"] for r in recs])
    return out


def kernel_trace(envs: int, rnn_type: str = "lstm") -> dict:
    """The memory-step kernel's own time: a `rocprofv3 --kernel-trace --stats` run of three fused rollouts, nothing else traced."""
    kernel = "lt_memory_step_kernel"  # both cells: the cell is a template argument of the one kernel (csrc/lt_memory_tile.h)
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="recurrent_trace_")
    try:
        p = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable,
                            os.path.abspath(__file__), "--mode", "trace", "--envs", str(envs), "--rnn_type", rnn_type], capture_output=True, text=True,
                           timeout=600)
        if p.returncode != 0:
            return {"error": f"rocprofv3 exit {p.returncode}: {p.stderr[-500:]}"}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if kernel in row.get("Name", ""):
                    return {"kernel": row["Name"], "calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                            "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        return {"error": f"no {kernel} row in the kernel statistics"}
    except (OSError, subprocess.TimeoutExpired, KeyError, ValueError) as exc:
        return {"error": f"{type(exc).__name__}: {exc}"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rnn_type", choices=["lstm", "gru"], default="lstm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--mode", choices=["off", "on", "trace"], help="(internal) measure one leg and print it")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("--rounds must be at least 5")
    if args.mode:
        print("RESULT " + json.dumps(measure(args.mode, args.envs, args.rounds, args.warmup, args.rnn_type)))
        return
    legs = {}
    for mode in ("off", "on"):  # a fresh process each: no allocator or graph state carried from one to the next
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(args.envs), "--rounds", str(args.rounds),
                            "--warmup", str(args.warmup), "--rnn_type", args.rnn_type], capture_output=True, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{mode}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        legs[mode] = json.loads(line[-1][7:])
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None

    def faster(key):  # on is faster by MORE than the spread of either leg: the intervals [min, max] do not even touch
        return legs["on"][key]["max"] < legs["off"][key]["min"]

    res = {"task": TASK, "envs": args.envs, "hidden": HIDDEN, "rnn_type": args.rnn_type, "measured_on_commit": args.commit or commit,
           "notes": {"off": "the switch off: the runner's eager loop, the same code as before the switch existed",
                     "rollout_ms": "host wall clock of one rollout between two device synchronisations",
                     "iteration_ms": "runner wall clock, collection + learning (the update ends in a host read)",
                     "spread": "min and max over the rounds, beside the median"},
           **legs, "memory_step_kernel": None if args.no_trace else kernel_trace(args.envs, args.rnn_type),
           "off_over_on_rollout": legs["off"]["rollout_ms"]["median"] / legs["on"]["rollout_ms"]["median"],
           "off_over_on_iteration": legs["off"]["iteration_ms"]["median"] / legs["on"]["iteration_ms"]["median"],
           "on_faster_than_the_spread": {"rollout": faster("rollout_ms"), "iteration": faster("iteration_ms")}}
    out = args.out or os.path.join(REPO, "profiles", f"recurrent_rollout_{'gru_' if args.rnn_type == 'gru' else ''}{args.envs}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
