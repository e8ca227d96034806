"""What `empirical_normalization` costs on the fused rollout path, and what it cost before: writes profiles/obs_norm_4096.json.

Teacher task, 4096 envs, three runner configurations on the same card in one session:
  off    switch off (every shipped agent cfg): the two-launch rollout step
  fused  switch on, fused rollout with the device normaliser (csrc/lt_obs_norm.hip): four launches per step
  eager  switch on, `fused_rollout=False`: the reference-shaped eager loop with the torch normaliser - the path a runner with the
         switch set took before the device normaliser existed (rl/runner.py's eager loop is the same code)
Rollout: the 24-step rollout captured into one hipGraph, warm, `--replays` replays timed one by one with events, median, per step
(eager: the runner's own collection time, it cannot be captured - the torch normaliser reads `count` on the host).
Iteration: median of the runner's collection + learning time over `--iters` iterations behind `--warmup` warm-up iterations.

    python tools/obs_norm_bench.py [--envs 4096] [--replays 30] [--iters 20] [--out profiles/obs_norm_4096.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"


def measure(mode: str, envs: int, replays: int, iters: int, warmup: int) -> dict:
    import torch

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    cfg = dict(train_cfg(TASK), empirical_normalization=mode != "off", fused_rollout=mode != "eager")
    runner = OnPolicyRunner(make(TASK, num_envs=envs, device="cuda:0", seed=1), cfg, log_dir=None, device="cuda:0")
    T = runner.num_steps_per_env
    out = {"mode": mode, "launches_per_step": None}
    runner.learn(warmup + iters)
    recs = runner.history[warmup:]
    out["iteration_ms"] = 1e3 * statistics.median(r["Perf/collection time"] + r["Perf/learning_time"] for r in recs)
    out["collection_ms"] = 1e3 * statistics.median(r["Perf/collection time"] for r in recs)
    fused = runner._make_fused()
    assert (fused is None) == (mode == "eager")
    if fused is None:
        out["rollout_us_per_step"] = 1e3 * out["collection_ms"] / T
        out["rollout_timing"] = "runner collection time (host-driven, not capturable)"
        return out
    out["launches_per_step"] = fused.launches_per_step
    fused.begin()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.rollout(T)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused.rollout(T)
    for _ in range(5):
        graph.replay()
    times = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    out["rollout_us_per_step"] = 1e3 * statistics.median(times) / T
    out["rollout_timing"] = f"hipGraph of {T} steps, median of {replays} replays"
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "obs_norm_4096.json"))
    ap.add_argument("--commit", help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--mode", choices=["off", "fused", "eager"], help="(internal) measure one configuration and print it")
    args = ap.parse_args()
    if args.mode:
        print("RESULT " + json.dumps(measure(args.mode, args.envs, args.replays, args.iters, args.warmup)))
        return
    rows = {}
    for mode in ("off", "fused", "eager"):  # a fresh process each: no allocator or graph state carried from one to the next
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(args.envs), "--replays", str(args.replays),
                            "--iters", str(args.iters), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=600)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{mode}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        rows[mode] = json.loads(line[-1][7:])
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    notes = {"eager": "this tree with fused_rollout=False: the runner's eager loop; not a checkout of an earlier commit",
             "iteration_ms": "runner wall clock (time.time), collection + learning; like for like across the three rows",
             "rollout_us_per_step": "off / fused: event-timed hipGraph replay; eager: host wall clock of the collection / steps, no device "
                                    "sync - not the same clock, so fused_over_eager_rollout is indicative only",
             "collection_ms": "the runner launches fused.rollout() un-captured: host time, not the graph replay"}
    res = {"task": TASK, "envs": args.envs, "measured_on_commit": args.commit or commit, "notes": notes, **rows,
           "fused_over_eager_iteration": rows["eager"]["iteration_ms"] / rows["fused"]["iteration_ms"],
           "fused_over_eager_rollout": rows["eager"]["rollout_us_per_step"] / rows["fused"]["rollout_us_per_step"],
           "price_us_per_step": rows["fused"]["rollout_us_per_step"] - rows["off"]["rollout_us_per_step"],
           "price_iteration_ms": rows["fused"]["iteration_ms"] - rows["off"]["iteration_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
