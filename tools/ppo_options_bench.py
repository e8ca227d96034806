"""What `noise_std_type="log"` and `normalize_advantage_per_mini_batch` cost a training iteration: writes profiles/ppo_options_<n>.json.

Teacher task, `--envs` envs (4096) x 24 steps, the registered agent cfg (feed-forward ActorCritic [512, 256, 128], 5 epochs x 4
minibatches, adaptive schedule).  Four legs, one fresh process each, `--warmup` (3) iterations, then the median of `--rounds` (7) with
[min, max]:
  scalar  the registered cfg as it is (the control)
  log     policy noise_std_type = "log"
  norm    algorithm normalize_advantage_per_mini_batch = True
  both
and per leg
  rollout_ms    `Perf/collection time` of `runner.learn` (host wall clock of the rollout and compute_returns)
  update_ms     `Perf/learning_time` (host wall clock of `alg.update()`, which ends in a host read)
  iteration_ms  their sum
The tool uses the public runner interface alone, so the same file measures a tree that serves the options on the fused path and one that
does not: THE BASELINE LEGS ARE THE PARENT COMMIT'S - run `--leg scalar|log|norm|both` in a checkout of the parent, collect the four
RESULT lines in one file and hand it to `--off-result`; without it the file holds this tree's legs alone and says so.  Two statements
are drawn, neither against a threshold set in advance: whether the control's [min, max] on this tree overlaps the parent's (the
no-regression condition), and per option leg the parent's median over this tree's with both intervals beside it.

Two processes a minute apart can differ by a few percent in clocks alone, and the parent's legs necessarily run before or after this
tree's.  `--control-runs FILE` therefore takes RESULT lines of the control leg run ALTERNATELY on the two trees (`--leg scalar --label
this`, `--leg scalar --label parent`, ... in that order) and records them with the overlap of every neighbouring pair.

    python tools/ppo_options_bench.py [--envs 4096] [--rounds 7] [--off-result FILE] [--control-runs FILE] [--out profiles/ppo_options_4096.json]
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
LEGS = {"scalar": (False, False), "log": (True, False), "norm": (False, True), "both": (True, True)}  # leg -> (log std, per-minibatch norm)
KEYS = ("rollout_ms", "update_ms", "iteration_ms")


def stats(xs: list[float]) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def tree() -> str | None:
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def measure(leg: str, envs: int, rounds: int, warmup: int, label: str | None = None) -> dict:
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    log, norm = LEGS[leg]
    cfg = train_cfg(TASK)
    cfg["policy"] = dict(cfg["policy"], noise_std_type="log" if log else "scalar")
    cfg["algorithm"] = dict(cfg["algorithm"], normalize_advantage_per_mini_batch=norm)
    runner = OnPolicyRunner(make(TASK, num_envs=envs, device="cuda:0", seed=1), cfg, log_dir=None, device="cuda:0")
    alg = runner.alg
    out = {"leg": leg, "tree": label or tree(), "fused_rollout": runner._make_fused() is not None, "steps": runner.num_steps_per_env,
           "num_mini_batches": alg.num_mini_batches, "num_learning_epochs": alg.num_learning_epochs}
    runner.learn(warmup + rounds)
    recs = runner.history[warmup:]
    out["rollout_ms"] = stats([1e3 * r["Perf/collection time"] for r in recs])
    out["update_ms"] = stats([1e3 * r["Perf/learning_time"] for r in recs])
    out["iteration_ms"] = stats([1e3 * (r["Perf/collection time"] + r["Perf/learning_time"]) for r in recs])
    return out


def overlap(a: dict, b: dict) -> bool:
    return a["min"] <= b["max"] and b["min"] <= a["max"]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--off-result", help="file holding the RESULT lines of `--leg ...` run in a checkout of the parent commit")
    ap.add_argument("--control-runs", help="file holding RESULT lines of `--leg scalar --label this|parent`, run alternately")
    ap.add_argument("--leg", choices=list(LEGS), help="measure one leg in this process and print its RESULT line")
    ap.add_argument("--label", help="with --leg: what to record as the leg's tree (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("--rounds must be at least 5")
    if args.leg:
        print("RESULT " + json.dumps(measure(args.leg, args.envs, args.rounds, args.warmup, args.label)))
        return
    legs, parent = {}, None
    if args.off_result:
        parent = {}
        for line in open(args.off_result).read().splitlines():
            if line.startswith("RESULT "):
                rec = json.loads(line[7:])
                parent[rec["leg"]] = rec
        if set(parent) != set(LEGS):
            sys.exit(f"{args.off_result}: RESULT lines of {sorted(set(LEGS) - set(parent))} are missing")
    for leg in LEGS:  # a fresh process each: no allocator state carried from one to the next
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--envs", str(args.envs), "--rounds", str(args.rounds),
                            "--warmup", str(args.warmup), "--label", "this"], capture_output=True, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{leg}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        legs[leg] = json.loads(line[-1][7:])
    res = {"task": TASK, "envs": args.envs, "measured_on_commit": args.commit or tree(),
           "notes": {"rollout_ms": "runner wall clock of the rollout and compute_returns", "update_ms": "runner wall clock of alg.update() (it ends in a host read)",
                     "iteration_ms": "their sum", "spread": "min and max over the rounds, beside the median",
                     "parent": "the same tool run leg by leg in a checkout of the parent commit (--off-result); null: not measured"},
           "legs": legs, "parent": parent}
    if parent is not None:
        res["control_intervals_overlap"] = {k: overlap(legs["scalar"][k], parent["scalar"][k]) for k in KEYS}
        res["parent_over_this_tree"] = {leg: {k: {"ratio_of_medians": parent[leg][k]["median"] / legs[leg][k]["median"],
                                                  "parent": [parent[leg][k]["min"], parent[leg][k]["max"]],
                                                  "this_tree": [legs[leg][k]["min"], legs[leg][k]["max"]],
                                                  "intervals_overlap": overlap(legs[leg][k], parent[leg][k])} for k in KEYS}
                                        for leg in ("log", "norm", "both")}
    if args.control_runs:
        runs = [json.loads(l[7:]) for l in open(args.control_runs).read().splitlines() if l.startswith("RESULT ")]
        if len(runs) < 2 or any(r["leg"] != "scalar" for r in runs) or any(a["tree"] == b["tree"] for a, b in zip(runs, runs[1:])):
            sys.exit(f"{args.control_runs}: needs RESULT lines of the scalar leg that alternate between two labels")
        res["control_alternating"] = {"runs": [{"tree": r["tree"], **{k: r[k] for k in KEYS}} for r in runs],
                                      "every_neighbouring_pair_overlaps": {k: all(overlap(a[k], b[k]) for a, b in zip(runs, runs[1:])) for k in KEYS}}
    out = args.out or os.path.join(REPO, "profiles", f"ppo_options_{args.envs}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
