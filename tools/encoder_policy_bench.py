"""What an iteration of an `ActorCriticEncoder` teacher costs with `fused_encoder_policy` off and on: writes profiles/encoder_policy_<n>.json.

Teacher task, `--envs` envs (4096) x 24 steps, the shape of the reference's teacher cfg (rows of 348 columns, head 270, the last 78
through 256 -> 128 -> 64 -> 64, ELU, tanh behind the embedding, a critic without an encoder; the stacks of the registered cfg); one fresh
process per leg, `--warmup` (3) iterations, then the median of `--rounds` (7) with [min, max]:
  rollout_ms    `Perf/collection time` of `runner.learn` (rollout + compute_returns, host wall clock)
  update_ms     `Perf/learning_time` (host wall clock of `alg.update()`, which ends in a host read)
  iteration_ms  their sum
Legs: `off` (the key off: the eager loop and the autograd op chain), `on` (the key on), `control` (the registered plain `ActorCritic`
cfg, which this change must not move).  The tool uses the public runner interface alone, and a tree without the key ignores it: THE
BASELINE IS THE PARENT COMMIT - run `--mode off` and `--mode control` in a checkout of the parent and hand their RESULT lines to
`--off-result` / `--control-result`; without them the file says so and the off leg of this tree stands alone.  The encoder kernel's own
time comes from a `rocprofv3 --kernel-trace --stats` run of its own (`--mode trace` under the profiler, no counters in it).  No speed-up
is fixed in advance: a gain is claimed only where the [min, max] intervals of both legs do not overlap, and the control's intervals on
the two trees are reported as overlapping or not.

    python tools/encoder_policy_bench.py [--envs 4096] [--rounds 7] [--off-result FILE] [--control-result FILE] [--out profiles/encoder_policy_4096.json]
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
ENCODER = dict(class_name="ActorCriticEncoder", actor_flatten_obs_end_idx=270, actor_encoder_obs_start_idx=270,
               actor_encoder_hidden_dims=[256, 128, 64], actor_encoder_embedding_dim=64, encoder_activation="elu", encoder_final_activation="tanh")
KEYS = ("rollout_ms", "update_ms", "iteration_ms")


def stats(xs: list[float]) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def tree() -> str | None:
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def make_runner(envs: int, mode: str):
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    cfg = dict(train_cfg(TASK))
    if mode != "control":
        cfg["policy"] = dict(cfg["policy"], **ENCODER)
        cfg["fused_encoder_policy"] = mode in ("on", "trace")
    return OnPolicyRunner(make(TASK, num_envs=envs, device="cuda:0", seed=1), cfg, log_dir=None, device="cuda:0")


def measure(mode: str, envs: int, rounds: int, warmup: int, commit: str | None = None) -> dict:
    runner = make_runner(envs, mode)
    alg = runner.alg
    out = {"mode": mode, "tree": commit or tree(), "policy": type(alg.actor_critic).__name__, "key": bool(getattr(alg, "fused_encoder_policy", False)),
           "fused_rollout": runner._make_fused() is not None, "steps": runner.num_steps_per_env, "num_mini_batches": alg.num_mini_batches,
           "num_learning_epochs": alg.num_learning_epochs}
    if mode == "trace":
        runner.learn(2)
        return out
    runner.learn(warmup + rounds)
    recs = runner.history[warmup:]
    out["rollout_ms"] = stats([1e3 * r["Perf/collection time"] for r in recs])
    out["update_ms"] = stats([1e3 * r["Perf/learning_time"] for r in recs])
    out["iteration_ms"] = stats([1e3 * (r["Perf/collection time"] + r["Perf/learning_time"]) for r in recs])
    return out


def kernel_trace(envs: int) -> dict:
    """Per-launch time of the encoder kernel and its share of all kernel time: a `rocprofv3 --kernel-trace --stats` run of two
    iterations with the key on, nothing else traced."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="encoder_policy_trace_")
    try:
        p = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable,
                            os.path.abspath(__file__), "--mode", "trace", "--envs", str(envs)], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            return {"error": f"rocprofv3 exit {p.returncode}: {p.stderr[-500:]}"}
        rows, total_ns = {}, 0.0
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                total_ns += int(row["Calls"]) * float(row["AverageNs"])
                if "lt_encoder_kernel" in row.get("Name", ""):
                    rows[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                         "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        for r in rows.values():  # of the whole traced run (two iterations; the rollout's launches and the update's have different row counts)
            r["share_of_kernel_time"] = r["calls"] * r["average_us"] * 1e3 / total_ns
        return rows or {"error": "no lt_encoder_kernel row in the kernel statistics"}
    except (OSError, subprocess.TimeoutExpired, KeyError, ValueError) as exc:
        return {"error": f"{type(exc).__name__}: {exc}"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def result_line(path: str) -> dict:
    line = [l for l in open(path).read().splitlines() if l.startswith("RESULT ")]
    if not line:
        sys.exit(f"{path}: no RESULT line")
    return json.loads(line[-1][7:])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--off-result", help="file holding the RESULT line of `--mode off` run in a checkout of the parent commit")
    ap.add_argument("--control-result", help="file holding the RESULT line of `--mode control` run in a checkout of the parent commit")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--mode", choices=["off", "on", "control", "trace"], help="(internal) measure one leg and print it")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("--rounds must be at least 5")
    if args.mode:
        print("RESULT " + json.dumps(measure(args.mode, args.envs, args.rounds, args.warmup, args.commit)))
        return
    legs = {}
    if args.off_result:
        legs["parent_off"] = result_line(args.off_result)
    if args.control_result:
        legs["parent_control"] = result_line(args.control_result)
    for mode in ("off", "on", "control"):  # a fresh process each: no allocator state carried from one to the next
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(args.envs), "--rounds", str(args.rounds),
                            "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{mode}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        legs[mode] = json.loads(line[-1][7:])
    if legs["off"]["key"] or legs["off"]["fused_rollout"] or not (legs["on"]["key"] and legs["on"]["fused_rollout"]) or legs["control"]["policy"] != "ActorCritic":
        sys.exit("a leg ran on another path than its name says")
    if any(legs.get(k, {}).get("key") for k in ("parent_off", "parent_control")):
        sys.exit("a parent leg ran with the key on")
    base = "parent_off" if "parent_off" in legs else "off"

    def outside(new, old, key):  # faster by MORE than the spread of either leg: the intervals [min, max] do not even touch
        return legs[new][key]["max"] < legs[old][key]["min"]

    def overlap(a, b, key):
        return legs[a][key]["min"] <= legs[b][key]["max"] and legs[b][key]["min"] <= legs[a][key]["max"]

    res = {"task": TASK, "envs": args.envs, "encoder": ENCODER, "measured_on_commit": args.commit or tree(),
           "notes": {"baseline": f"the `{base}` leg" + (": `--mode off` in a checkout of the parent commit" if base == "parent_off"
                                                       else ": this tree with the key off; the parent commit's leg was not measured"),
                     "rollout_ms": "runner wall clock of the rollout and compute_returns",
                     "update_ms": "runner wall clock of alg.update() (it ends in a host read)",
                     "iteration_ms": "their sum",
                     "spread": "min and max over the rounds, beside the median"},
           **legs, "kernels": None if args.no_trace else kernel_trace(args.envs),
           "baseline_over_on": {k[:-3]: legs[base][k]["median"] / legs["on"][k]["median"] for k in KEYS},
           "on_faster_than_the_spread": {k[:-3]: outside("on", base, k) for k in KEYS},
           "control_overlaps_parent": {k[:-3]: overlap("control", "parent_control", k) for k in KEYS} if "parent_control" in legs else "not measured"}
    out = args.out or os.path.join(REPO, "profiles", f"encoder_policy_{args.envs}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
