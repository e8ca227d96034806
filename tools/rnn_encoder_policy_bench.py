"""What an iteration of an `ActorCriticRNNEncoder` teacher costs with `fused_rnn_encoder_policy` off and on: writes
profiles/rnn_encoder_policy_<n>.json.

Teacher task, `--envs` envs (4096) x 24 steps, the shape of the reference's RNN-encoder teacher cfg (rows of 348 columns, head 270, the
last 78 through a GRU of 256 and then 256 -> 128 -> 64 -> 64, ELU, tanh behind the embedding; the critic of the same form; the stacks
of the registered cfg); one fresh process per leg, `--warmup` (3) iterations, then the median of `--rounds` (7) with [min, max]:
  rollout_ms    `Perf/collection time` of `runner.learn` (rollout + compute_returns, host wall clock)
  update_ms     `Perf/learning_time` (host wall clock of `alg.update()`: the eager recurrent update in both legs)
  iteration_ms  their sum
Legs: `off` (the key off: the eager torch loop, the only other implementation of this class) and `on` (the key on: four launches per
step, rl/fused.py).  The memory-step and encoder kernels' own time comes from a `rocprofv3 --kernel-trace --stats` run of its own
(`--mode trace` under the profiler, no counters in it).  No speed-up is fixed in advance: a gain is claimed only where the [min, max]
intervals of both legs do not overlap.

Controls: the memory kernel's addressing changed with this class (a row stride), so `--controls DIR` takes the outputs of two
programs run on the parent commit and on this tree, and records them and whether their [min, max] intervals overlap:
  {parent,tree}_recurrent_{lstm,gru}*.txt  the RESULT line of `tools/recurrent_rollout_bench.py --mode on [--rnn_type gru]`, one file per run
  {parent,tree}_bench_<i>.txt              the JSON line of `bench.py --gpus 1 --steps 20 --warmup 5`, one file per run
Without the directory the file says "not measured".

    python tools/rnn_encoder_policy_bench.py [--envs 4096] [--rounds 7] [--controls DIR] [--out profiles/rnn_encoder_policy_4096.json]

`--update` measures the UPDATE key instead, `direct_rnn_encoder_update` (rl/ppo.py `_direct_rnn_encoder_update`), and writes
profiles/rnn_encoder_update_<n>.json: the rollout key is on in both legs, `update_off` runs the eager recurrent update and `update_on`
the graph-free one; the traced kernels are then `lt_rnn_encoder_backward_kernel` and `lt_encoder_kernel`.  The parent commit has no such
key: its `--mode on` run IS the off leg, so the controls directory also takes
  parent_update*.txt                       the RESULT line of this tool's `--mode on` run on the parent commit's tree, one file per run
and the file records whether its update and iteration intervals overlap this tree's `update_off` leg.
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
POLICY = dict(class_name="ActorCriticRNNEncoder", actor_flatten_obs_end_idx=270, actor_encoder_obs_start_idx=270,
              actor_encoder_hidden_dims=[256, 128, 64], actor_encoder_embedding_dim=64, critic_flatten_obs_end_idx=270,
              critic_encoder_obs_start_idx=270, critic_encoder_hidden_dims=[256, 128, 64], critic_encoder_embedding_dim=64,
              encoder_rnn_type="gru", encoder_rnn_hidden_size=256, encoder_rnn_num_layers=1, encoder_activation="elu",
              encoder_final_activation="tanh")
KEYS = ("rollout_ms", "update_ms", "iteration_ms")
KERNELS = ("lt_memory_step_kernel", "lt_encoder_kernel")
UPDATE_KERNELS = ("lt_rnn_encoder_backward_kernel", "lt_encoder_kernel")
CONTROL_KEYS = ("rollout_ms", "rollout_graph_ms", "iteration_ms")


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
    cfg["policy"] = dict(cfg["policy"], **POLICY)
    cfg["fused_rnn_encoder_policy"] = mode != "off"
    if mode in ("update_on", "update_trace"):
        cfg["direct_rnn_encoder_update"] = True
    return OnPolicyRunner(make(TASK, num_envs=envs, device="cuda:0", seed=1), cfg, log_dir=None, device="cuda:0")


def measure(mode: str, envs: int, rounds: int, warmup: int, commit: str | None = None) -> dict:
    runner = make_runner(envs, mode)
    alg, fused = runner.alg, runner._make_fused()
    out = {"mode": mode, "tree": commit or tree(), "policy": type(alg.actor_critic).__name__, "key": bool(runner.cfg.get("fused_rnn_encoder_policy")),
           "update_key": bool(runner.cfg.get("direct_rnn_encoder_update")), "fused_rollout": fused is not None, "launches_per_step": fused.launches_per_step if fused is not None else None,
           "steps": runner.num_steps_per_env, "num_mini_batches": alg.num_mini_batches, "num_learning_epochs": alg.num_learning_epochs}
    if mode.endswith("trace"):
        runner.learn(2)
        return out
    runner.learn(warmup + rounds)
    recs = runner.history[warmup:]
    out["rollout_ms"] = stats([1e3 * r["Perf/collection time"] for r in recs])
    out["update_ms"] = stats([1e3 * r["Perf/learning_time"] for r in recs])
    out["iteration_ms"] = stats([1e3 * (r["Perf/collection time"] + r["Perf/learning_time"]) for r in recs])
    return out


def kernel_trace(envs: int, mode: str = "trace", kernels=KERNELS) -> dict:
    """Per-launch time of `kernels` (the memory-step and encoder kernels; with `mode="update_trace"` the encoder's backward and forward
    kernels) and their share of all kernel time: a `rocprofv3 --kernel-trace --stats` run of two iterations with the key(s) on, nothing
    else traced."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="rnn_encoder_policy_trace_")
    try:
        p = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable,
                            os.path.abspath(__file__), "--mode", mode, "--envs", str(envs)], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            return {"error": f"rocprofv3 exit {p.returncode}: {p.stderr[-500:]}"}
        rows, total_ns = {}, 0.0
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                total_ns += int(row["Calls"]) * float(row["AverageNs"])
                if any(k in row.get("Name", "") for k in kernels):
                    rows[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                         "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        for r in rows.values():  # of the whole traced run (two iterations: the rollout's launches; the eager update launches neither kernel)
            r["share_of_kernel_time"] = r["calls"] * r["average_us"] * 1e3 / total_ns
        return rows or {"error": "no row of the kernels in the kernel statistics"}
    except (OSError, subprocess.TimeoutExpired, KeyError, ValueError) as exc:
        return {"error": f"{type(exc).__name__}: {exc}"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def overlap(a: dict, b: dict) -> bool:
    return a["min"] <= b["max"] and b["min"] <= a["max"]


def controls(d: str | None):
    """The control runs of both trees out of `d` (module docstring) and whether their intervals overlap."""
    if not d:
        return "not measured"
    out = {}
    for cell in ("lstm", "gru"):
        legs = {}
        for side in ("parent", "tree"):  # every run of a side is kept (a fresh process each); the side's interval is the hull of its runs
            runs = []
            for path in sorted(glob.glob(os.path.join(d, f"{side}_recurrent_{cell}*.txt"))):
                line = [l for l in open(path).read().splitlines() if l.startswith("RESULT ")]
                if line:
                    runs.append(json.loads(line[-1][7:]))
            if runs:
                legs[side] = {"runs": runs, **{k: {"min": min(r[k]["min"] for r in runs), "max": max(r[k]["max"] for r in runs)} for k in CONTROL_KEYS}}
        entry = dict(legs)
        if len(legs) == 2:
            entry["intervals_overlap"] = {k: overlap(legs["parent"][k], legs["tree"][k]) for k in CONTROL_KEYS}
        out[f"recurrent_rollout_{cell}"] = entry or "not measured"
    bench = {}
    for side in ("parent", "tree"):
        vals = []
        for path in sorted(glob.glob(os.path.join(d, f"{side}_bench_*.txt"))):
            for l in open(path).read().splitlines():
                if l.startswith("{") and '"value"' in l:
                    vals.append(json.loads(l)["value"])
        if vals:
            bench[side] = dict(stats(vals), unit="env-steps/s", command="bench.py --gpus 1 --steps 20 --warmup 5")
    if len(bench) == 2:
        bench["intervals_overlap"] = overlap(bench["parent"], bench["tree"])
    out["bench"] = bench or "not measured"
    runs = []  # the update leg's baseline: this tool's `--mode on` on the parent commit's tree
    for path in sorted(glob.glob(os.path.join(d, "parent_update*.txt"))):
        line = [l for l in open(path).read().splitlines() if l.startswith("RESULT ")]
        if line:
            runs.append(json.loads(line[-1][7:]))
    if runs:
        out["parent_update_off"] = {"runs": runs, **{k: {"min": min(r[k]["min"] for r in runs), "max": max(r[k]["max"] for r in runs)} for k in KEYS}}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--controls", help="directory with the control runs of the parent commit and of this tree (module docstring)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--update", action="store_true", help="measure the update key direct_rnn_encoder_update (rollout key on in both legs)")
    ap.add_argument("--mode", choices=["off", "on", "trace", "update_off", "update_on", "update_trace"], help="(internal) measure one leg and print it")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("--rounds must be at least 5")
    if args.mode:
        print("RESULT " + json.dumps(measure(args.mode, args.envs, args.rounds, args.warmup, args.commit)))
        return
    if args.update:
        return main_update(args)
    legs = {}
    for mode in ("off", "on"):  # a fresh process each: no allocator state carried from one to the next
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(args.envs), "--rounds", str(args.rounds),
                            "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{mode}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        legs[mode] = json.loads(line[-1][7:])
    if legs["off"]["key"] or legs["off"]["fused_rollout"] or not (legs["on"]["key"] and legs["on"]["fused_rollout"]):
        sys.exit("a leg ran on another path than its name says")

    def outside(key):  # faster by MORE than the spread of either leg: the intervals [min, max] do not even touch
        return legs["on"][key]["max"] < legs["off"][key]["min"]

    res = {"task": TASK, "envs": args.envs, "policy": POLICY, "measured_on_commit": args.commit or tree(),
           "notes": {"off": "the key off: the runner's eager torch loop, the only other implementation of this class",
                     "rollout_ms": "runner wall clock of the rollout and compute_returns",
                     "update_ms": "runner wall clock of alg.update(): the eager recurrent update in both legs",
                     "iteration_ms": "their sum",
                     "spread": "min and max over the rounds, beside the median"},
           **legs, "kernels": None if args.no_trace else kernel_trace(args.envs),
           "off_over_on": {k[:-3]: legs["off"][k]["median"] / legs["on"][k]["median"] for k in KEYS},
           "on_faster_than_the_spread": {k[:-3]: outside(k) for k in KEYS},
           "controls": controls(args.controls)}
    out = args.out or os.path.join(REPO, "profiles", f"rnn_encoder_policy_{args.envs}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main_update(args) -> None:
    """The update key's file: legs `update_off` / `update_on`, the new kernel's own time, the controls."""
    legs = {}
    for mode in ("update_off", "update_on"):  # a fresh process each; `--commit` names the tree in each leg's record as well
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(args.envs), "--rounds", str(args.rounds),
                            "--warmup", str(args.warmup)] + (["--commit", args.commit] if args.commit else []),
                           capture_output=True, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{mode}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        legs[mode] = json.loads(line[-1][7:])
    off, on = legs["update_off"], legs["update_on"]
    if off["update_key"] or not on["update_key"] or not (off["fused_rollout"] and on["fused_rollout"]):
        sys.exit("a leg ran on another path than its name says")
    ctl = controls(args.controls)
    parent = ctl.get("parent_update_off") if isinstance(ctl, dict) else None
    res = {"task": TASK, "envs": args.envs, "policy": POLICY, "measured_on_commit": args.commit or tree(),
           "notes": {"update_off": "fused_rnn_encoder_policy on, direct_rnn_encoder_update off: the eager recurrent update",
                     "update_on": "both keys on: rl/ppo.py _direct_rnn_encoder_update",
                     "update_ms": "runner wall clock of alg.update()", "iteration_ms": "rollout + update",
                     "spread": "min and max over the rounds, beside the median",
                     "parent_update_off": "the parent commit's tree, which has no update key: its eager update, the off baseline"},
           **legs, "kernels": None if args.no_trace else kernel_trace(args.envs, "update_trace", UPDATE_KERNELS),
           "off_over_on": {k[:-3]: off[k]["median"] / on[k]["median"] for k in KEYS},
           "on_faster_than_the_spread": {k[:-3]: on[k]["max"] < off[k]["min"] for k in KEYS},
           "off_overlaps_parent": {k[:-3]: overlap(parent[k], off[k]) for k in KEYS} if parent else "not measured",
           "on_faster_than_parent_spread": {k[:-3]: on[k]["max"] < parent[k]["min"] for k in KEYS} if parent else "not measured",
           "controls": ctl}
    out = args.out or os.path.join(REPO, "profiles", f"rnn_encoder_update_{args.envs}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
