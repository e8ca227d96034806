"""What the PPO update of a recurrent (LSTM) policy costs with `fused_recurrent_update` off and on: writes profiles/recurrent_update_<n>.json.

Teacher task, `--envs` envs (4096), `ActorCriticRecurrent` with LSTM memories of H = 256, 24 steps per rollout, the recurrent runner cfg
(the fused rollout in both legs, so that the legs differ in the update alone); one fresh process per leg, `--warmup` (3) iterations, then
the median of `--rounds` (7) with [min, max]:
  update_ms     `Perf/learning_time` of `runner.learn` (host wall clock of `alg.update()`, which ends in a host read)
  iteration_ms  collection + learning time
The tool uses the public runner / PPO interface alone, and a tree without the switch ignores the cfg key: THE BASELINE LEG IS THE PARENT
COMMIT - run `--mode off` in a checkout of the parent and hand its RESULT line to `--off-result`; without it the off leg runs on this
tree with the switch off (the same code path, `_eager_update`), and the file says which tree each leg ran on.
The two new kernels' per-launch time comes from a `rocprofv3 --kernel-trace --stats` run of its own (`--mode trace` under the profiler,
no counters in it).  A gain is claimed only where the legs' [min, max] intervals do not overlap.

`--rnn_type gru`: GRU memories; both legs set `fused_gru_memories` (a tree without the key ignores it and collects in the eager loop:
`update_ms` is the figure that compares), the off leg updates through `nn.GRU` on padded trajectories, the on leg through
csrc/lt_memory_gru.hip, and the file is profiles/recurrent_update_gru_<n>.json.

`--direct`: the third leg, `direct_recurrent_update` on top of `fused_recurrent_update` (rl/ppo.py `_direct_recurrent_update`).  The legs are
then `on` (this tree, the key off) and `direct` (the key on), the baseline is `--mode on` run in a checkout of the parent commit and handed
to `--off-result`, the trace run is of the direct leg and records the dx hop's kernel (csrc/lt_mlp_dx.hip) with its share of all kernel
time, and the file is profiles/recurrent_update_direct_[gru_]<n>.json.

    python tools/recurrent_update_bench.py [--envs 4096] [--rounds 7] [--rnn_type lstm] [--direct] [--off-result FILE] [--out profiles/recurrent_update_4096.json]
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
HIDDEN = 256
# (one set of kernel templates serves both cells, csrc/lt_memory_tile.h: the cell is a template argument in the traced name)
KERNELS = {rnn: ("lt_memory_step_kernel", "lt_memory_seq_bwd_kernel", "lt_memory_seq_bwd_open_kernel", "lt_mlp_dx_kernel") for rnn in ("lstm", "gru")}


def stats(xs: list[float]) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def tree() -> str | None:
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def make_runner(envs: int, on: bool, rnn_type: str = "lstm", direct: bool = False):
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    cfg = dict(train_cfg(TASK), fused_recurrent_rollout=True, fused_recurrent_update=on)
    if rnn_type == "gru":
        cfg["fused_gru_memories"] = True
    if direct:
        cfg["direct_recurrent_update"] = True
    cfg["policy"] = dict(cfg["policy"], class_name="ActorCriticRecurrent", rnn_type=rnn_type, rnn_hidden_size=HIDDEN, rnn_num_layers=1)
    return OnPolicyRunner(make(TASK, num_envs=envs, device="cuda:0", seed=1), cfg, log_dir=None, device="cuda:0")


def measure(mode: str, envs: int, rounds: int, warmup: int, rnn_type: str = "lstm") -> dict:
    runner = make_runner(envs, mode != "off", rnn_type, direct=mode in ("direct", "trace_direct"))
    alg = runner.alg
    out = {"mode": mode, "tree": tree(), "switch": bool(getattr(alg, "fused_recurrent_update", False)),
           "direct": bool(getattr(alg, "direct_recurrent_update", False)), "steps": runner.num_steps_per_env,
           "num_mini_batches": alg.num_mini_batches, "num_learning_epochs": alg.num_learning_epochs}
    if mode in ("trace", "trace_direct"):
        runner.learn(2)
        return out
    runner.learn(warmup + rounds)
    recs = runner.history[warmup:]
    out["update_ms"] = stats([1e3 * r["Perf/learning_time"] for r in recs])
    out["iteration_ms"] = stats([1e3 * (r["Perf/collection time"] + r["Perf/learning_time"]) for r in recs])
    return out


def kernel_trace(envs: int, rnn_type: str = "lstm", mode: str = "trace") -> dict:
    """Per-launch time of the sequence kernels (`trace_direct`: and of the dx hop, with each kernel's share of all kernel time): a
    `rocprofv3 --kernel-trace --stats` run of two iterations, nothing else traced."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="recurrent_update_trace_")
    try:
        p = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable,
                            os.path.abspath(__file__), "--mode", mode, "--envs", str(envs), "--rnn_type", rnn_type], capture_output=True, text=True,
                           timeout=600)
        if p.returncode != 0:
            return {"error": f"rocprofv3 exit {p.returncode}: {p.stderr[-500:]}"}
        rows, total_ns = {}, 0.0
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                total_ns += int(row["Calls"]) * float(row["AverageNs"])
                if any(k in row.get("Name", "") for k in KERNELS[rnn_type]):
                    rows[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                         "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        for r in rows.values():  # of the whole traced run (two iterations, rollouts included)
            r["share_of_kernel_time"] = r["calls"] * r["average_us"] * 1e3 / total_ns
        return rows or {"error": "no sequence-kernel row in the kernel statistics"}
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
    ap.add_argument("--off-result", help="file holding the RESULT line of `--mode off` run in a checkout of the parent commit")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--direct", action="store_true", help="compare `direct_recurrent_update` on with it off (baseline: the parent's `--mode on`)")
    ap.add_argument("--mode", choices=["off", "on", "direct", "trace", "trace_direct"], help="(internal) measure one leg and print it")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("--rounds must be at least 5")
    if args.mode:
        print("RESULT " + json.dumps(measure(args.mode, args.envs, args.rounds, args.warmup, args.rnn_type)))
        return
    base, new = ("on", "direct") if args.direct else ("off", "on")  # the leg a gain is measured against, and the leg that is new
    legs = {}
    if args.off_result:
        line = [l for l in open(args.off_result).read().splitlines() if l.startswith("RESULT ")]
        if not line:
            sys.exit(f"{args.off_result}: no RESULT line")
        legs["baseline" if args.direct else "off"] = json.loads(line[-1][7:])
    for mode in (base, new):  # a fresh process each: no allocator state carried from one to the next
        if mode in legs:
            continue
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(args.envs), "--rounds", str(args.rounds),
                            "--warmup", str(args.warmup), "--rnn_type", args.rnn_type], capture_output=True, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{mode}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        legs[mode] = json.loads(line[-1][7:])
    if (not args.direct and legs["off"]["switch"]) or not legs["on"]["switch"]:
        sys.exit("the off leg ran with the switch on, or the on leg without it")
    if args.direct and (legs["on"].get("direct") or not legs["direct"]["direct"] or legs.get("baseline", legs["on"]).get("direct")):
        sys.exit("the direct leg ran without its key, or another leg with it")

    def faster(key, than=base):  # faster by MORE than the spread of either leg: the intervals [min, max] do not even touch
        return legs[new][key]["max"] < legs[than][key]["min"]

    res = {"task": TASK, "envs": args.envs, "hidden": HIDDEN, "rnn_type": args.rnn_type, "measured_on_commit": args.commit or tree(),
           "notes": {"off": "the parent commit's tree where `tree` differs from the on leg's; else this tree with the switch off",
                     "update_ms": "runner wall clock of alg.update() (it ends in a host read)",
                     "iteration_ms": "runner wall clock, collection + learning",
                     "spread": "min and max over the rounds, beside the median"},
           **legs, "kernels": None if args.no_trace else kernel_trace(args.envs, args.rnn_type, "trace_direct" if args.direct else "trace"),
           f"{base}_over_{new}_update": legs[base]["update_ms"]["median"] / legs[new]["update_ms"]["median"],
           f"{base}_over_{new}_iteration": legs[base]["iteration_ms"]["median"] / legs[new]["iteration_ms"]["median"],
           f"{new}_faster_than_the_spread": {"update": faster("update_ms"), "iteration": faster("iteration_ms")}}
    if args.direct:
        res["notes"]["baseline"] = "`--mode on` (fused_recurrent_update alone) in a checkout of the parent commit, through --off-result; absent: not measured"
        if "baseline" in legs:
            res["direct_faster_than_the_baseline_spread"] = {k: faster(k + "_ms", "baseline") for k in ("update", "iteration")}
    name = "recurrent_update_direct_" if args.direct else "recurrent_update_"
    out = args.out or os.path.join(REPO, "profiles", f"{name}{'gru_' if args.rnn_type == 'gru' else ''}{args.envs}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
