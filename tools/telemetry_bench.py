"""What the telemetry record of `--telemetry` and the strip charts of `--video_telemetry` cost in a `--video` play window; writes
profiles/telemetry_640x360.json.

    python tools/telemetry_bench.py [--out profiles/telemetry_640x360.json] [--no-trace] [--parent-json FILE]
    python tools/telemetry_bench.py --legs plain --no-trace --out FILE      # on a checkout of the parent commit: the no-flag leg alone

Frame 640x360, the teacher -Play- env with its registered env count (50), zero actions, the scripts' default channels (36) of env 0
and render.default_chart.  Two measurements, each in a fresh child process with a time limit of its own (this driver never opens the
GPU):
  kernels: the kernels' own time - lt_render_kernel, lt_telemetry_record_kernel, lt_telemetry_chart_kernel - from one
           `rocprofv3 --kernel-trace --stats` run of `--mode trace` (the program after `--`, no counters in the run).
  wall:    the per-step wall time of a `--video` recording window (env.step with the recorder attached: step, record, render, chart,
           copy to pinned host memory, deflate on the writer thread) for three legs - no flag, --telemetry, --telemetry
           --video_telemetry -, alternating, median [min, max] of 7 rounds of 100 steps, each round ending in a device synchronise.
`--legs plain` measures the first leg alone and imports nothing of the telemetry unit, so the same file runs on a checkout of the
parent commit; `--parent-json` takes that run's output and says whether the two no-flag intervals overlap (if they do not, the hook in
env.step is not free).  No speed is promised.
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
TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-Play-v1"
W, H = 640, 360
KERNELS = ("lt_render_kernel", "lt_telemetry_record_kernel", "lt_telemetry_chart_kernel")
LEGS = {"plain": (False, False), "telemetry": (True, False), "telemetry_chart": (True, True)}  # name -> (--telemetry, --video_telemetry)


def stats(xs) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def setup(leg: str, folder: str):
    """(env, recorder) of a recording whose video spans the whole measurement."""
    import torch

    from locotouch_amd.env import make
    from locotouch_amd.video import recorder_for

    record, chart = LEGS[leg]
    env = make(TASK, device="cuda:0", seed=1)
    act = torch.zeros(env.num_envs, 12, device="cuda:0")
    for _ in range(20):
        env.step(act)
    args = argparse.Namespace(video=True, video_length=10 ** 9, video_interval=10 ** 9, video_camera="follow", video_resolution=f"{W}x{H}",
                              video_tactile=False, video_telemetry=chart, telemetry=record, telemetry_envs="0", telemetry_capacity=4096)
    if not record:  # (nothing of the telemetry unit is imported: this leg also runs on the parent commit)
        return env, recorder_for(env, args, folder)
    from locotouch_amd.telemetry import DEFAULT_CHANNELS, telemetry_for

    args.telemetry_channels = ",".join(DEFAULT_CHANNELS)
    return env, recorder_for(env, args, folder, telemetry=telemetry_for(env, args))


def trace(steps: int) -> dict:
    """`steps` recorded env steps with both flags: under the profiler this is the run whose kernel statistics are read."""
    import torch

    from locotouch_amd import render as R

    tmp = tempfile.mkdtemp(prefix="telemetry_trace_")
    env, rec = setup("telemetry_chart", tmp)
    act = torch.zeros(env.num_envs, 12, device="cuda:0")
    for _ in range(steps):
        env.step(act)
    torch.cuda.synchronize()
    out = {"steps": steps, "chart_size": list(R.chart_size(R.default_chart(W, H))), "channels": len(env.telemetry.names), "envs_recorded": len(env.telemetry.env_ids)}
    rec.close(wait=False)
    shutil.rmtree(tmp, ignore_errors=True)
    return out


def wall(legs: list, rounds: int, steps: int, warmup: int) -> dict:
    import torch

    tmp = tempfile.mkdtemp(prefix="telemetry_wall_")
    made = {leg: setup(leg, os.path.join(tmp, leg)) for leg in legs}
    act = torch.zeros(made[legs[0]][0].num_envs, 12, device="cuda:0")
    times = {leg: [] for leg in legs}
    for r in range(warmup + rounds):
        for leg in legs:  # alternating: every leg sees the same machine
            env, _ = made[leg]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                env.step(act)
            torch.cuda.synchronize()
            if r >= warmup:
                times[leg].append((time.perf_counter() - t0) * 1e3 / steps)
    for _, rec in made.values():
        rec.close(wait=False)
    shutil.rmtree(tmp, ignore_errors=True)
    return {"device": torch.cuda.get_device_name(0), "envs": made[legs[0]][0].num_envs, "steps_per_round": steps,
            **{f"step_ms_{leg}": stats(times[leg]) for leg in legs}}


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
    rows = {}
    for path in glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in row.get("Name", ""):
                    rows[k] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                               "max_us": float(row["MaxNs"]) / 1e3}
    return rows


def overlap(a: dict, b: dict) -> bool:
    return a["min"] <= b["max"] and b["min"] <= a["max"]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", f"telemetry_{W}x{H}.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-steps", type=int, default=200)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated legs of the wall measurement: " + ", ".join(LEGS))
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--parent-json", default=None, help="the output of `--legs plain --no-trace` on a checkout of the parent commit")
    ap.add_argument("--mode", choices=["trace", "wall"], help="(internal) one measurement in this process; prints a RESULT line")
    args = ap.parse_args()
    legs = [leg for leg in args.legs.split(",") if leg]
    if args.mode == "trace":
        print("RESULT " + json.dumps(trace(args.trace_steps)))
        return
    if args.mode == "wall":
        print("RESULT " + json.dumps(wall(legs, args.rounds, args.steps, args.warmup)))
        return
    res = {"task": TASK, "frame": [W, H], "setup": "zero actions; the scripts' default channels of env 0; render.default_chart"}
    if args.no_trace:
        res["kernels"] = "not measured"
    else:
        tmp = tempfile.mkdtemp(prefix="telemetry_prof_")
        run = child("trace", ["--trace-steps", str(args.trace_steps)], 300, profiler_dir=tmp)
        rows = kernel_stats(tmp) if "error" not in run else {}
        shutil.rmtree(tmp, ignore_errors=True)
        res["kernels"] = {**run, **(rows or {"error": run.get("error", "no row of the three kernels in the kernel statistics")}),
                          "source": "rocprofv3 --kernel-trace --stats, one run, no counters"}
    res["wall"] = child("wall", ["--legs", ",".join(legs), "--rounds", str(args.rounds), "--steps", str(args.steps), "--warmup", str(args.warmup)], 420)
    res["wall_note"] = "per env step of a recording window: step (+ record), render (+ chart), copy to pinned host memory; deflate on the writer thread"
    if args.parent_json:
        parent = json.load(open(args.parent_json))
        res["parent_commit"] = {"wall": parent.get("wall"), "note": "the no-flag leg, measured with this tool on a checkout of the parent commit"}
        mine, theirs = res["wall"].get("step_ms_plain"), (parent.get("wall") or {}).get("step_ms_plain")
        if mine and theirs:
            res["parent_commit"]["no_flag_intervals_overlap"] = overlap(mine, theirs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
