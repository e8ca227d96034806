"""What the taxel panel of `--video_tactile` costs beside the render launch it follows; writes profiles/tactile_panel_640x360.json.

    python tools/tactile_panel_bench.py [--out profiles/tactile_panel_640x360.json] [--no-trace]

Frame 640x360, the default panel (render.TactilePanel()), the student -Play- env with its registered env count (20), the four rows of
scripts/distill.py (`policy`, `tactile`, `original_tactile`, `processed_tactile`).  Two measurements, each in a fresh child process
with a time limit of its own (this driver never opens the GPU):
  kernels: the kernels' own time for both launches - lt_render_kernel and lt_tactile_panel_kernel - from one
           `rocprofv3 --kernel-trace --stats` run of `--mode trace` (the program after `--`, no counters in the run).
  wall:    the per-step wall time of a `--video` recording window (env.step with the recorder attached: step, render, copy to pinned
           host memory, deflate on the writer thread) with the flag off and on, alternating, median [min, max] of 7 rounds of 100
           steps, each round ending in a device synchronise.
No speed is promised; that recording with the panel changes nothing is tests/test_hip_tactile_panel.py's to show.
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
TASK = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-Play-v1"
W, H = 640, 360
KERNELS = ("lt_render_kernel", "lt_tactile_panel_kernel")


def stats(xs) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def setup(tactile: bool, folder: str):
    """(env, recorder) of a recording whose video spans the whole measurement."""
    import torch

    from locotouch_amd.env import make
    from locotouch_amd.scripts.distill import panel_signals_of
    from locotouch_amd.video import recorder_for

    env = make(TASK, device="cuda:0", seed=1)
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(20):
        env.step((0.3 * torch.randn(env.num_envs, 12, generator=g)).to("cuda:0"))
    args = argparse.Namespace(video=True, video_length=10 ** 9, video_interval=10 ** 9, video_camera="follow", video_resolution=f"{W}x{H}",
                              video_tactile=tactile)
    rec = recorder_for(env, args, folder, tactile_signals=panel_signals_of(env, {}) if tactile else None)
    return env, rec


def trace(launches: int) -> dict:
    """`launches` frames with the panel: under the profiler this is the run whose kernel statistics are read."""
    import torch

    from locotouch_amd import render as R

    tmp = tempfile.mkdtemp(prefix="tactile_panel_trace_")
    env, rec = setup(True, tmp)
    for _ in range(launches):
        rec.render_fn()
    torch.cuda.synchronize()
    size = R.panel_size(R.TactilePanel(), {"policy": env.obs_tactile, **env.tactile_groups()})
    rec.close(wait=False)
    shutil.rmtree(tmp, ignore_errors=True)
    return {"launches": launches, "panel_size": list(size)}


def wall(rounds: int, steps: int, warmup: int) -> dict:
    import torch

    tmp = tempfile.mkdtemp(prefix="tactile_panel_wall_")
    legs = {flag: setup(flag, os.path.join(tmp, str(int(flag)))) for flag in (False, True)}
    act = torch.zeros(legs[False][0].num_envs, 12, device="cuda:0")
    times = {False: [], True: []}
    for r in range(warmup + rounds):
        for flag in (False, True):  # alternating: both legs see the same machine
            env, _ = legs[flag]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                env.step(act)
            torch.cuda.synchronize()
            if r >= warmup:
                times[flag].append((time.perf_counter() - t0) * 1e3 / steps)
    for _, rec in legs.values():
        rec.close(wait=False)
    shutil.rmtree(tmp, ignore_errors=True)
    return {"device": torch.cuda.get_device_name(0), "envs": legs[False][0].num_envs, "steps_per_round": steps,
            "step_ms_video": stats(times[False]), "step_ms_video_tactile": stats(times[True])}


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


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tactile_panel_640x360.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--mode", choices=["trace", "wall"], help="(internal) one measurement in this process; prints a RESULT line")
    args = ap.parse_args()
    if args.mode == "trace":
        print("RESULT " + json.dumps(trace(args.launches)))
        return
    if args.mode == "wall":
        print("RESULT " + json.dumps(wall(args.rounds, args.steps, args.warmup)))
        return
    res = {"task": TASK, "frame": [W, H], "panel": "render.TactilePanel() defaults; rows policy, tactile, original_tactile, processed_tactile"}
    if args.no_trace:
        res["kernels"] = "not measured"
    else:
        tmp = tempfile.mkdtemp(prefix="tactile_panel_prof_")
        run = child("trace", ["--launches", str(args.launches)], 300, profiler_dir=tmp)
        rows = kernel_stats(tmp) if "error" not in run else {}
        shutil.rmtree(tmp, ignore_errors=True)
        res["kernels"] = {**run, **(rows or {"error": run.get("error", "no row of the two kernels in the kernel statistics")}),
                          "source": "rocprofv3 --kernel-trace --stats, one run, no counters"}
        if all(k in rows for k in KERNELS):
            res["kernels"]["panel_over_render"] = rows[KERNELS[1]]["average_us"] / rows[KERNELS[0]]["average_us"]
    res["wall"] = child("wall", ["--rounds", str(args.rounds), "--steps", str(args.steps), "--warmup", str(args.warmup)], 420)
    res["wall_note"] = "per env step of a recording window: step, render (+ panel), copy to pinned host memory; deflate on the writer thread"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
