"""Student-driven collection through `ReplayBuffer.collect_data` with the collection switch off (`TactileRecorder`: the loop as it
was) against on (`DeviceTactileRecorder` -> lt_delay_push + lt_collect_after_step); the student acts through `FusedStudent` on both
sides.  A third leg, `ledger`, is `on` plus the device episode ledger (`ReplayBuffer(..., device_ledger=True)` -> lt_ledger_step behind
each env step, a non-blocking poll instead of the blocking read every 16 steps): all three switches against the first two.
Every case runs in a fresh child process; times are HIP events over >= 200 env steps after a warm-up collection.
Results: profiles/collect_step_<n>.json with `measured_on_commit`; with `--trace` the ledger leg runs once more under
`rocprofv3 --kernel-trace --stats` (a run of its own) and the file records the ledger launch's own time from its kernel statistics.

    python tools/collect_step_bench.py [--envs 405 4096] [--steps 200] [--out profiles] [--trace]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/collect_step_bench.py --case on --n 405   (a run of its own)
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STUDENT = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"


def case(switch: str, n: int, steps: int) -> dict:
    import torch

    from locotouch_amd.distill import DeviceTactileRecorder, ReplayBuffer, Student, TactileRecorder, distillation_cfg
    from locotouch_amd.distill.fused_student import FusedStudent
    from locotouch_amd.env import make

    with tempfile.TemporaryDirectory() as tmp:
        cfg = distillation_cfg(STUDENT)
        cfg.device, cfg.log_dir = "cuda:0", tmp
        torch.manual_seed(0)
        st = Student(cfg, 270, 442, 12, verbose=False).eval()
    pol = FusedStudent.for_student(st)
    env = make(STUDENT, num_envs=n, device="cuda:0", seed=3)
    rec = (TactileRecorder if switch == "off" else DeviceTactileRecorder)(env.device, n, 442, cfg.min_delay, cfg.max_delay)
    rb = ReplayBuffer(env, rec, 270, device_ledger=switch == "ledger")
    stepped = [0]
    real_step = env.step

    def counting_step(a):
        stepped[0] += 1
        return real_step(a)

    env.step = counting_step
    torch.manual_seed(1)
    rb.collect_data(None, pol, num_steps=20 * n)  # warm-up
    rb.clear_buffer()
    # an untrained student's episodes are short: collect until at least `steps` env steps have been timed
    stepped[0], ms = 0, 0.0
    while stepped[0] < steps:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        rb.collect_data(None, pol, num_steps=steps * n)
        b.record()
        torch.cuda.synchronize()
        ms += a.elapsed_time(b)
        rb.clear_buffer()
    return {"switch": switch, "n": n, "env_steps": stepped[0], "seconds": ms * 1e-3, "us_per_env_step": ms * 1e3 / stepped[0],
            "env_steps_per_s": stepped[0] * n / (ms * 1e-3)}


def ledger_kernel_stats(n: int, steps: int, timeout: int) -> dict:
    """The ledger leg once more under `rocprofv3 --kernel-trace --stats`: the lt_ledger_step_kernel row of its kernel statistics."""
    import csv
    import glob

    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--case", "ledger",
                            "--n", str(n), "--steps", str(steps)], capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:  # a failed child ends the whole run: nothing more is started on the device
            sys.exit(f"rocprofv3 run of ledger/{n} failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "lt_ledger_step_kernel" in row.get("Name", ""):
                    return {"kernel": "lt_ledger_step_kernel", "calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) * 1e-3,
                            "min_us": float(row["MinNs"]) * 1e-3, "max_us": float(row["MaxNs"]) * 1e-3}
    sys.exit("no lt_ledger_step_kernel row in the rocprofv3 kernel statistics")


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["off", "on", "ledger"], default=None, help="child mode: one case in this process")
    ap.add_argument("--n", type=int, default=405)
    ap.add_argument("--envs", type=int, nargs="+", default=[405, 4096])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--trace", action="store_true", help="also run the ledger leg under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--commit", default=None, help="what to record as measured_on_commit (default: git rev-parse HEAD of this tree)")
    args = ap.parse_args()
    if args.case is not None:
        print("RESULT " + json.dumps(case(args.case, args.n, max(200, args.steps))), flush=True)
        return
    os.makedirs(args.out, exist_ok=True)
    for n in args.envs:
        cases = []
        for switch in ("off", "on", "ledger"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", switch, "--n", str(n), "--steps", str(args.steps)],
                               capture_output=True, text=True, timeout=args.timeout)
            lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not lines:  # a failed child ends the whole run: nothing more is started on the device
                sys.exit(f"case {switch}/{n} failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            cases.append(json.loads(lines[-1][7:]))
            print(cases[-1], flush=True)
        by = {c["switch"]: c for c in cases}
        rec = {"measured_on_commit": args.commit or commit(), "n": n, "baseline": "switch off: the parent commit's loop", "cases": cases,
               "speedup": by["off"]["us_per_env_step"] / by["on"]["us_per_env_step"],
               "ledger_speedup_over_on": by["on"]["us_per_env_step"] / by["ledger"]["us_per_env_step"]}
        if args.trace:
            rec["ledger_kernel"] = ledger_kernel_stats(n, args.steps, args.timeout)
        with open(os.path.join(args.out, f"collect_step_{n}.json"), "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({k: v for k, v in rec.items() if k != "cases"}), flush=True)


if __name__ == "__main__":
    main()
