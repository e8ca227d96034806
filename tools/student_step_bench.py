"""Student inference step, eager (`Student.forward`) vs fused (`FusedStudent` -> lt_student_step), and student-driven collection
through `ReplayBuffer.collect_data` with either.  Every case runs in a fresh child process; times are HIP events over >= 200 steps
after a warm-up.  Results: profiles/student_step_<n>.json with `measured_on_commit`.

    python tools/student_step_bench.py [--envs 405 4096] [--steps 200] [--out profiles]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/student_step_bench.py --case step --mode fused --n 405   (a run of its own)
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


def _student(tmp):
    import torch

    from locotouch_amd.distill import Student, distillation_cfg

    cfg = distillation_cfg(STUDENT)
    cfg.device, cfg.log_dir = "cuda:0", tmp
    torch.manual_seed(0)
    return Student(cfg, 270, 442, 12, verbose=False).eval()


def case_step(mode: str, n: int, steps: int) -> dict:
    import torch

    from locotouch_amd.distill.fused_student import FusedStudent

    with tempfile.TemporaryDirectory() as tmp:
        st = _student(tmp)
    pol = FusedStudent.for_student(st) if mode == "fused" else st
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.randn(n, 348, device="cuda", generator=g)
    tac = (torch.rand(n, 442, device="cuda", generator=g) < 0.1).float()
    done = torch.rand(n, device="cuda", generator=g) < 0.02
    prop = rows[:, :270]

    def one():
        pol(prop, tac)
        pol.reset(done)

    with torch.no_grad():
        for _ in range(50):
            one()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                one()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / steps)
    times.sort()
    return {"case": "step", "mode": mode, "n": n, "steps": steps, "us_per_step_median": times[2], "us_per_step_min": times[0], "us_per_step_max": times[-1]}


def case_collect(mode: str, n: int, steps: int) -> dict:
    import torch

    from locotouch_amd.distill import ReplayBuffer, TactileRecorder
    from locotouch_amd.distill.fused_student import FusedStudent
    from locotouch_amd.env import make

    with tempfile.TemporaryDirectory() as tmp:
        st = _student(tmp)
    pol = FusedStudent.for_student(st) if mode == "fused" else st
    env = make(STUDENT, num_envs=n, device="cuda:0", seed=3)
    rb = ReplayBuffer(env, TactileRecorder(env.device, n, 442, 1, 2), 270)
    rb.collect_data(None, pol, num_steps=20 * n)  # warm-up
    rb.clear_buffer()
    stepped = [0]
    real_step = env.step

    def counting_step(a):
        stepped[0] += 1
        return real_step(a)

    env.step = counting_step
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    rb.collect_data(None, pol, num_steps=steps * n)
    b.record()
    torch.cuda.synchronize()
    sec = a.elapsed_time(b) * 1e-3
    return {"case": "collect", "mode": mode, "n": n, "env_steps": stepped[0], "seconds": sec, "env_steps_per_s": stepped[0] * n / sec}


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["step", "collect"], default=None, help="child mode: one case in this process")
    ap.add_argument("--mode", choices=["eager", "fused"], default="fused")
    ap.add_argument("--n", type=int, default=405)
    ap.add_argument("--envs", type=int, nargs="+", default=[405, 4096])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--commit", default=None, help="what to record as measured_on_commit (default: git rev-parse HEAD of this tree)")
    args = ap.parse_args()
    if args.case is not None:
        fn = case_step if args.case == "step" else case_collect
        print("RESULT " + json.dumps(fn(args.mode, args.n, args.steps)), flush=True)
        return
    os.makedirs(args.out, exist_ok=True)
    for n in args.envs:
        cases = []
        for case in ("step", "collect"):
            for mode in ("eager", "fused"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--mode", mode, "--n", str(n), "--steps", str(args.steps)],
                                   capture_output=True, text=True, timeout=args.timeout)
                lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not lines:  # a failed child ends the whole run: nothing more is started on the device
                    sys.exit(f"case {case}/{mode}/{n} failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                cases.append(json.loads(lines[-1][7:]))
                print(cases[-1], flush=True)
        by = {(c["case"], c["mode"]): c for c in cases}
        rec = {"measured_on_commit": args.commit or commit(), "n": n, "cases": cases,
               "step_speedup": by["step", "eager"]["us_per_step_median"] / by["step", "fused"]["us_per_step_median"],
               "collect_speedup": by["collect", "fused"]["env_steps_per_s"] / by["collect", "eager"]["env_steps_per_s"]}
        with open(os.path.join(args.out, f"student_step_{n}.json"), "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({k: v for k, v in rec.items() if k != "cases"}), flush=True)


if __name__ == "__main__":
    main()
