#!/usr/bin/env python3
"""LSTM over whole trajectories at the distillation's shapes, forward + backward: `nn.LSTM` (MIOpen's RNN path) against rl/lstm.py's
PyTorch-op time loop and its HIP form (csrc/lt_lstm.hip).  The LSTM counterpart of tools/gru_probe.py.

Every leg runs in a FRESH process (`--child`), the three legs of a shape one after the other.  A leg is `iters` back-to-back repeats of
zero_grad + forward + `out.sum().backward()` between two stream events after a warm-up, 5 rounds: median / min / max (the spread).
Results: profiles/lstm_probe_<L * B>.json with `measured_on_commit`; `hip_beats_miopen_beyond_spread` is true when the HIP form's
slowest round is faster than nn.LSTM's fastest - the rule the default of `rl/lstm.py::use_hip_kernels` follows (on only if true at
every shape)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LEGS = ("miopen", "torch_loop", "hip")


def timed(fn, warm: int, iters: int, rounds: int = 5) -> dict:
    import torch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / iters)
    t = sorted(times)
    return {"ms_median": t[len(t) // 2], "ms_min": t[0], "ms_max": t[-1], "rounds": rounds, "iters": iters}


def child(leg: str, L: int, B: int, I: int, H: int, warm: int, iters: int) -> None:
    import torch
    import torch.nn as nn

    import locotouch_amd.rl.lstm as LS

    if not torch.cuda.is_available():
        raise SystemExit("lstm_probe: no GPU - a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    lstm = nn.LSTM(I, H).cuda()
    x = torch.randn(L, B, I, device="cuda", requires_grad=True)
    LS.use_hip_kernels = leg == "hip"
    fwd = (lambda v: lstm(v)[0]) if leg == "miopen" else (lambda v: LS.lstm_sequence(lstm, v)[0])

    def step():
        lstm.zero_grad()
        x.grad = None
        fwd(x).sum().backward()

    out = {"leg": leg, "L": L, "B": B, "I": I, "H": H, **timed(step, warm, iters)}
    out["ms_per_time_step"] = out["ms_median"] / L
    print("RESULT " + json.dumps(out), flush=True)


def commit():
    """(HEAD, whether the tree differs from it); (None, None) outside a checkout"""
    try:
        run = lambda *a: subprocess.run(["git", "-C", REPO, *a], capture_output=True, text=True, check=True).stdout.strip()  # noqa: E731
        return run("rev-parse", "--short", "HEAD"), bool(run("status", "--porcelain", "--untracked-files=no"))
    except Exception:  # noqa: BLE001
        return None, None


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--B", type=int, nargs="+", default=[48, 100])
    ap.add_argument("--I", type=int, default=64)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--commit", default=None, help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--dirty", action="store_true", help="with --commit: the measured tree differs from that commit (recorded as tree_differs_from_commit)")
    ap.add_argument("--child", choices=LEGS, default=None, help="internal: run one leg for the first --B and print its result")
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.L, args.B[0], args.I, args.H, args.warmup, args.iters)
    os.makedirs(args.out, exist_ok=True)
    for B in args.B:
        legs = {}
        for leg in LEGS:  # a fresh process per leg
            cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--L", str(args.L), "--B", str(B), "--I", str(args.I), "--H", str(args.H),
                   "--warmup", str(args.warmup), "--iters", str(args.iters)]
            run = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
            lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                raise RuntimeError(f"leg {leg} B={B} failed ({run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
            legs[leg] = json.loads(lines[0][len("RESULT "):])
            print(legs[leg], flush=True)
        head, dirty = (args.commit, args.dirty) if args.commit else commit()
        rec = {"measured_on_commit": head, "tree_differs_from_commit": dirty, "n": args.L * B, "L": args.L, "B": B, "I": args.I, "H": args.H,
               "legs": [legs[k] for k in LEGS],
               "hip_speedup_over_miopen": legs["miopen"]["ms_median"] / legs["hip"]["ms_median"],
               "hip_speedup_over_torch_loop": legs["torch_loop"]["ms_median"] / legs["hip"]["ms_median"],
               "hip_beats_miopen_beyond_spread": legs["hip"]["ms_max"] < legs["miopen"]["ms_min"]}
        with open(os.path.join(args.out, f"lstm_probe_{args.L * B}.json"), "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({k: v for k, v in rec.items() if k != "legs"}), flush=True)


if __name__ == "__main__":
    main()
