"""The student's behaviour-cloning step with `fused_bc_step` off (batch assembly, loss and AdamW as torch ops: the default path) against on
(include/lt_bc.h: `lt_bc_gather`, `lt_bc_loss_forward` / `_backward`, `lt_adamw_step`): one `Student.training_step` on a ready batch, and
one epoch of the `train_on_data` loop (assembly + step for every batch of a synthetic buffer of 4 B trajectories of up to L steps).
Every leg runs in a FRESH process (`--child`), the two legs of a shape one after the other.  Events on the stream around `iters`
back-to-back repeats after a warm-up, 5 rounds (median / min / max); peak memory by `torch.cuda.max_memory_allocated` above the resident
set around one call.  Results: profiles/bc_step_<L * B>.json with `measured_on_commit`."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STUDENT = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"


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
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    t = sorted(times)
    return {"ms_median": t[len(t) // 2], "ms_min": t[0], "ms_max": t[-1], "peak_mb_above_resident": (torch.cuda.max_memory_allocated() - base) / 2**20}


def child(L: int, B: int, fused: bool, warm: int, iters: int) -> None:
    import numpy as np
    import torch

    from locotouch_amd.distill import ReplayBuffer, Student, distillation_cfg

    dev = torch.device("cuda:0")
    W = torch.randn(348, 12, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 0.05
    with tempfile.TemporaryDirectory() as tmp:
        cfg = distillation_cfg(STUDENT)
        cfg.device, cfg.log_dir = "cuda:0", tmp
        torch.manual_seed(0)
        st = Student(cfg, 270, 442, 12, teacher_policy_inference=lambda obs: obs @ W, verbose=False)
    if fused:
        st.enable_fused_bc_step()
    st.train()
    # a synthetic buffer: one kept block of L steps of n = 4 B envs; env e holds one trajectory that begins at step 0
    n = 4 * B
    g = torch.Generator(device=dev).manual_seed(1)
    rb = ReplayBuffer(types.SimpleNamespace(num_envs=n, device=dev), None, 270, fused_batches=fused)
    rb._policy_blocks = [torch.randn(L * n, 348, device=dev, generator=g)]
    rb._tactile_blocks = [(torch.rand(L * n, 442, device=dev, generator=g) < 0.1).float()]
    rb._block_base, rb._rows_total = [0], L * n
    lens = np.random.default_rng(1).integers(L // 2, L + 1, n)
    lens[0] = L
    rb._traj_first, rb._traj_len = list(range(n)), [int(x) for x in lens]
    rb._steps_count = int(lens.sum())
    np.random.seed(0)
    batch = next(iter(rb.to_recurrent_generator(batch_size=B)))

    def epoch():
        for b in rb.to_recurrent_generator(batch_size=B):
            st.training_step(b)

    out = {"fused": fused, "L": L, "B": B, "n": L * B, "batches_per_epoch": -(-n // B),
           "training_step": timed(lambda: st.training_step(batch), warm, iters),
           "assembly": timed(lambda: rb._prepare_padded_sequence(np.arange(B), pad_to=(L, B)), warm, iters),
           "epoch": timed(epoch, 1, 1, rounds=3)}
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
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--commit", default=None, help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--dirty", action="store_true", help="with --commit: the measured tree differs from that commit (recorded as tree_differs_from_commit)")
    ap.add_argument("--child", type=int, default=None, help="internal: run one leg (0: switch off, 1: on) for the first --B and print its result")
    args = ap.parse_args()
    if args.child is not None:
        return child(args.L, args.B[0], bool(args.child), args.warmup, args.iters)
    os.makedirs(args.out, exist_ok=True)
    for B in args.B:
        legs = {}
        for fused in (0, 1):  # a fresh process per leg
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(fused), "--L", str(args.L), "--B", str(B), "--warmup", str(args.warmup),
                   "--iters", str(args.iters)]
            run = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
            lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                raise RuntimeError(f"leg fused={fused} B={B} failed ({run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
            legs[fused] = json.loads(lines[0][len("RESULT "):])
            print(legs[fused], flush=True)
        head, dirty = (args.commit, args.dirty) if args.commit else commit()
        rec = {"measured_on_commit": head, "tree_differs_from_commit": dirty, "n": args.L * B, "L": args.L, "B": B, "legs": [legs[0], legs[1]]}
        for k in ("training_step", "assembly", "epoch"):
            rec[f"{k}_speedup"] = legs[0][k]["ms_median"] / legs[1][k]["ms_median"]
        with open(os.path.join(args.out, f"bc_step_{args.L * B}.json"), "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({k: v for k, v in rec.items() if k != "legs"}), flush=True)


if __name__ == "__main__":
    main()
