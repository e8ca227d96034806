"""Recurrent policy inference step, eager (`ActorCriticRecurrent.act_inference` + `reset(dones)`) vs fused (`FusedRecurrentPolicy` ->
lt_policy_step), at the teacher's shape: I = 348, H = 256, actor 256-512-256-128-12, LSTM and GRU memories.  Every leg runs in a fresh
child process; a round is a HIP-event time over `--steps` steps after a warm-up, a leg reports the median of its rounds with [min, max].
Results: profiles/policy_step_<n>.json with `measured_on_commit`.

    python tools/policy_step_bench.py [--envs 50 4096] [--steps 200] [--rounds 7] [--out profiles]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OBS, HIDDEN, ACTIONS = 348, 256, 12


def leg(cell: str, mode: str, n: int, steps: int, rounds: int) -> dict:
    import torch

    from locotouch_amd.rl.fused_policy import FusedRecurrentPolicy
    from locotouch_amd.rl.modules import ActorCriticRecurrent

    torch.manual_seed(0)
    ac = ActorCriticRecurrent(OBS, OBS, ACTIONS, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], rnn_type=cell,
                              rnn_hidden_size=HIDDEN).to("cuda:0").eval()
    fused = FusedRecurrentPolicy.for_actor_critic(ac) if mode == "fused" else None
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.randn(n, OBS, device="cuda", generator=g)
    done = torch.rand(n, device="cuda", generator=g) < 0.02

    def one():
        if fused is not None:
            fused(obs)
            fused.reset(done)
        else:
            ac.act_inference(obs)
            ac.reset(done)

    with torch.inference_mode():
        for _ in range(50):
            one()
        torch.cuda.synchronize()
        times = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                one()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / steps)
    times.sort()
    return {"cell": cell, "mode": mode, "n": n, "steps": steps, "rounds": rounds, "us_per_step_median": times[len(times) // 2],
            "us_per_step_min": times[0], "us_per_step_max": times[-1], "launches_per_step": fused.launches if fused is not None else None}


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs=2, metavar=("CELL", "MODE"), default=None, help="child mode: one leg (lstm|gru, eager|fused) in this process")
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--envs", type=int, nargs="+", default=[50, 4096])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--commit", default=None, help="what to record as measured_on_commit (default: git rev-parse HEAD of this tree)")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds must be at least 5")
    if args.leg is not None:
        print("RESULT " + json.dumps(leg(args.leg[0], args.leg[1], args.n, args.steps, args.rounds)), flush=True)
        return
    os.makedirs(args.out, exist_ok=True)
    for n in args.envs:
        legs = []
        for cell in ("lstm", "gru"):
            for mode in ("eager", "fused"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", cell, mode, "--n", str(n), "--steps", str(args.steps),
                                    "--rounds", str(args.rounds)], capture_output=True, text=True, timeout=args.timeout)
                lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not lines:  # a failed child ends the whole run: nothing more is started on the device
                    sys.exit(f"leg {cell}/{mode}/{n} failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                legs.append(json.loads(lines[-1][7:]))
                print(legs[-1], flush=True)
        by = {(c["cell"], c["mode"]): c["us_per_step_median"] for c in legs}
        rec = {"measured_on_commit": args.commit or commit(), "n": n, "obs_dim": OBS, "hidden": HIDDEN,
               "notes": {"step": "one policy call and one reset(dones) with 2 % of the rows done: the eager leg is act_inference + the module's "
                                 "reset (a masked multiply per state tensor), the fused leg is lt_policy_step with the mask folded in",
                         "us_per_step": "HIP-event time of a round of `steps` steps / steps; median of the rounds with min and max"},
               "legs": legs, "eager_over_fused": {cell: by[cell, "eager"] / by[cell, "fused"] for cell in ("lstm", "gru")}}
        with open(os.path.join(args.out, f"policy_step_{n}.json"), "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({k: v for k, v in rec.items() if k not in ("legs", "notes")}), flush=True)


if __name__ == "__main__":
    main()
