"""Policy inference step, eager (`act_inference` + `reset(dones)`) vs fused (rl/fused_policy.py), at the teacher's shape; every leg runs
in a fresh child process; a round is a HIP-event time over `--steps` steps after a warm-up, a leg reports the median of its rounds with
[min, max].  `--policy_class` says which policy:

    recurrent    (default) `ActorCriticRecurrent` vs `FusedRecurrentPolicy` -> lt_policy_step: I = 348, H = 256, actor 256-512-256-128-12,
                 LSTM and GRU memories.  Results: profiles/policy_step_<n>.json
    rnn_encoder  `ActorCriticRNNEncoder` vs `FusedEncoderPolicy` -> lt_policy_encoder_step: rows 348 = 270 + 78, GRU / LSTM H = 256 on the
                 tail, encoder 256-128-64 -> 64, actor 334-512-256-128-12.  Results: profiles/policy_encoder_step_<n>.json
    encoder      `ActorCriticEncoder` vs `FusedEncoderPolicy`: the same without a memory (encoder 78-256-128-64 -> 64).  Results:
                 profiles/policy_encoder_step_<n>_plain.json
Every result file carries `measured_on_commit`.

    python tools/policy_step_bench.py [--policy_class recurrent] [--envs 50 4096] [--steps 200] [--rounds 7] [--out profiles]
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
FLAT, TAIL, ENCODER, EMBEDDING = 270, 78, [256, 128, 64], 64
CELLS = {"recurrent": ("lstm", "gru"), "rnn_encoder": ("lstm", "gru"), "encoder": ("none",)}
FILES = {"recurrent": "policy_step_{n}.json", "rnn_encoder": "policy_encoder_step_{n}.json", "encoder": "policy_encoder_step_{n}_plain.json"}


def build(policy_class: str, cell: str, mode: str):
    """(the module, its fused front or None)."""
    import torch

    from locotouch_amd.rl.fused_policy import FusedEncoderPolicy, FusedRecurrentPolicy
    from locotouch_amd.rl.modules import ActorCriticEncoder, ActorCriticRecurrent, ActorCriticRNNEncoder

    torch.manual_seed(0)
    stacks = dict(actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128])
    if policy_class == "recurrent":
        ac = ActorCriticRecurrent(OBS, OBS, ACTIONS, rnn_type=cell, rnn_hidden_size=HIDDEN, **stacks).to("cuda:0").eval()
        return ac, (FusedRecurrentPolicy.for_actor_critic(ac) if mode == "fused" else None)
    enc = dict(actor_flatten_obs_end_idx=FLAT, actor_encoder_obs_start_idx=-TAIL, actor_encoder_hidden_dims=ENCODER,
               actor_encoder_embedding_dim=EMBEDDING, critic_flatten_obs_end_idx=FLAT, critic_encoder_obs_start_idx=-TAIL,
               critic_encoder_hidden_dims=ENCODER, critic_encoder_embedding_dim=EMBEDDING, **stacks)
    if policy_class == "rnn_encoder":
        ac = ActorCriticRNNEncoder(OBS, OBS, ACTIONS, encoder_rnn_type=cell, encoder_rnn_hidden_size=HIDDEN, **enc).to("cuda:0").eval()
    else:
        ac = ActorCriticEncoder(OBS, OBS, ACTIONS, **enc).to("cuda:0").eval()
    return ac, (FusedEncoderPolicy.for_actor_critic(ac, obs_dim=OBS) if mode == "fused" else None)


def leg(policy_class: str, cell: str, mode: str, n: int, steps: int, rounds: int) -> dict:
    import torch

    ac, fused = build(policy_class, cell, mode)
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


def kernel_trace(policy_class: str, cell: str, n: int, steps: int, rounds: int, timeout: int) -> dict:
    """Per-launch time of the fused leg's kernels: one `rocprofv3 --kernel-trace --stats` run of that leg, nothing else traced."""
    import csv
    import glob
    import shutil
    import tempfile

    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="policy_step_trace_")
    try:
        p = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable,
                            os.path.abspath(__file__), "--policy_class", policy_class, "--leg", cell, "fused", "--n", str(n), "--steps", str(steps),
                            "--rounds", str(rounds)], capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            return {"error": f"rocprofv3 exit {p.returncode}: {p.stderr[-500:]}"}
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                for key in ("lt_policy_encoder_kernel", "lt_policy_memory_kernel"):
                    if key in name:
                        out[key] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
        return out or {"error": "no kernel of the step in the trace"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy_class", choices=sorted(CELLS), default="recurrent", help="which policy and front to time (default: recurrent)")
    ap.add_argument("--leg", nargs=2, metavar=("CELL", "MODE"), default=None, help="child mode: one leg (lstm|gru|none, eager|fused) in this process")
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--envs", type=int, nargs="+", default=[50, 4096])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--trace", action="store_true", help="also record the fused leg's per-launch kernel times from a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--commit", default=None, help="what to record as measured_on_commit (default: git rev-parse HEAD of this tree)")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds must be at least 5")
    if args.leg is not None:
        print("RESULT " + json.dumps(leg(args.policy_class, args.leg[0], args.leg[1], args.n, args.steps, args.rounds)), flush=True)
        return
    os.makedirs(args.out, exist_ok=True)
    cells = CELLS[args.policy_class]
    for n in args.envs:
        legs = []
        for cell in cells:
            for mode in ("eager", "fused"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--policy_class", args.policy_class, "--leg", cell, mode, "--n", str(n),
                                    "--steps", str(args.steps), "--rounds", str(args.rounds)], capture_output=True, text=True, timeout=args.timeout)
                lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not lines:  # a failed child ends the whole run: nothing more is started on the device
                    sys.exit(f"leg {cell}/{mode}/{n} failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                legs.append(json.loads(lines[-1][7:]))
                print(legs[-1], flush=True)
        by = {(c["cell"], c["mode"]): c["us_per_step_median"] for c in legs}
        fused_step = "lt_policy_step" if args.policy_class == "recurrent" else "lt_policy_encoder_step"
        rec = {"measured_on_commit": args.commit or commit(), "n": n, "obs_dim": OBS, "hidden": HIDDEN,
               "notes": {"step": "one policy call and one reset(dones) with 2 % of the rows done: the eager leg is act_inference + the module's "
                                 f"reset (a masked multiply per state tensor), the fused leg is {fused_step} with the mask folded in",
                         "us_per_step": "HIP-event time of a round of `steps` steps / steps; median of the rounds with min and max"},
               "legs": legs, "eager_over_fused": {cell: by[cell, "eager"] / by[cell, "fused"] for cell in cells}}
        if args.trace:
            rec["kernel_trace"] = {cell: kernel_trace(args.policy_class, cell, n, args.steps, 5, args.timeout) for cell in cells}
        if args.policy_class != "recurrent":
            rec.update(policy_class=args.policy_class, flat_dim=FLAT, tail_dim=TAIL, encoder=ENCODER + [EMBEDDING], actor=[512, 256, 128, ACTIONS])
        with open(os.path.join(args.out, FILES[args.policy_class].format(n=n)), "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({k: v for k, v in rec.items() if k not in ("legs", "notes")}), flush=True)


if __name__ == "__main__":
    main()
