"""What PPO's `symmetry_cfg` costs a training iteration: writes profiles/ppo_symmetry_<n>.json.

Teacher task, `--envs` envs (4096) x 24 steps, the registered agent cfg (feed-forward ActorCritic [512, 256, 128], 5 epochs x 4
minibatches, adaptive schedule).  Eight legs, one fresh process each, `--warmup` (3) iterations, then the median of `--rounds` (7) with
[min, max]:
  control          the registered cfg as it is, no symmetry_cfg
  aug              use_data_augmentation with `mirror_go1`: the fused path (rl/ppo.py `_direct_update`, include/lt_ppo_sym.h)
  aug_mirror       ... plus the mirror loss (mirror_loss_coeff 0.5)
  aug_ops          `aug` through the torch op chain (`direct_update=False, fused_loss=False`: `_symmetry_update`)
  aug_mirror_ops   `aug_mirror` through the op chain
  mirror           the mirror loss alone, no augmentation: the fused path with the actor on 2 m rows and the critic on m
                   (include/lt_ppo_mirror.h, include/lt_mlp_rows.h)
  mirror_ops       `mirror` through the op chain
  log_only         both switches off, the symmetry loss formed for the log alone: the fused path, backward on m rows
and per leg
  rollout_ms    `Perf/collection time` of `runner.learn` (host wall clock of the rollout and compute_returns)
  update_ms     `Perf/learning_time` (host wall clock of `alg.update()`, which ends in a host read)
  iteration_ms  their sum
  which         the update each iteration ran: "direct" or "ops" (taken from the PPO object, not assumed)
Every leg uses the public runner interface alone, so the same file measures the parent commit: run `--leg control --label parent` (and
any other leg) in a checkout of the parent and hand the RESULT lines to `--parent-result`; without it the file says "not measured"
there.  Per leg measured on both trees one statement is drawn, and not against a threshold set in advance: whether the [min, max] on
this tree overlaps the parent's (for the control, the no-regression condition), and whether it lies wholly below it.  The symmetric
legs are recorded as measured.  `--legs` names the legs to run (default: all of them); `--this-results FILE` hands over legs of this
tree that were already measured (`--leg X --label this`, alternating with the parent's in one session).

Two processes a minute apart can differ by a few percent in clocks alone; `--control-runs FILE` takes RESULT lines of the control leg
run ALTERNATELY on the two trees (`--label this`, `--label parent`, ...) and records them with the overlap of every neighbouring pair.

    python tools/ppo_symmetry_bench.py [--envs 4096] [--rounds 7] [--legs control,aug,mirror] [--parent-result FILE] [--control-runs FILE] [--out profiles/ppo_symmetry_4096.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TASK = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
MIRROR_LOSS_COEFF = 0.5
# leg -> (symmetry_cfg given, data augmentation, mirror loss, through the op chain)
LEGS = {"control": (False, False, False, False), "aug": (True, True, False, False), "aug_mirror": (True, True, True, False),
        "aug_ops": (True, True, False, True), "aug_mirror_ops": (True, True, True, True), "mirror": (True, False, True, False),
        "mirror_ops": (True, False, True, True), "log_only": (True, False, False, False)}
KEYS = ("rollout_ms", "update_ms", "iteration_ms")


def stats(xs: list[float]) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def tree() -> str | None:
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def measure(leg: str, envs: int, rounds: int, warmup: int, label: str | None = None) -> dict:
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import PPO, OnPolicyRunner

    sym, aug, mirror, ops = LEGS[leg]
    cfg = train_cfg(TASK)
    alg_cfg = dict(cfg["algorithm"])
    if sym:
        alg_cfg["symmetry_cfg"] = dict(use_data_augmentation=aug, use_mirror_loss=mirror, mirror_loss_coeff=MIRROR_LOSS_COEFF if mirror else 0.0,
                                       data_augmentation_func="locotouch_amd.rl.symmetry:mirror_go1")
    if ops:
        alg_cfg.update(direct_update=False, fused_loss=False)
    cfg["algorithm"] = alg_cfg
    runner = OnPolicyRunner(make(TASK, num_envs=envs, device="cuda:0", seed=1), cfg, log_dir=None, device="cuda:0")
    alg = runner.alg
    which = []
    for name, tag in (("_direct_update", "direct"), ("_symmetry_update", "ops")):
        real = getattr(PPO, name, None)
        if real is not None:
            setattr(PPO, name, (lambda real, tag: lambda self, *a, **k: (which.append(tag), real(self, *a, **k))[1])(real, tag))
    out = {"leg": leg, "tree": label or tree(), "fused_rollout": runner._make_fused() is not None, "steps": runner.num_steps_per_env,
           "num_mini_batches": alg.num_mini_batches, "num_learning_epochs": alg.num_learning_epochs}
    runner.learn(warmup + rounds)
    recs = runner.history[warmup:]
    out["which"] = sorted(set(which))
    out["rollout_ms"] = stats([1e3 * r["Perf/collection time"] for r in recs])
    out["update_ms"] = stats([1e3 * r["Perf/learning_time"] for r in recs])
    out["iteration_ms"] = stats([1e3 * (r["Perf/collection time"] + r["Perf/learning_time"]) for r in recs])
    if sym:
        out["loss_symmetry_last"] = recs[-1].get("Loss/symmetry")
    return out


def overlap(a: dict, b: dict) -> bool:
    return a["min"] <= b["max"] and b["min"] <= a["max"]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--parent-result", help="file holding the RESULT lines of `--leg control --label parent` (and of other legs) run in a checkout of the parent commit")
    ap.add_argument("--this-results", help="file holding RESULT lines of `--leg X --label this` of this tree (run alternately with the parent's): those legs are taken from it, not run again")
    ap.add_argument("--legs", help="comma-separated legs to run (default: all); update_over_control needs the control among them")
    ap.add_argument("--control-runs", help="file holding RESULT lines of `--leg control --label this|parent`, run alternately")
    ap.add_argument("--leg", choices=list(LEGS), help="measure one leg in this process and print its RESULT line")
    ap.add_argument("--label", help="with --leg: what to record as the leg's tree (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("--rounds must be at least 5")
    if args.leg:
        print("RESULT " + json.dumps(measure(args.leg, args.envs, args.rounds, args.warmup, args.label)))
        return
    legs, parent, parent_legs = {}, None, {}
    chosen = [l for l in (args.legs.split(",") if args.legs else LEGS) if l]
    if any(l not in LEGS for l in chosen):
        sys.exit(f"--legs: known legs are {list(LEGS)}")
    if args.parent_result:
        recs = [json.loads(l[7:]) for l in open(args.parent_result).read().splitlines() if l.startswith("RESULT ")]
        parent_legs = {r["leg"]: r for r in recs}  # (the last line of a leg counts)
        if "control" not in parent_legs:
            sys.exit(f"{args.parent_result}: no RESULT line of the control leg")
        parent = parent_legs.pop("control")
    if args.this_results:
        legs = {r["leg"]: r for r in (json.loads(l[7:]) for l in open(args.this_results).read().splitlines() if l.startswith("RESULT ")) if r["tree"] == "this"}
    for leg in [l for l in chosen if l not in legs]:  # a fresh process each: no allocator state carried from one to the next
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--envs", str(args.envs), "--rounds", str(args.rounds),
                            "--warmup", str(args.warmup), "--label", "this"], capture_output=True, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{leg}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        legs[leg] = json.loads(line[-1][7:])
    res = {"task": TASK, "envs": args.envs, "measured_on_commit": args.commit or tree(), "mirror_loss_coeff": MIRROR_LOSS_COEFF,
           "notes": {"rollout_ms": "runner wall clock of the rollout and compute_returns", "update_ms": "runner wall clock of alg.update() (it ends in a host read)",
                     "iteration_ms": "their sum", "spread": "min and max over the rounds, beside the median",
                     "parent_control": "the control leg run by the same tool in a checkout of the parent commit (--parent-result)"},
           "legs": legs, "parent_control": parent if parent is not None else "not measured"}
    if parent is not None and "control" in legs:
        res["control_intervals_overlap"] = {k: overlap(legs["control"][k], parent[k]) for k in KEYS}
    if parent_legs:  # the other legs of the parent commit, where the same cfg may take another path (`which` says so)
        res["parent_legs"] = parent_legs
        both = [leg for leg in parent_legs if leg in legs]
        res["leg_intervals_overlap_parent"] = {leg: {k: overlap(legs[leg][k], parent_legs[leg][k]) for k in KEYS} for leg in both}
        res["leg_update_wholly_below_parent"] = {leg: legs[leg]["update_ms"]["max"] < parent_legs[leg]["update_ms"]["min"] for leg in both}
    if "control" in legs:
        res["update_over_control"] = {leg: legs[leg]["update_ms"]["median"] / legs["control"]["update_ms"]["median"] for leg in legs if leg != "control"}
    if args.control_runs:
        runs = [json.loads(l[7:]) for l in open(args.control_runs).read().splitlines() if l.startswith("RESULT ")]
        if len(runs) < 2 or any(r["leg"] != "control" for r in runs) or any(a["tree"] == b["tree"] for a, b in zip(runs, runs[1:])):
            sys.exit(f"{args.control_runs}: needs RESULT lines of the control leg that alternate between two labels")
        res["control_alternating"] = {"runs": [{"tree": r["tree"], **{k: r[k] for k in KEYS}} for r in runs],
                                      "every_neighbouring_pair_overlaps": {k: all(overlap(a[k], b[k]) for a, b in zip(runs, runs[1:])) for k in KEYS}}
    out = args.out or os.path.join(REPO, "profiles", f"ppo_symmetry_{args.envs}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
