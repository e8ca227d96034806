#!/usr/bin/env python3
"""Play a trained policy: the reference's `locotouch/scripts/play.py` flow on the MI355X-native env: the loop steps the policy, prints
episode statistics, optionally exports the actor (with its memory, for a recurrent policy) as TorchScript for the robot-side runtime,
with `--fused_policy` serves a recurrent or an encoder policy from its fused HIP inference step (include/lt_policy.h,
include/lt_policy_encoder.h), and with `--video` records env 0 (animated
PNG, locotouch_amd/video.py) into <run>/videos/play (`--video_tactile`: with the env's tactile groups drawn into the frames, on a tactile
task; refused by name for a task without one; `--video_telemetry`: with strip charts of env 0's command, foot forces and reward).
`--telemetry` records chosen scalars of chosen envs behind every step on the device (locotouch_amd/telemetry.py; `--telemetry_envs`,
`--telemetry_channels`) and writes <run>/telemetry/play.npz at exit.  `--episode_stats` keeps statistics over the finished episodes of
all envs on the device (locotouch_amd/episode_stats.py; `--episode_stats_metrics`), prints their table and writes
<run>/episode_stats/play.json at exit.  Where the run directory holds `params/agent.yaml` (scripts/train.py writes it), its
`policy` and `empirical_normalization` entries take the place of the registered agent cfg's, so a recurrent checkpoint loads.

    python -m locotouch_amd.scripts.play --task Isaac-RandCylinderTransportTeacher-LocoTouch-Play-v1 --num_envs 50 --steps 1000 --export
"""
from __future__ import annotations

import argparse
import os

import torch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="Isaac-RandCylinderTransportTeacher-LocoTouch-Play-v1")
    ap.add_argument("--num_envs", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--headless", action="store_true")
    ap.add_argument("--video", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--load_run", default=None)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--steps", type=int, default=None, help="stop after this many env steps (default: run until interrupted)")
    ap.add_argument("--export", action="store_true", help="write <run>/exported/policy.pt (TorchScript: normaliser -> actor)")
    ap.add_argument("--fused_policy", action="store_true",
                    help="ActorCriticRecurrent, ActorCriticEncoder and ActorCriticRNNEncoder policies: step through the fused HIP inference "
                         "step (rl/fused_policy.py) and reset the memory of finished envs")
    from locotouch_amd.episode_stats import add_episode_stats_args, episode_stats_for, refuse_episode_stats_metrics, report_for
    from locotouch_amd.telemetry import add_telemetry_args, save_for, telemetry_for
    from locotouch_amd.video import add_video_args, refuse_video_tactile, refuse_video_telemetry

    add_video_args(ap)
    add_telemetry_args(ap)
    add_episode_stats_args(ap)
    args, _unknown = ap.parse_known_args()
    refuse_episode_stats_metrics(args)  # an unknown metric name: refused by name before anything is built
    refuse_video_tactile(args, args.task)  # --video_tactile: tactile tasks only, refused by name before anything is built
    refuse_video_telemetry(args)  # --video_telemetry without --video

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.compat.runtime import export_policy_as_jit, get_checkpoint_path
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    agent = train_cfg(args.task)
    root = os.path.abspath(os.path.join("logs", "rsl_rl", agent["experiment_name"]))
    print(f"[INFO] Loading experiment from directory: {root}")
    resume = args.checkpoint if (args.checkpoint and os.path.isfile(args.checkpoint)) else get_checkpoint_path(
        root, args.load_run or ".*", args.checkpoint or "model_.*.pt")
    # the run's own record of what was trained (scripts/train.py `dump_params`): a policy class or normaliser switch that differs from
    # the registered agent cfg - a recurrent teacher - is played as it was trained
    params = os.path.join(os.path.dirname(resume), "params", "agent.yaml")
    if os.path.isfile(params):
        import yaml

        with open(params) as f:
            trained = yaml.safe_load(f) or {}
        agent.update({k: trained[k] for k in ("policy", "empirical_normalization") if k in trained})
    torch.cuda.set_device(args.device)
    env = make(args.task, num_envs=args.num_envs, device=args.device, seed=args.seed if args.seed is not None else agent["seed"])
    runner = OnPolicyRunner(env, agent, log_dir=None, device=args.device)
    print(f"[INFO]: Loading model checkpoint from: {resume}")
    runner.load(resume)
    policy = runner.get_inference_policy(device=args.device, fused=True) if args.fused_policy else runner.get_inference_policy(device=args.device)
    reset_memory = args.fused_policy and hasattr(policy, "reset")
    if args.export:
        out = export_policy_as_jit(runner.alg.actor_critic, runner.obs_normalizer if runner.empirical_normalization else None,
                                   path=os.path.join(os.path.dirname(resume), "exported"), filename="policy.pt")
        print(f"[INFO]: Exported policy to: {out}")
    telemetry = telemetry_for(env, args)  # None without --telemetry / --video_telemetry: nothing is launched then
    stats = episode_stats_for(env, args, skip_running=False)  # (the env was reset just now: no episode is running); None without the flag
    recorder = None
    if args.video:
        from locotouch_amd.video import recorder_for

        recorder = recorder_for(env, args, os.path.join(os.path.dirname(resume), "videos", "play"), telemetry=telemetry)
    obs, _ = env.get_observations()
    t, finished, ret_sum = 0, 0, torch.zeros(env.num_envs, device=env.device)
    try:
        with torch.inference_mode():
            while args.steps is None or t < args.steps:
                obs, rew, dones, _ = env.step(policy(obs))
                if reset_memory:
                    policy.reset(dones)
                ret_sum += rew
                t += 1
                if t % 200 == 0 or t == args.steps:  # (a run of --steps ends on a statistics line)
                    log = env.episode_log()
                    print(f"[play] step {t}: " + ", ".join(f"{k}={v:.3f}" for k, v in sorted(log.items()) if k.startswith(("Episode/", "Metrics/"))))
    finally:
        if recorder is not None:
            recorder.close()
        save_for(telemetry, args, os.path.dirname(resume), "play")
        report_for(stats, os.path.dirname(resume), "play")


if __name__ == "__main__":
    main()
