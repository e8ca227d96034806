#!/usr/bin/env python3
"""Distil a trained teacher into the tactile student: the reference's `locotouch/scripts/distill.py` flow on the MI355X-native env.

    python -m locotouch_amd.scripts.distill --task Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1 --training --headless
    python -m locotouch_amd.scripts.distill --task Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-Play-v1 \\
        --log_dir_distill 2025-... --checkpoint_distill model_7.pt

Flags follow the reference CLI (locotouch/scripts/cli_args.py:11-33,92-124, distill.py:8-20).  The teacher checkpoint is looked
up as the reference does: logs/rsl_rl/<teacher experiment>/<--load_run>/<--checkpoint> (latest matching).  `--video` records env 0
(animated PNG, locotouch_amd/video.py) into <distill log root>/videos/{train,play}; `--video --video_tactile` draws the tactile signals
into the frames' top-right corner, top to bottom: `policy` (the delayed rows the student reads), `tactile`, and on the -Play- env
`original_tactile` and `processed_tactile` (include/lt_tactile_panel.h) - the reference play loop's three ROS topics plus the undelayed signal.
`--telemetry` (both modes) records chosen scalars of chosen envs behind every env step on the device (locotouch_amd/telemetry.py) and
writes <distill log root>/telemetry/{train,play}.npz at exit; `--video --video_telemetry` charts env 0's command, foot forces and reward
in the frames' bottom-left corner.  `--episode_stats` (both modes) keeps statistics over the finished episodes of all envs on the device
(locotouch_amd/episode_stats.py), prints their table and writes <distill log root>/episode_stats/{train,play}.json at exit.
"""
from __future__ import annotations

import argparse
import os

import torch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1")
    ap.add_argument("--num_envs", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--headless", action="store_true")
    ap.add_argument("--video", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--training", action="store_true", default=False)
    ap.add_argument("--load_run", default=None)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--log_dir_distill", default=None)
    ap.add_argument("--checkpoint_distill", default=None)
    ap.add_argument("--distill_lr", type=float, default=None)
    ap.add_argument("--logger", default=None, choices=["wandb", "tensorboard"])
    ap.add_argument("--play_steps", type=int, default=None, help="play mode: stop after this many env steps (default: run until interrupted)")
    ap.add_argument("--fused_student", action="store_true",
                    help="run the student's env steps (DAgger collection, evaluation, play) through the fused HIP step (lt_student_step)")
    ap.add_argument("--fused_collect", action="store_true",
                    help="run the tactile delay line and the per-step recording of collection / play in HIP kernels (lt_delay_push, lt_collect_after_step)")
    ap.add_argument("--device_ledger", action="store_true",
                    help="keep the trajectory bookkeeping of collection / evaluation on the device (lt_ledger_step behind each env step)")
    ap.add_argument("--fused_cnn_train", action="store_true",
                    help="train the student's tactile CNN head through the HIP kernels of lt_cnn_train.h (lt_cnn_forward, lt_cnn_backward)")
    ap.add_argument("--fused_bc_step", action="store_true",
                    help="assemble batches, compute the masked BC loss and step AdamW through the HIP kernels of lt_bc.h (lt_bc_gather, "
                         "lt_bc_loss_forward / _backward, lt_adamw_step)")
    from locotouch_amd.episode_stats import add_episode_stats_args, episode_stats_for, refuse_episode_stats_metrics, report_for
    from locotouch_amd.telemetry import add_telemetry_args, save_for, telemetry_for
    from locotouch_amd.video import add_video_args, refuse_video_tactile, refuse_video_telemetry

    add_video_args(ap)
    add_telemetry_args(ap)
    add_episode_stats_args(ap)
    args, _unknown = ap.parse_known_args()
    refuse_episode_stats_metrics(args)
    refuse_video_tactile(args, args.task)
    refuse_video_telemetry(args)

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.distill import distillation_cfg
    from locotouch_amd.env import make

    cfg = distillation_cfg(args.task)
    cfg.device = args.device
    if args.logger is not None:
        cfg.logger = args.logger
    if args.distill_lr is not None:
        cfg.distill_lr = args.distill_lr
    torch.cuda.set_device(args.device)
    agent = train_cfg(args.task)
    env = make(args.task, num_envs=args.num_envs, device=args.device, seed=args.seed if args.seed is not None else agent["seed"])
    distill_root = os.path.abspath(os.path.join(cfg.log_root_path, cfg.experiment_name))
    mode = "train" if args.training else "play"
    telemetry = telemetry_for(env, args)  # None without --telemetry / --video_telemetry: nothing is launched then
    stats = episode_stats_for(env, args, skip_running=args.training)  # play: the env was reset just now; None without --episode_stats
    recorder = None
    delay_line: dict = {}  # "recorder": the Distillation's tactile recorder, once there is one (_run)
    if args.video:
        from locotouch_amd.video import recorder_for

        recorder = recorder_for(env, args, os.path.join(distill_root, "videos", mode),
                                tactile_signals=panel_signals_of(env, delay_line) if args.video_tactile else None, telemetry=telemetry)
    try:
        _run(args, cfg, agent, env, distill_root, delay_line)
    finally:
        if recorder is not None:
            recorder.close()
        save_for(telemetry, args, distill_root, mode)
        report_for(stats, distill_root, mode)


def panel_signals_of(env, delay_line: dict):
    """The callable `recorder_for(..., tactile_signals=)` asks for the --video_tactile panel's rows, top to bottom: `policy` - the DELAYED
    rows the student reads, as the loops' delay line handed them out last (`last_delayed` of delay_line["recorder"]: the loops' own
    buffer, no copy and no launch; zeros until the first push, as the delay line itself answers then) - and the env's own groups:
    `tactile`, and on the -Play- env `original_tactile` and `processed_tactile`.  These are the reference play loop's three topics
    (distillation.py:132-143, 202-211) plus the undelayed signal."""
    groups = env.tactile_groups()  # ValueError, naming the task, without a tactile group
    zeros = torch.zeros_like(groups["tactile"], memory_format=torch.contiguous_format)

    def signals():
        rec = delay_line.get("recorder")
        delayed = getattr(rec, "last_delayed", None)
        policy = zeros if delayed is None else delayed.reshape(delayed.shape[0], -1)  # (a view: the rows are contiguous inside)
        return {"policy": policy, **groups}

    return signals


def _run(args, cfg, agent, env, distill_root, delay_line: dict | None = None) -> None:
    from locotouch_amd.compat.runtime import get_checkpoint_path
    from locotouch_amd.distill import Distillation
    from locotouch_amd.rl import OnPolicyRunner

    if args.training:
        teacher_root = os.path.abspath(os.path.join("logs", "rsl_rl", agent["experiment_name"]))
        resume = get_checkpoint_path(teacher_root, args.load_run or ".*", args.checkpoint or "model_.*.pt")
        print(f"[INFO] Loading teacher policy checkpoint from: {resume}")
        runner = OnPolicyRunner(env, agent, log_dir=None, device=args.device)
        runner.load(resume)
        mono = cfg.distillation_type == "Monolithic"
        d = Distillation(env, cfg, teacher_policy=runner.get_inference_policy(device=args.device),
                         teacher_encoder=None if mono else runner.get_inference_encoder(device=args.device),
                         teacher_backbone_weights=None if mono else runner.get_backbone_weights(), training=True,
                         fused_student_inference=args.fused_student, fused_collection=args.fused_collect, device_ledger=args.device_ledger,
                         fused_cnn_training=args.fused_cnn_train, fused_bc_step=args.fused_bc_step)
        if delay_line is not None:
            delay_line["recorder"] = d.tactile_recorder
        d.train()
    else:
        # (`--video`, `--telemetry` and `--episode_stats` keep their files in <distill root>/videos, /telemetry and /episode_stats, beside the runs:
        # those folders are no runs)
        ckpt = get_checkpoint_path(distill_root, args.log_dir_distill or r"(?!(videos|telemetry|episode_stats)$).*", args.checkpoint_distill or "model_.*.pt")
        d = Distillation(env, cfg, training=False, checkpoint=ckpt, fused_student_inference=args.fused_student, fused_collection=args.fused_collect,
                         device_ledger=args.device_ledger)
        if delay_line is not None:
            delay_line["recorder"] = d.tactile_recorder
        d.play(num_steps=args.play_steps)


if __name__ == "__main__":
    main()
