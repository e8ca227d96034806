#!/usr/bin/env python3
"""Distil a trained teacher into the tactile student: the reference's `locotouch/scripts/distill.py` flow on the MI355X-native env.

    python -m locotouch_amd.scripts.distill --task Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1 --training --headless
    python -m locotouch_amd.scripts.distill --task Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-Play-v1 \\
        --log_dir_distill 2025-... --checkpoint_distill model_7.pt

Flags follow the reference CLI (locotouch/scripts/cli_args.py:11-33,92-124, distill.py:8-20).  The teacher checkpoint is looked
up as the reference does: logs/rsl_rl/<teacher experiment>/<--load_run>/<--checkpoint> (latest matching).  `--video` records env 0
(animated PNG, locotouch_amd/video.py) into <distill log root>/videos/{train,play}.
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
    from locotouch_amd.video import add_video_args

    add_video_args(ap)
    args, _unknown = ap.parse_known_args()

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
    recorder = None
    if args.video:
        from locotouch_amd.video import recorder_for

        recorder = recorder_for(env, args, os.path.join(distill_root, "videos", "train" if args.training else "play"))
    try:
        _run(args, cfg, agent, env, distill_root)
    finally:
        if recorder is not None:
            recorder.close()


def _run(args, cfg, agent, env, distill_root) -> None:
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
        d.train()
    else:
        ckpt = get_checkpoint_path(distill_root, args.log_dir_distill or ".*", args.checkpoint_distill or "model_.*.pt")
        d = Distillation(env, cfg, training=False, checkpoint=ckpt, fused_student_inference=args.fused_student, fused_collection=args.fused_collect,
                         device_ledger=args.device_ledger)
        d.play(num_steps=args.play_steps)


if __name__ == "__main__":
    main()
