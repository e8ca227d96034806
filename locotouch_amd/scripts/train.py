#!/usr/bin/env python3
"""Train a teacher policy: the reference's `locotouch/scripts/train.py` flow on the MI355X-native env.

    python -m locotouch_amd.scripts.train --task Isaac-RandCylinderTransportTeacher-LocoTouch-v1 --num_envs 4096 --headless
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m locotouch_amd.scripts.train --task ... (one rank per GPU)

Flags follow the reference CLI (locotouch/scripts/cli_args.py:11-33, train.py:17-29); `--headless` is accepted and ignored.  `--video`
records env 0 every --video_interval env steps for --video_length steps (animated PNG, locotouch_amd/video.py) into <log_dir>/videos/train;
on a tactile task `--video_tactile` draws the env's tactile groups into the frames (refused by name for a task without one), and
`--video_telemetry` strip charts of env 0's command, foot forces and reward.  `--telemetry` records chosen scalars of chosen envs
behind every env step on the device (locotouch_amd/telemetry.py) and writes <log_dir>/telemetry/train.npz at the end (the newest
--telemetry_capacity steps).  `--episode_stats` keeps statistics over the finished episodes of all envs on the device
(locotouch_amd/episode_stats.py) and adds `Eval/<metric>/mean` and `Eval/termination/<name>` to every iteration's record.
Logs: logs/rsl_rl/<experiment>/<timestamp>/{progress.jsonl, model_<it>.pt, params/{env,agent}.{yaml,pkl}, videos/train/*.apng}.
"""
from __future__ import annotations

import argparse
import datetime
import os

import torch


def dump_params(log_dir: str, env_cfg: dict, agent_cfg: dict) -> None:
    """params/env.yaml, agent.yaml, env.pkl, agent.pkl (reference locotouch/scripts/train.py:150-153, isaaclab.utils.io.dump_yaml /
    dump_pickle [DEP]).  The env config is the resolved lt_cfg the kernels run on, as a plain dict (the reference pickles its
    cfg object; a dict loads without this package)."""
    import pickle

    import yaml

    d = os.path.join(log_dir, "params")
    os.makedirs(d, exist_ok=True)
    for name, obj in (("env", env_cfg), ("agent", agent_cfg)):
        with open(os.path.join(d, name + ".yaml"), "w") as f:
            yaml.safe_dump(obj, f)
        with open(os.path.join(d, name + ".pkl"), "wb") as f:
            pickle.dump(obj, f)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="Isaac-RandCylinderTransportTeacher-LocoTouch-v1")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--max_iterations", type=int, default=None)
    ap.add_argument("--headless", action="store_true")
    ap.add_argument("--video", action="store_true")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--load_run", default=None)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--logger", default="tensorboard")
    ap.add_argument("--log_root", default="logs/rsl_rl")
    ap.add_argument("--fused_recurrent_rollout", action="store_true",
                    help="recurrent (LSTM) policies: collect on the fused rollout path (rl/fused.py); exploration noise then comes from "
                         "the kernels' Philox stream instead of torch's generator")
    ap.add_argument("--fused_recurrent_update", action="store_true",
                    help="recurrent (LSTM) policies: update on whole rollouts of env blocks, without padding (rl/ppo.py `_recurrent_update`)")
    ap.add_argument("--fused_gru_memories", action="store_true",
                    help="the two switches above also serve GRU memories (csrc/lt_memory_gru.hip); on its own it does nothing")
    ap.add_argument("--direct_recurrent_update", action="store_true",
                    help="with --fused_recurrent_update: that update without an autograd graph or a host read between its steps "
                         "(rl/ppo.py `_direct_recurrent_update`)")
    ap.add_argument("--fused_encoder_policy", action="store_true",
                    help="encoder policies (ActorCriticEncoder): collect on the fused rollout path and update without an autograd graph or a "
                         "host read between minibatch steps (csrc/lt_encoder.hip, rl/ppo.py `_direct_encoder_update`); exploration noise "
                         "then comes from the kernels' Philox stream instead of torch's generator")
    ap.add_argument("--fused_rnn_encoder_policy", action="store_true",
                    help="RNN-encoder policies (ActorCriticRNNEncoder, LSTM or GRU memories): collect on the fused rollout path "
                         "(include/lt_rnn_encoder.h, rl/fused.py); the update stays the eager one; exploration noise then comes from the "
                         "kernels' Philox stream instead of torch's generator")
    ap.add_argument("--direct_rnn_encoder_update", action="store_true",
                    help="RNN-encoder policies (ActorCriticRNNEncoder): update on whole rollouts of env blocks without padding, an autograd "
                         "graph or a host read between the steps (include/lt_rnn_encoder_train.h, rl/ppo.py `_direct_rnn_encoder_update`); "
                         "independent of --fused_rnn_encoder_policy")
    ap.add_argument("--symmetry_augmentation", action="store_true",
                    help="PPO's mirrored data augmentation (rl/symmetry.py `mirror_go1`): every minibatch with its left-right mirror image; "
                         "on the GPU inside the fused update (include/lt_ppo_sym.h)")
    ap.add_argument("--mirror_loss_coeff", type=float, default=None, metavar="FLOAT",
                    help="PPO's mirror loss with this coefficient (the symmetry loss is logged as Loss/symmetry either way)")
    from locotouch_amd.episode_stats import add_episode_stats_args, episode_stats_for, refuse_episode_stats_metrics
    from locotouch_amd.telemetry import add_telemetry_args, save_for, telemetry_for
    from locotouch_amd.video import add_video_args, refuse_video_tactile, refuse_video_telemetry

    add_video_args(ap)
    add_episode_stats_args(ap)
    add_telemetry_args(ap)
    args, _unknown = ap.parse_known_args()  # hydra-style overrides of the reference CLI are tolerated and ignored
    refuse_video_tactile(args, args.task)  # --video_tactile: tactile tasks only, refused by name before anything is built
    refuse_video_telemetry(args)  # --video_telemetry without --video
    refuse_episode_stats_metrics(args)  # an unknown metric name: refused by name before anything is built

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.rl import Dist, OnPolicyRunner

    dist = Dist.from_env()
    cfg = train_cfg(args.task)
    cfg["logger"] = args.logger
    if args.seed is not None:
        cfg["seed"] = args.seed
    if args.max_iterations is not None:
        cfg["max_iterations"] = args.max_iterations
    if args.fused_recurrent_rollout:
        cfg["fused_recurrent_rollout"] = True
    if args.fused_recurrent_update:
        cfg["fused_recurrent_update"] = True
    if args.fused_gru_memories:
        cfg["fused_gru_memories"] = True
    if args.direct_recurrent_update:
        cfg["direct_recurrent_update"] = True
    if args.fused_encoder_policy:
        cfg["fused_encoder_policy"] = True
    if args.fused_rnn_encoder_policy:
        cfg["fused_rnn_encoder_policy"] = True
    if args.direct_rnn_encoder_update:
        cfg["direct_rnn_encoder_update"] = True
    if args.symmetry_augmentation or args.mirror_loss_coeff is not None:
        from locotouch_amd.rl.symmetry import MIRROR_GO1

        cfg["algorithm"] = dict(cfg["algorithm"], symmetry_cfg=dict(
            use_data_augmentation=bool(args.symmetry_augmentation), use_mirror_loss=args.mirror_loss_coeff is not None,
            mirror_loss_coeff=float(args.mirror_loss_coeff or 0.0), data_augmentation_func=MIRROR_GO1))
    device = f"cuda:{dist.local_rank}"
    torch.cuda.set_device(device)
    torch.manual_seed(cfg["seed"])
    # one population over all ranks: same seed, RNG streams keyed by the GLOBAL env index (rank r owns envs [r*N, (r+1)*N)),
    # and - with more than one rank - the curriculum gate decided on cross-rank sums
    env = make(args.task, num_envs=args.num_envs, device=device, seed=cfg["seed"], env_index_offset=dist.rank * args.num_envs,
               cur_gate_external=1 if dist.world_size > 1 else 0)
    log_dir = os.path.join(args.log_root, cfg["experiment_name"], datetime.datetime.now().strftime("%Y-%m-%d_%H-%M-%S"))
    runner = OnPolicyRunner(env, cfg, log_dir=log_dir, device=device, dist=dist)
    recorder = None
    telemetry = telemetry_for(env, args) if dist.is_main else None  # only the main rank records; None without the flags
    episode_stats_for(env, args)  # every rank keeps its own envs' statistics (the runner logs them); nothing without --episode_stats
    if args.video and dist.is_main:
        from locotouch_amd.video import recorder_for

        recorder = recorder_for(env, args, os.path.join(log_dir, "videos", "train"), telemetry=telemetry)
    if args.resume:  # train.py:131-137 of the reference: newest matching run / checkpoint under the experiment's log root
        from locotouch_amd.compat.runtime import get_checkpoint_path

        ckpt = args.checkpoint if (args.checkpoint and os.path.isfile(args.checkpoint)) else get_checkpoint_path(
            os.path.join(args.log_root, cfg["experiment_name"]), args.load_run or ".*", args.checkpoint or "model_.*.pt")
        print(f"[INFO]: Loading model checkpoint from: {ckpt}")
        runner.load(ckpt)
    if dist.is_main:  # train.py:150-153 of the reference: params/{env,agent}.{yaml,pkl}
        dump_params(log_dir, dict(env.cfg.to_dict(), gym_id=args.task), cfg)
    runner.learn(cfg["max_iterations"], init_at_random_ep_len=True)
    if dist.is_main and runner.history:
        last = runner.history[-1]
        print({k: last[k] for k in ("iter", "Perf/total_fps", "Loss/value_function", "Loss/surrogate", "Loss/learning_rate")})
    if recorder is not None:
        recorder.close()
    save_for(telemetry, args, log_dir, "train")
    dist.shutdown()


if __name__ == "__main__":
    main()
