"""DAgger distillation loop (reference locotouch/distill/distillation.py:20-212) on the MI355X-native student env.

    iteration 0:  collect `bc_data_steps` with the TEACHER acting        -> behaviour cloning
    iteration i:  collect `dagger_data_steps` with the STUDENT acting, teacher actions as labels (the buffer keeps growing)
    last:         evaluate the student on `evaluation_trajs_num` episodes

The env is the student registration (`cfg.tactile_enabled`): observation groups policy (proprioception 270 | object state 78),
tactile (442) and object_state (78).  The teacher is a trained PPO runner of the same task family (its checkpoint loads
with `weights_only=True`).
"""
from __future__ import annotations

import datetime
import os

import numpy as np
import torch

from .config import DistillationCfg
from .replay_buffer import ReplayBuffer
from .student import Student
from .tactile_recorder import TactileRecorder


class Distillation:
    def __init__(self, env, cfg: DistillationCfg, teacher_policy=None, teacher_encoder=None, teacher_backbone_weights=None,
                 training: bool = True, log_dir: str | None = None, checkpoint: str | None = None, verbose: bool = True,
                 fused_student_inference: bool = False, fused_collection: bool = False,
                 device_ledger: bool = False, fused_cnn_training: bool = False, fused_bc_step: bool = False):
        """`fused_student_inference`: the student's env steps (DAgger collection, evaluation, play) run through
        `FusedStudent` - one `lt_student_step` per step instead of `Student.forward`; training is unchanged.
        `fused_collection`: the tactile delay line and the per-step recording of `collect_data` / `play` run through
        `DeviceTactileRecorder` (two HIP launches per step, same bits); needs a CUDA env, composes with the other switch.
        `device_ledger`: the trajectory bookkeeping of `collect_data` / `evaluate` runs in `DeviceEpisodeLedger` (one HIP launch behind
        each env step, a non-blocking poll instead of the blocking copy every `check_every` steps; same bits, the loop may run up to
        `2 * check_every - 1` discarded steps past the stopping step); needs a CUDA env, composes with the other two.
        `fused_cnn_training`: the student's tactile CNN head trains through the HIP kernels of include/lt_cnn_train.h
        (`CNN2dHead.enable_fused_training`: direct convolutions, a backward that recomputes the maps) instead of `Conv2dAsGemm` and
        autograd's saved maps; needs a CUDA env and a served conv stack (ValueError otherwise), composes with the other three.
        `fused_bc_step`: the two ends of the student's training step run through the HIP kernels of include/lt_bc.h - padded batches are
        assembled by one launch (`ReplayBuffer(..., fused_batches=True)`), the masked loss with its statistics takes two launches forward
        and one backward and AdamW one (`Student.enable_fused_bc_step`); needs a CUDA env and `training=True` (ValueError otherwise),
        composes with the other four."""
        self.env, self.cfg, self.training = env, cfg, training
        obs, extras = env.get_observations()
        groups = extras["observations"]
        if "tactile" not in groups or "object_state" not in groups:
            raise ValueError("distillation needs a student task (observation groups `tactile` and `object_state`)")
        self.proprioception_dim = groups["policy"].shape[-1] - groups["object_state"].shape[-1]   # distillation.py:57
        self.tactile_signal_dim = groups["tactile"].shape[-1]
        if verbose:
            print(f"[INFO] Tactile signal dim: {self.tactile_signal_dim}, Proprioception dim: {self.proprioception_dim}")
        if fused_collection:
            from .device_recorder import DeviceTactileRecorder  # ValueError for a non-CUDA env: no fall-back

            self.tactile_recorder = DeviceTactileRecorder(env.device, env.num_envs, self.tactile_signal_dim, cfg.min_delay, cfg.max_delay)
        else:
            self.tactile_recorder = TactileRecorder(env.device, env.num_envs, self.tactile_signal_dim, cfg.min_delay, cfg.max_delay)
        if fused_cnn_training and torch.device(env.device).type != "cuda":
            raise ValueError("Distillation: fused_cnn_training needs a CUDA env")
        if fused_cnn_training and not training:  # (play trains nothing, but the switch never passes quietly)
            raise ValueError("Distillation: fused_cnn_training needs training=True")
        if fused_bc_step and torch.device(env.device).type != "cuda":
            raise ValueError("Distillation: fused_bc_step needs a CUDA env")
        if fused_bc_step and not training:  # (play trains nothing, but the switch never passes quietly)
            raise ValueError("Distillation: fused_bc_step needs training=True")
        cfg.device = str(env.device)
        self.logger = None
        if training:
            if teacher_policy is None:
                raise ValueError("training needs the teacher's inference policy")
            root = os.path.abspath(os.path.join(cfg.log_root_path, cfg.experiment_name))
            cfg.log_dir = log_dir or os.path.join(root, datetime.datetime.now().strftime("%Y-%m-%d_%H-%M-%S"))
            os.makedirs(cfg.log_dir, exist_ok=True)
            if verbose:
                print(f"[INFO] Logging student distillation in: {cfg.log_dir}")
            if cfg.logger == "tensorboard":
                from ..rl.tb_writer import SummaryWriter

                self.logger = SummaryWriter(log_dir=cfg.log_dir)
            elif cfg.logger == "wandb":
                try:
                    import wandb  # noqa: F401
                except ImportError:  # no wandb in this image: keep the run alive, log to TensorBoard event files instead
                    print("[WARN] wandb is not installed: logging scalars to TensorBoard event files instead")
                    from ..rl.tb_writer import SummaryWriter

                    self.logger = SummaryWriter(log_dir=cfg.log_dir)
                else:
                    self.logger = wandb.init(project=cfg.wandb_project, config=cfg.to_dict(), name=os.path.basename(cfg.log_dir))
            self.teacher_policy_inference = teacher_policy
            mono = cfg.distillation_type == "Monolithic"
            self.student = Student(cfg, self.proprioception_dim, self.tactile_signal_dim, env.num_actions,
                                   teacher_policy_inference=teacher_policy,
                                   teacher_encoder_inference=None if mono else teacher_encoder,
                                   teacher_backbone_weights=None if mono else teacher_backbone_weights, logger=self.logger, verbose=verbose)
            self.replay_buffer = ReplayBuffer(env, self.tactile_recorder, self.proprioception_dim, device_ledger=device_ledger,
                                              fused_batches=fused_bc_step)
            if fused_bc_step:
                self.student.enable_fused_bc_step()
            if fused_cnn_training:
                if not hasattr(getattr(self.student, "pre_encoder", None), "enable_fused_training"):
                    raise ValueError("Distillation: fused_cnn_training needs a CNN2dHead pre_encoder")
                self.student.pre_encoder.enable_fused_training(self.student.tactile_signal_img_shape)
        else:
            if device_ledger and torch.device(env.device).type != "cuda":  # (play keeps no books, but the switch never passes quietly)
                raise ValueError("Distillation: device_ledger needs a CUDA env")
            self.student = Student(cfg, self.proprioception_dim, self.tactile_signal_dim, env.num_actions, verbose=verbose)
            if checkpoint is not None:
                self.student.load_checkpoint(checkpoint)
                if verbose:
                    print(f"[INFO] Loading student policy checkpoint from: {checkpoint}")
        self.history: list[dict] = []
        self.fused_student = None
        if fused_student_inference:
            from .fused_student import FusedStudent

            self.fused_student = FusedStudent.for_student(self.student)  # ValueError for an architecture the kernels do not serve

    def _acting_student(self):
        return self.student if self.fused_student is None else self.fused_student

    def run(self):
        return self.train() if self.training else self.play()

    def train(self):
        c = self.cfg
        for it in range(c.num_iterations):
            print("-" * 100)
            rewards, lengths = self.replay_buffer.collect_data(
                teacher_policy=self.teacher_policy_inference, student_policy=self._acting_student() if it else None,
                num_steps=c.dagger_data_steps if it else c.bc_data_steps)
            rec = self.log_trajectory_rewards_and_lengths(rewards, lengths, it)
            self.student.train_on_data(self.replay_buffer, it)
            if self.fused_student is not None:
                self.fused_student.refresh()
            rec.update({"iter": it, **{f"train/{k}": v for k, v in self.student.last_stats.items()}})
            self.history.append(rec)
            if it == c.num_iterations - 1:
                self.replay_buffer.clear_buffer()
                rewards, lengths = self.replay_buffer.evaluate(self._acting_student(), c.evaluation_trajs_num)
                self.history.append({"iter": "eval", **self.log_trajectory_rewards_and_lengths(rewards, lengths, it + 1)})
                print("Log dir: ", self.student.log_dir)
        if self.logger is not None:
            (self.logger.close if hasattr(self.logger, "close") else self.logger.finish)()
        return self.history

    def log_trajectory_rewards_and_lengths(self, rewards: list, lengths: list, step: int = 0) -> dict:
        rewards, lengths = np.array(rewards, dtype=np.float64), np.array(lengths, dtype=np.float64)
        if rewards.size == 0:
            return {"collect/trj_num": 0}
        rec = {"collect/trj_num": int(rewards.size), "collect/trj_less_half_len_num": int((lengths < 0.5 * lengths.max()).sum()),
               "collect/step_reward_mean": float(np.mean(rewards / lengths)), "collect/trj_rwd_mean": float(rewards.mean()),
               "collect/trj_rwd_std": float(rewards.std()), "collect/trj_len_mean": float(lengths.mean()),
               "collect/trj_len_std": float(lengths.std())}
        if self.logger is not None:
            if hasattr(self.logger, "add_scalar"):
                for k, v in rec.items():
                    self.logger.add_scalar(k, v, step)
            else:
                self.logger.log(rec, commit=False)
        print(f"Collected {rec['collect/trj_num']} trajectories:")
        print(f"Trajectories less than half length: {rec['collect/trj_less_half_len_num']}")
        print(f"Mean step reward: {rec['collect/step_reward_mean']}")
        print(f"Mean reward: {rec['collect/trj_rwd_mean']}, Std reward: {rec['collect/trj_rwd_std']}")
        print(f"Mean length: {rec['collect/trj_len_mean']}, Std length: {rec['collect/trj_len_std']}")
        return rec

    def play(self, num_steps: int | None = None):
        """distillation.py:172-212: the student drives the env on DELAYED tactile rows; returns the actions of the last step."""
        self.student.eval()
        student = self._acting_student()
        obs, extras = self.env.get_observations()
        groups = dict(extras["observations"])
        action, t = None, 0
        rec = self.tactile_recorder
        fused = not isinstance(rec, TactileRecorder)
        with torch.inference_mode():
            delayed = torch.empty_like(groups["tactile"], memory_format=torch.contiguous_format) if fused else None  # one reused buffer
            while num_steps is None or t < num_steps:
                if fused:
                    groups["tactile"] = rec.push(groups["tactile"], delayed)
                else:
                    rec.record_new_tactile_signals(groups["tactile"])
                    groups["tactile"] = rec.get_tactile_signals().clone()
                action = student.extract_input_and_forward(groups)
                obs, _, dones, extras = self.env.step(action)
                groups = dict(extras["observations"])
                done_mask = dones != 0
                self.tactile_recorder.reset(done_mask)
                student.reset(done_mask)
                t += 1
        return action
