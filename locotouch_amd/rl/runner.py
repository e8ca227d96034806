"""On-policy training loop: rollout (policy act -> env step -> storage) then PPO update, with checkpoints and logging.

Interface of the reference's `OnPolicyRunner` (loco_rl/loco_rl/runners/on_policy_runner.py:21-489):
`OnPolicyRunner(env, train_cfg: dict, log_dir, device)`, `.learn(n, init_at_random_ep_len)`, `.save/.load` with the
checkpoint dict keys `model_state_dict, optimizer_state_dict, iter, infos` (:369-385), `.get_inference_policy`.
Perf scalars keep the reference's names (`Perf/total_fps`, `Perf/collection time`, `Perf/learning_time`, :275,291-293).
The per-step host syncs of the reference's bookkeeping (:197-199) are replaced by device-side accumulators that are
read once per iteration.
"""
from __future__ import annotations

import json
import os
import time
from collections import deque

import torch

from .dist import Dist
from .modules import ActorCritic, ActorCriticEncoder, ActorCriticRecurrent, ActorCriticRNNEncoder
from .normalizer import EmpiricalNormalization
from .ppo import PPO


class OnPolicyRunner:
    def __init__(self, env, train_cfg: dict, log_dir: str | None = None, device="cpu", dist: Dist | None = None):
        self.cfg = dict(train_cfg)
        self.alg_cfg = dict(train_cfg["algorithm"])
        self.policy_cfg = dict(train_cfg["policy"])
        self.device, self.env, self.dist = device, env, dist or Dist()
        obs, extras = env.get_observations()
        self.num_obs = num_obs = obs.shape[1]
        num_critic_obs = extras["observations"]["critic"].shape[1] if "critic" in extras["observations"] else num_obs
        from . import modules as _m

        cls_name = self.policy_cfg.pop("class_name", "ActorCritic")  # on_policy_runner.py:42 (`eval(class_name)`)
        if cls_name not in ("ActorCritic", "ActorCriticRecurrent", "ActorCriticEncoder", "ActorCriticRNNEncoder"):
            raise NotImplementedError(f"policy class {cls_name!r} is not implemented (ActorCritic, ActorCriticRecurrent, ActorCriticEncoder, "
                                      "ActorCriticRNNEncoder are)")
        if cls_name == "ActorCriticRNNEncoder" and self.cfg.get("fused_recurrent_rollout", False):
            raise ValueError("fused_recurrent_rollout: the policy is an ActorCriticRNNEncoder: that key collects an ActorCriticRecurrent; "
                             "fused_rnn_encoder_policy is the key of this class")
        self.alg_cfg.pop("class_name", None)
        if self.cfg.get("fused_rnn_encoder_policy", False) and cls_name != "ActorCriticRNNEncoder":
            raise ValueError(f"fused_rnn_encoder_policy: the policy is a {cls_name}, not an ActorCriticRNNEncoder")
        if self.cfg.get("direct_rnn_encoder_update", False) and cls_name != "ActorCriticRNNEncoder":
            raise ValueError(f"direct_rnn_encoder_update: the policy is a {cls_name}, not an ActorCriticRNNEncoder")
        ac = getattr(_m, cls_name)(num_obs, num_critic_obs, env.num_actions, **self.policy_cfg).to(device)
        if "fused_recurrent_update" in self.cfg:  # opt-in (rl/ppo.py `_recurrent_update`); a refusal is PPO's ValueError
            self.alg_cfg["fused_recurrent_update"] = bool(self.cfg["fused_recurrent_update"])
        if "fused_gru_memories" in self.cfg:  # opt-in: the two switches above / below also serve GRU memories (csrc/lt_memory_gru.hip)
            self.alg_cfg["fused_gru_memories"] = bool(self.cfg["fused_gru_memories"])
        if "direct_recurrent_update" in self.cfg:  # opt-in on top of `fused_recurrent_update` (rl/ppo.py `_direct_recurrent_update`)
            self.alg_cfg["direct_recurrent_update"] = bool(self.cfg["direct_recurrent_update"])
        if "fused_encoder_policy" in self.cfg:  # opt-in: an ActorCriticEncoder on the fused rollout and `_direct_encoder_update`
            self.alg_cfg["fused_encoder_policy"] = bool(self.cfg["fused_encoder_policy"])
        if "direct_rnn_encoder_update" in self.cfg:  # opt-in: an ActorCriticRNNEncoder updates through `_direct_rnn_encoder_update`
            self.alg_cfg["direct_rnn_encoder_update"] = bool(self.cfg["direct_rnn_encoder_update"])
        sym = self.alg_cfg.get("symmetry_cfg")
        if sym is not None:  # on_policy_runner.py:60-63: the augmentation function is handed the env; PPO takes a plain dict
            sym = sym.to_dict() if hasattr(sym, "to_dict") else (dict(sym) if isinstance(sym, dict) else dict(vars(sym)))
            sym["_env"] = env
            self.alg_cfg["symmetry_cfg"] = sym
        self.alg = PPO(ac, device=device, dist=self.dist, **self.alg_cfg)
        self.num_steps_per_env = int(self.cfg["num_steps_per_env"])
        self.save_interval = int(self.cfg.get("save_interval", 50))
        self.alg.init_storage(env.num_envs, self.num_steps_per_env, [num_obs], [num_critic_obs], [env.num_actions])
        # observation normalisers (on_policy_runner.py:85-95); identity unless `empirical_normalization` is set
        self.empirical_normalization = bool(self.cfg.get("empirical_normalization", False))
        if self.empirical_normalization:
            self.obs_normalizer = EmpiricalNormalization(shape=[num_obs], until=1.0e8).to(device)
            self.critic_obs_normalizer = EmpiricalNormalization(shape=[num_critic_obs], until=1.0e8).to(device)
        else:
            self.obs_normalizer = self.critic_obs_normalizer = torch.nn.Identity().to(device)
        self.log_dir = log_dir if self.dist.is_main else None
        self.writer = None
        self.logger_type = str(self.cfg.get("logger", "tensorboard")).lower()
        self.tot_timesteps, self.tot_time, self.current_learning_iteration = 0, 0.0, 0
        self.history: list[dict] = []
        self.git_status_repos: list[str] = []

    def learn(self, num_learning_iterations: int, init_at_random_ep_len: bool = False) -> None:
        env, alg = self.env, self.alg
        if self.log_dir is not None and self.writer is None:  # on_policy_runner.py:98-118
            if self.logger_type == "tensorboard":
                from .tb_writer import SummaryWriter

                self.writer = SummaryWriter(self.log_dir, flush_secs=10)
            elif self.logger_type in ("wandb", "neptune"):
                raise NotImplementedError(f"logger {self.logger_type!r} needs a network service; use --logger tensorboard (quirk Q9: the "
                                          "reference's agent cfgs default to wandb)")
            else:
                raise ValueError("Logger type not found. Please choose 'neptune', 'wandb' or 'tensorboard'.")
        if init_at_random_ep_len:  # on_policy_runner.py:121-124
            env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))
        obs, extras = env.get_observations()
        critic_obs = extras["observations"].get("critic", obs)
        obs, critic_obs = obs.to(self.device), critic_obs.to(self.device)
        self.train_mode()
        n = env.num_envs
        fused = self._make_fused()
        if fused is not None:
            fused.begin()  # with normalisers: the env's current rows are merged once and normalised, as `it == start` below does
        rew_acc = torch.zeros(n, device=self.device)
        len_acc = torch.zeros(n, device=self.device)
        rewbuffer, lenbuffer = deque(maxlen=100), deque(maxlen=100)
        start = self.current_learning_iteration
        for it in range(start, start + num_learning_iterations):
            t0 = time.time()
            fin_rew, fin_len = [], []
            if fused is not None:
                # GPU path: GEMMs + fused kernels, episode statistics from the env's device-side accumulators
                fused.rollout(self.num_steps_per_env)
                fused.normalize_storage()  # (nothing without normalisers) the slots hold raw rows until here
                with torch.inference_mode():
                    alg.compute_returns(fused.last_critic_obs)
            else:
              with torch.inference_mode():
                if it == start:
                    obs, critic_obs = self.obs_normalizer(obs), self.critic_obs_normalizer(critic_obs)
                for _ in range(self.num_steps_per_env):
                    actions = alg.act(obs, critic_obs)
                    obs, rewards, dones, infos = env.step(actions.to(env.device))
                    obs, rewards, dones = obs.to(self.device), rewards.to(self.device), dones.to(self.device)
                    obs = self.obs_normalizer(obs)                                                    # on_policy_runner.py:163-169
                    critic_obs = self.critic_obs_normalizer(infos["observations"]["critic"].to(self.device)) if "critic" in infos["observations"] else obs
                    alg.process_env_step(rewards, dones, infos)
                    rew_acc += rewards
                    len_acc += 1
                    d = dones > 0
                    fin_rew.append(torch.where(d, rew_acc, torch.full_like(rew_acc, float("nan"))))
                    fin_len.append(torch.where(d, len_acc, torch.full_like(len_acc, float("nan"))))
                    rew_acc = torch.where(d, torch.zeros_like(rew_acc), rew_acc)
                    len_acc = torch.where(d, torch.zeros_like(len_acc), len_acc)
                alg.compute_returns(critic_obs)
            if hasattr(env, "curriculum_sync"):  # multi-rank: one all-reduce of the curriculum sums per rollout
                env.curriculum_sync(self.dist, self.num_steps_per_env)
            t1 = time.time()
            value_loss, surrogate_loss, entropy, _, symmetry_loss = alg.update()
            t2 = time.time()
            # one host read per iteration for the episode statistics
            if fin_rew:
                fr, fl = torch.stack(fin_rew).flatten(), torch.stack(fin_len).flatten()
                keep = ~torch.isnan(fr)
                rewbuffer.extend(fr[keep].tolist())
                lenbuffer.extend(fl[keep].tolist())
            self.current_learning_iteration = it
            collect, learn = t1 - t0, t2 - t1
            steps = self.num_steps_per_env * n * self.dist.world_size
            self.tot_timesteps += steps
            self.tot_time += collect + learn
            rec = {"iter": it, "Perf/total_fps": steps / (collect + learn), "Perf/collection time": collect,
                   "Perf/learning_time": learn, "Loss/value_function": value_loss, "Loss/surrogate": surrogate_loss,
                   "Loss/entropy": entropy, "Loss/learning_rate": alg.learning_rate,
                   "Policy/mean_noise_std": float(alg.actor_critic.action_std.detach().mean()),
                   "Train/mean_reward": (sum(rewbuffer) / len(rewbuffer)) if rewbuffer else None,
                   "Train/mean_episode_length": (sum(lenbuffer) / len(lenbuffer)) if lenbuffer else None}
            if alg.symmetry is not None:  # on_policy_runner.py:284-285; records of other runs keep their keys
                rec["Loss/symmetry"] = symmetry_loss
            if hasattr(env, "episode_log"):
                rec.update(env.episode_log())
                if fused is not None:  # the env's own per-episode accumulators stand in for rewbuffer / lenbuffer
                    rec["Train/mean_reward"] = rec.get("Episode/reward")
                    rec["Train/mean_episode_length"] = rec.get("Episode/length")
            if getattr(env, "episode_stats", None) is not None:  # --episode_stats: the iteration's finished episodes, then cleared
                rec.update(env.episode_stats.eval_record(clear=True))
            self.history.append(rec)
            if self.log_dir is not None:
                os.makedirs(self.log_dir, exist_ok=True)
                with open(os.path.join(self.log_dir, "progress.jsonl"), "a") as f:
                    f.write(json.dumps(rec) + "\n")
                if self.writer is not None:  # the reference's scalar tags (on_policy_runner.py:268-309), same x axis
                    for k, v in rec.items():
                        if k != "iter" and isinstance(v, (int, float)):
                            self.writer.add_scalar(k, v, it)
                    if rec.get("Train/mean_reward") is not None:
                        self.writer.add_scalar("Train/mean_reward/time", rec["Train/mean_reward"], int(self.tot_time))
                        self.writer.add_scalar("Train/mean_episode_length/time", rec["Train/mean_episode_length"], int(self.tot_time))
                if it % self.save_interval == 0:
                    self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
        # the final model, under the number of the LAST iteration run - the reference's naming (on_policy_runner.py:221,243-245):
        # `current_learning_iteration` is that iteration, and a resumed run starts again from it
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))
            if self.writer is not None:
                self.writer.flush()

    def _make_fused(self):
        """FusedRollout when the env is the HIP env on a GPU and the policy is the plain feed-forward ActorCritic (either noise_std_type), or - behind the cfg
        key `fused_recurrent_rollout` (default False: the fused path draws its exploration noise from the kernels' Philox stream, which
        would change existing runs) - an ActorCriticRecurrent whose memories csrc/lt_memory.hip serves, or - behind `fused_encoder_policy`, for
        the same reason - an ActorCriticEncoder whose encoders csrc/lt_encoder.hip serves, or - behind `fused_rnn_encoder_policy`, again opt-in - an
        ActorCriticRNNEncoder whose memories and encoders include/lt_rnn_encoder.h serves (LSTM or GRU, by that key alone)."""
        try:
            from ..env import LocoTouchVecEnv
            from .fused import FusedRollout, rollout_unsupported
        except Exception:
            return None
        target = self.env
        if not isinstance(target, LocoTouchVecEnv):  # the scripts' wrapper (compat/runtime.py) hands the HIP env over when it adds nothing to a step
            target = getattr(self.env, "fused_target", lambda: None)()
        rnn_encoder_key = bool(self.cfg.get("fused_rnn_encoder_policy", False))  # opt-in, and never quietly dropped: what it cannot serve raises
        if not isinstance(target, LocoTouchVecEnv) or self.cfg.get("fused_rollout", True) is False:
            if rnn_encoder_key:
                raise ValueError("fused_rnn_encoder_policy: there is no fused rollout to put the policy on (the env is not the HIP env, or "
                                 "fused_rollout is off)")
            return None
        ac, kw = self.alg.actor_critic, {}
        if type(ac) is ActorCriticRecurrent:
            if not self.cfg.get("fused_recurrent_rollout", False):
                return None
            kw["fused_gru_memories"] = bool(self.cfg.get("fused_gru_memories", False))
        elif type(ac) is ActorCriticEncoder:
            if not self.cfg.get("fused_encoder_policy", False):
                return None
            kw["fused_encoder_policy"] = True
        elif type(ac) is ActorCriticRNNEncoder:
            if not rnn_encoder_key:
                return None
            kw["fused_rnn_encoder_policy"] = True
        elif type(ac) is not ActorCritic:
            return None  # the fused rollout packs the actor / critic MLPs
        if self.empirical_normalization:
            # The device normaliser (csrc/lt_obs_norm.hip) keeps per-process statistics: ranks cannot all-reduce them per step inside a
            # captured rollout, and one sync per iteration would change what the policy sees.  Multi-rank runs keep the eager loop below.
            if self.dist.world_size > 1:
                return None
            kw.update(obs_normalizer=self.obs_normalizer, critic_obs_normalizer=self.critic_obs_normalizer)
        # what FusedRollout would refuse (a normaliser beside a memory or an encoder or on bf16 rows, shapes outside the kernels' limits): the
        # eager loop - rl/fused.py states it once, for its constructor and for this.  That covers normalisers whose buffers, eps or until
        # the kernels do not serve as well: this runner builds its own, which are served
        why = rollout_unsupported(self.alg, **kw)
        if why is not None:
            if rnn_encoder_key:
                raise ValueError(why)
            return None
        return FusedRollout(target, self.alg, **kw)

    # ---- checkpoints (reference on_policy_runner.py:369-422) -------------------------------------------
    def save(self, path: str, infos=None) -> None:
        if not self.dist.is_main:
            return
        opt_sd = self.alg.optimizer.state_dict()
        for g in opt_sd["param_groups"]:  # the graph-replayed update keeps the learning rate in a device scalar: save a float
            if torch.is_tensor(g.get("lr")):
                g["lr"] = float(g["lr"])
        saved = {"model_state_dict": self.alg.actor_critic.state_dict(),
                 "optimizer_state_dict": opt_sd,
                 "iter": self.current_learning_iteration, "infos": infos}
        if self.empirical_normalization:  # on_policy_runner.py:376-379
            saved["obs_norm_state_dict"] = self.obs_normalizer.state_dict()
            saved["critic_obs_norm_state_dict"] = self.critic_obs_normalizer.state_dict()
        torch.save(saved, path)

    def load(self, path: str, load_optimizer: bool = True, pretrained: bool = False):
        loaded = torch.load(path, map_location=self.device, weights_only=True)
        sd = loaded["model_state_dict"]
        if pretrained:  # actor only + reset exploration noise (reference :404-412)
            actor_sd = {k[len("actor."):]: v for k, v in sd.items() if k.startswith("actor.")}
            self.alg.actor_critic.actor.load_state_dict(actor_sd)
            self.alg.actor_critic.reset_init_std()
        else:
            self.alg.actor_critic.load_state_dict(sd)
            if self.empirical_normalization:  # on_policy_runner.py:413-415
                self.obs_normalizer.load_state_dict(loaded["obs_norm_state_dict"])
                self.critic_obs_normalizer.load_state_dict(loaded["critic_obs_norm_state_dict"])
            if load_optimizer:
                self.alg.optimizer.load_state_dict(loaded["optimizer_state_dict"])
            self.current_learning_iteration = loaded["iter"]
        if self.dist.world_size > 1:
            self.alg.broadcast_parameters()
        return loaded.get("infos")

    def train_mode(self) -> None:  # reference on_policy_runner.py:466-475
        self.alg.train_mode()
        if self.empirical_normalization:
            self.obs_normalizer.train()
            self.critic_obs_normalizer.train()

    def eval_mode(self) -> None:  # reference on_policy_runner.py:477-486
        self.alg.test_mode()
        if self.empirical_normalization:
            self.obs_normalizer.eval()
            self.critic_obs_normalizer.eval()

    def add_git_repo_to_log(self, repo_file_path: str) -> None:
        """Reference on_policy_runner.py:488-489: remembers code locations whose git state goes into the log directory.  There is
        no GitPython in this image, so the paths are recorded (`<log_dir>/git/repos.txt`) and no diff is taken."""
        self.git_status_repos.append(repo_file_path)
        if self.log_dir is not None:
            os.makedirs(os.path.join(self.log_dir, "git"), exist_ok=True)
            with open(os.path.join(self.log_dir, "git", "repos.txt"), "a") as f:
                f.write(str(repo_file_path) + "\n")

    def get_inference_encoder(self, device=None):  # reference on_policy_runner.py:435-448: None unless the policy has an encoder
        self.eval_mode()
        ac = self.alg.actor_critic
        if device is not None:
            ac.to(device)
        if callable(getattr(ac, "act_encoder_inference", None)):
            if self.empirical_normalization:
                return lambda x: ac.act_encoder_inference(self.obs_normalizer(x))
            return ac.act_encoder_inference
        return None

    def get_backbone_weights(self):  # :463-464 (RMA distillation: the teacher's actor becomes the student's frozen backbone)
        return self.alg.actor_critic.actor.state_dict()

    def get_inference_policy(self, device=None, fused=False):  # reference on_policy_runner.py:424-436
        """`fused=True`: the opt-in fronts of rl/fused_policy.py, the normaliser folded into their first launch - `FusedRecurrentPolicy` for
        a recurrent policy (one memory launch and one actor launch per step), `FusedEncoderPolicy` for an ActorCriticRNNEncoder (two
        launches) or an ActorCriticEncoder (one) whose parameters are on a GPU; they raise for what the kernels do not serve.  Everything
        else is the reference's."""
        self.eval_mode()
        if device is not None:
            self.alg.actor_critic.to(device)
        ac = self.alg.actor_critic
        if fused and type(ac) in (ActorCriticEncoder, ActorCriticRNNEncoder):
            if next(ac.parameters()).is_cuda:
                from .fused_policy import FusedEncoderPolicy

                if self.empirical_normalization and device is not None:
                    self.obs_normalizer.to(device)
                return FusedEncoderPolicy.for_actor_critic(ac, self.obs_normalizer if self.empirical_normalization else None, obs_dim=self.num_obs)
            if type(ac) is ActorCriticRNNEncoder:
                raise NotImplementedError("get_inference_policy(fused=True): the fused inference step of an ActorCriticRNNEncoder "
                                          "(rl/fused_policy.py, FusedEncoderPolicy) runs on a GPU only and this policy is on the CPU; "
                                          "fused=False steps it through its modules")
            # (an ActorCriticEncoder on the CPU: the eager policy below, as ever)
        elif fused and getattr(ac, "is_recurrent", False):
            from .fused_policy import FusedRecurrentPolicy

            if self.empirical_normalization and device is not None:
                self.obs_normalizer.to(device)
            return FusedRecurrentPolicy.for_actor_critic(self.alg.actor_critic, self.obs_normalizer if self.empirical_normalization else None)
        policy = self.alg.actor_critic.act_inference
        if self.empirical_normalization:
            if device is not None:
                self.obs_normalizer.to(device)
            policy = lambda x: self.alg.actor_critic.act_inference(self.obs_normalizer(x))  # noqa: E731
        return policy
