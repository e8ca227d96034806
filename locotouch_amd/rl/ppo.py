"""PPO with clipped surrogate / clipped value loss and the adaptive-KL learning-rate schedule.

Behavioural twin of the reference's `PPO` (loco_rl/loco_rl/algorithms/ppo.py:19-385) for the feed-forward
ActorCritic path the LocoTouch agents use (agents/rsl_rl_ppo_cfg.py:11-30: clip 0.2, gamma 0.99, lam 0.95, lr 1e-3
adaptive, desired KL 0.01, entropy 0.01, value coef 1.0, grad-norm 1.0, 5 epochs x 4 minibatches), with the reference's `symmetry_cfg`
branch (mirrored data augmentation and / or a mirror loss: `_symmetry_update`; on the GPU inside `_direct_update`, include/lt_ppo_sym.h
with augmentation and include/lt_ppo_mirror.h without).  The RND branch is not built: a `rnd_cfg` is refused.
An `ActorCriticEncoder` updates through the op chain, or - behind the opt-in key `fused_encoder_policy` - without an autograd graph
(`_direct_encoder_update`, include/lt_encoder.h).
An `ActorCriticRNNEncoder` updates through the eager loop, or - behind the opt-in key `direct_rnn_encoder_update` - on whole rollouts
of env blocks without an autograd graph (`_direct_rnn_encoder_update`, include/lt_rnn_encoder_train.h).
The updates without an autograd graph (`_direct_update`, `_direct_encoder_update`, `_direct_recurrent_update`,
`_direct_rnn_encoder_update`) share one skeleton -
`_direct_begin`, `_direct_loss_and_rule` per step (for the three that need dx inside `_direct_stacks_step`), `_direct_end` with the update's
one host read - and keep only their own forward and backward passes; the updates that run the loss as torch ops share `_op_chain_loss`.
What the opt-in keys need is stated once (`_keys_unsupported`), and `_update_form` names the update that `update()` runs.

Data parallelism (new): gradients live in one flat fp32 bucket that is all-reduced (mean) between
`backward()` and the gradient clip, and the KL estimate is all-reduced before the learning-rate decision.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _abi
from .dist import Dist
from .modules import ActorCritic
from .storage import RolloutStorage


class PPO:
    def __init__(self, actor_critic: ActorCritic, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998,
                 lam=0.95, value_loss_coef=1.0, entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0,
                 use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01, device="cpu",
                 normalize_advantage_per_mini_batch=False, dist: Dist | None = None, rnd_cfg: dict | None = None,
                 symmetry_cfg: dict | None = None, **unused):
        if rnd_cfg is not None:
            raise NotImplementedError("rnd_cfg: random network distillation is not built (DESIGN.md §7: it needs an `rnd_state` observation "
                                      "group no env here produces); pass rnd_cfg=None")
        self.symmetry = self._resolve_symmetry(symmetry_cfg, actor_critic)
        self._sym_tables = None  # the packed device tables of `_direct_update` (include/lt_ppo_sym.h), built at the first symmetric update
        self.device = device
        self.dist = dist or Dist()
        self.actor_critic = actor_critic.to(device)
        on_gpu = torch.device(device).type == "cuda"
        self.fused_loss = on_gpu and bool(unused.get("fused_loss", True))  # csrc/lt_ppo.hip: the loss chain and its backward in one launch
        self.packed_forward = on_gpu and bool(unused.get("packed_forward", True))  # csrc/lt_mlp.hip: both networks' training forward in one launch
        self.direct_update = on_gpu and bool(unused.get("direct_update", True))  # no autograd graph, no host read between minibatch steps (_direct_update)
        # opt-in: recurrent (LSTM) policies update on whole rollouts of env blocks, without padding (_recurrent_update, rl/memory_seq.py)
        self.fused_recurrent_update = bool(unused.get("fused_recurrent_update", False))
        # opt-in: `fused_recurrent_update` serves GRU memories as well (csrc/lt_memory_gru.hip); on its own it does nothing
        self.fused_gru_memories = bool(unused.get("fused_gru_memories", False))
        # opt-in, on top of `fused_recurrent_update`: that update without an autograd graph or a host read between its steps (_direct_recurrent_update)
        self.direct_recurrent_update = bool(unused.get("direct_recurrent_update", False))
        # opt-in: an `ActorCriticEncoder` updates without an autograd graph or a host read between its minibatch steps (_direct_encoder_update, csrc/lt_encoder.hip)
        self.fused_encoder_policy = bool(unused.get("fused_encoder_policy", False))
        self._encoders = None  # rl/encoder.py EncoderPair, built at the first update (the storage names the rows' widths)
        # opt-in: an `ActorCriticRNNEncoder` updates on whole rollouts of env blocks without padding, an autograd graph or a host read
        # between its steps (_direct_rnn_encoder_update, include/lt_rnn_encoder_train.h)
        self.direct_rnn_encoder_update = bool(unused.get("direct_rnn_encoder_update", False))
        self._rnn_encoders = None  # rl/encoder.py RnnEncoderPair, built at the first update
        self._pair = None
        why = self._keys_unsupported(flat_bucket=False)  # (before anything is broadcast or flattened; the rest below, with the bucket there)
        if why is not None:
            raise ValueError(why)
        if on_gpu and bool(unused.get("tuned_gemms", True)):
            from . import tuned_gemms

            tuned_gemms.enable()  # library-GEMM algorithm selection recorded for this stack (rl/tuned_gemms.py); no run-time tuning
        self.optimizer = torch.optim.Adam(self.actor_critic.parameters(), lr=learning_rate)
        self.storage: RolloutStorage | None = None
        self.learning_rate = learning_rate
        self.schedule, self.desired_kl = schedule, desired_kl
        self.clip_param, self.gamma, self.lam = clip_param, gamma, lam
        self.num_learning_epochs, self.num_mini_batches = num_learning_epochs, num_mini_batches
        self.value_loss_coef, self.entropy_coef, self.max_grad_norm = value_loss_coef, entropy_coef, max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.normalize_advantage_per_mini_batch = normalize_advantage_per_mini_batch
        self._t = {}
        self._flat_grad: torch.Tensor | None = None
        # clip_grad_norm_ + Adam.step() in two launches on flat buffers (rl/flat_adam.py); the tensors the module and the optimizer
        # hold become views of those buffers, checkpoints keep the reference's layout
        self._flat_adam = None
        use_flat_adam = on_gpu and bool(unused.get("fused_adam", True))
        if self.dist.world_size > 1:
            if not use_flat_adam:
                self._make_flat_grad_bucket()
            self.broadcast_parameters()
        if use_flat_adam:
            from .flat_adam import FlatAdam

            self._flat_adam = FlatAdam(self.optimizer)
            self._flat_grad = self._flat_adam.flat_g  # also the all-reduce bucket of a multi-rank job
        why = self._keys_unsupported(flat_bucket=True)
        if why is not None:
            raise ValueError(why)

    def _keys_unsupported(self, flat_bucket: bool) -> str | None:
        """Why the opt-in keys that are set cannot be served, with the key's name in front (None: they can): what is refused is never
        run on another path.  `flat_bucket`: the optimizer's flat bucket exists, so what a form needs of it and of the kernels behind
        it is asked as well (`_direct_stacks_unsupported` builds `self._pair`); without it only what can be said before that."""
        ac, kind = self.actor_critic, type(self.actor_critic).__name__
        ranks = device = None  # what every graph-free opt-in form needs: one rank and a GPU
        if self.dist.world_size > 1:
            ranks = (f"dist.world_size is {self.dist.world_size}: the collectives of this form are not covered by a multi-rank test, it runs "
                     "on one rank only")
        if torch.device(self.device).type != "cuda":
            device = f"the device is {self.device!r}: its kernels run on a GPU only"
        if kind == "ActorCriticRNNEncoder":  # (first, whatever the device: the keys of the other kinds do not serve this class)
            for key in ("fused_encoder_policy", "direct_recurrent_update", "fused_recurrent_update"):
                if getattr(self, key):
                    return (f"{key}: the policy is an ActorCriticRNNEncoder: its update is the eager one (the key serves "
                            f"{'ActorCriticEncoder' if key == 'fused_encoder_policy' else 'ActorCriticRecurrent'})")
        if self.fused_encoder_policy:
            if self.fused_recurrent_update or self.direct_recurrent_update or self.fused_gru_memories:
                return ("fused_encoder_policy: the recurrent keys (fused_recurrent_update, direct_recurrent_update, fused_gru_memories) "
                        "belong to ActorCriticRecurrent: an encoder policy has no memories")
            if self.symmetry is not None:
                return "fused_encoder_policy: symmetry_cfg is not served for an encoder policy (the mirror tables cover the plain ActorCritic's rows)"
            why = ranks or device or (self._direct_encoder_unsupported() if flat_bucket else None)
            if why is not None:
                return f"fused_encoder_policy: {why}"
        if self.direct_recurrent_update:
            if not self.fused_recurrent_update:
                return "direct_recurrent_update: it is a form of the whole-rollout update: set fused_recurrent_update=True as well"
            why = device or ranks or self._recurrent_update_unsupported() or (self._direct_recurrent_unsupported() if flat_bucket else None)
            if why is not None:
                return f"direct_recurrent_update: {why}"
        if self.fused_recurrent_update:
            why = self._recurrent_update_unsupported()
            if why is not None:
                return f"fused_recurrent_update: {why}"
        if self.direct_rnn_encoder_update:
            if kind != "ActorCriticRNNEncoder":
                why = f"the policy is a {kind}, not an ActorCriticRNNEncoder"
            elif not ac.critic_with_encoder:
                why = "the critic has no encoder"
            else:  # (no word on symmetry_cfg: `_resolve_symmetry` has refused it for this class, whose `is_recurrent` is True)
                why = ranks or device or (self._direct_rnn_encoder_unsupported() if flat_bucket else None)
            if why is not None:
                return f"direct_rnn_encoder_update: {why}"
        return None

    @staticmethod
    def _resolve_symmetry(symmetry_cfg, actor_critic):
        """The reference's `symmetry_cfg` (ppo.py:66-84) as a dict of its own with every key present, or None.  Keys: use_data_augmentation,
        use_mirror_loss, mirror_loss_coeff, data_augmentation_func (callable or 'module:function'), _env (the runner sets it)."""
        if symmetry_cfg is None:
            return None
        known = ("use_data_augmentation", "use_mirror_loss", "mirror_loss_coeff", "data_augmentation_func", "_env")
        other = sorted(set(symmetry_cfg) - set(known))
        if other:
            raise ValueError(f"symmetry_cfg: unknown keys {other} (known: {list(known)})")
        if getattr(actor_critic, "is_recurrent", False):
            raise ValueError("symmetry_cfg: the policy is recurrent: its hidden states have no mirror (the reference does not support it either)")
        sym = dict(use_data_augmentation=False, use_mirror_loss=False, mirror_loss_coeff=0.0, data_augmentation_func=None, _env=None)
        sym.update(symmetry_cfg)
        sym["use_data_augmentation"], sym["use_mirror_loss"] = bool(sym["use_data_augmentation"]), bool(sym["use_mirror_loss"])
        sym["mirror_loss_coeff"] = float(sym["mirror_loss_coeff"] or 0.0)
        if not (sym["use_data_augmentation"] or sym["use_mirror_loss"]):
            import warnings

            warnings.warn("Symmetry not used for learning. We will use it for logging instead.")
        if isinstance(sym["data_augmentation_func"], str):
            from .symmetry import string_to_callable

            sym["data_augmentation_func"] = string_to_callable(sym["data_augmentation_func"])
        if not callable(sym["data_augmentation_func"]):
            raise ValueError(f"symmetry_cfg: data_augmentation_func is not callable: {sym['data_augmentation_func']!r}")
        return sym

    # ---- data-parallel plumbing ------------------------------------------------------------------
    def _make_flat_grad_bucket(self) -> None:
        params = [p for p in self.actor_critic.parameters() if p.requires_grad]
        total = sum(p.numel() for p in params)
        self._flat_grad = torch.zeros(total, device=params[0].device, dtype=params[0].dtype)
        off = 0
        for p in params:
            p.grad = self._flat_grad[off:off + p.numel()].view_as(p)  # gradients accumulate straight into the bucket
            off += p.numel()

    def broadcast_parameters(self) -> None:
        for t in list(self.actor_critic.parameters()) + list(self.actor_critic.buffers()):
            self.dist.broadcast_(t.data, src=0)

    # ---- rollout -----------------------------------------------------------------------------------
    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape,
                     obs_dtype: torch.dtype = torch.float32) -> None:
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape[0], critic_obs_shape[0],
                                      action_shape[0], self.device, obs_dtype=obs_dtype)

    def test_mode(self) -> None:
        self.actor_critic.eval()

    def train_mode(self) -> None:
        self.actor_critic.train()

    def act(self, obs: torch.Tensor, critic_obs: torch.Tensor) -> torch.Tensor:
        ac, t = self.actor_critic, self._t
        if getattr(ac, "is_recurrent", False):  # the state the memories hold BEFORE this step (ppo.py:130-131)
            t["hidden"] = tuple(None if h is None else (tuple(x.clone() for x in h) if isinstance(h, tuple) else h.clone())
                                for h in ac.get_hidden_states())
        t["actions"] = ac.act(obs).detach()
        t["values"] = ac.evaluate(critic_obs).detach()
        t["log_prob"] = ac.get_actions_log_prob(t["actions"]).detach()
        t["mu"] = ac.action_mean.detach()
        t["sigma"] = ac.action_std.detach()
        t["obs"], t["critic_obs"] = obs, critic_obs  # recorded before env.step() overwrites the env's buffers
        return t["actions"]

    def process_env_step(self, rewards: torch.Tensor, dones: torch.Tensor, infos: dict) -> None:
        t = self._t
        rew = rewards.clone()
        if "time_outs" in infos:  # bootstrap the value through time-limit terminations (ppo.py:162-165)
            rew += self.gamma * torch.squeeze(t["values"] * infos["time_outs"].unsqueeze(1).to(self.device), 1)
        self.storage.add(t["obs"], t["critic_obs"], t["actions"], rew, dones, t["values"], t["log_prob"], t["mu"], t["sigma"],
                         hidden_states=t.get("hidden"))
        self._t = {}
        self.actor_critic.reset(dones)

    def compute_returns(self, last_critic_obs: torch.Tensor) -> None:
        last_values = self.actor_critic.evaluate(last_critic_obs).detach()
        self.storage.compute_returns(last_values, self.gamma, self.lam,
                                     normalize_advantage=not self.normalize_advantage_per_mini_batch, dist=self.dist)

    # ---- update ------------------------------------------------------------------------------------
    def _fused_loss_ok(self, b) -> bool:
        ac = self.actor_critic
        st = self.storage
        # (both noise_std_types: the loss kernel forms sigma from `std` or from `log_std`, include/lt_ppo_opts.h)
        return self.fused_loss and st.observations.is_cuda and type(ac) is ActorCritic and st.actions.shape[-1] <= 16

    def _packed_pair(self):
        """PackedPair of the policy's two stacks (None: shapes the MLP kernel does not cover, or `packed_forward=False`)."""
        if not self.packed_forward:
            return None
        if self._pair is None:
            from .mlp import PackedPair, describe

            ac = self.actor_critic
            self._pair = False
            if describe(ac.actor) is not None and describe(ac.critic) is not None:
                try:
                    self._pair = PackedPair(ac.actor, ac.critic)
                except ValueError:
                    self._pair = False
        return self._pair or None

    def _flat_storage(self):
        """(obs, critic obs, [actions, log-probs, advantages, returns, values, mu, sigma]) of the rollout storage as rows."""
        st = self.storage
        f = lambda t: t.flatten(0, 1)  # noqa: E731
        small = [f(t).contiguous() for t in (st.actions, st.actions_log_prob, st.advantages, st.returns, st.values, st.mu, st.sigma)]
        return f(st.observations), f(st.privileged_observations), small

    def _fused_update(self):
        """The update of the plain ActorCritic on the GPU: per minibatch step two row gathers (obs, critic obs), the two MLPs,
        ONE loss launch that reads the seven small per-row tensors of the rollout storage through the minibatch index
        (csrc/lt_ppo.hip), backward, two launches of clip + Adam; one host read per step (the KL of the learning-rate rule,
        ppo.py:273-281), the statistics once at the end.  Same arithmetic as the op chain below (tests/test_hip_ppo_graph.py).

        A `noise_std_type="log"` policy passes `log_std` and takes its gradient back.  `normalize_advantage_per_mini_batch`: ONE
        `lt_adv_stats` launch per update on the update's permutation (the reference reuses it in every epoch, so the statistics of
        minibatch i are the same in every epoch), and the loss launch of minibatch i normalises with its two floats while it loads.
        In a multi-rank job those statistics stay per rank, as the op chain below has them."""
        from .fused_loss import adv_stats, fused_ppo_loss, std_param

        ac, st = self.actor_critic, self.storage
        obs, cobs, small = self._flat_storage()
        stats = torch.zeros(3, device=obs.device)
        pair = self._packed_pair()
        std_p, std_is_log = std_param(ac)
        if pair is not None:
            pair.arm_domain_check()  # the first minibatch of the update reports the largest layer input (LT_MLP_INPUT_CLAMP)
        perm, mb = st.mini_batch_permutation(self.num_mini_batches)
        mb_stats = adv_stats(small[2], perm, mb, self.num_mini_batches) if self.normalize_advantage_per_mini_batch else None
        for step_i in range(self.num_learning_epochs * self.num_mini_batches):
            i = step_i % self.num_mini_batches
            idx = perm[i * mb:(i + 1) * mb]
            # both networks' forward in one launch of the MFMA MLP kernel where their shape allows (rl/mlp.py PackedPair)
            o, co = obs[idx], cobs[idx]
            if o.dtype != torch.float32:  # bf16 observation storage (BASELINE config 5): the update computes in f32
                o, co = o.float(), co.float()
            mu, value = pair(o, co) if pair is not None else (ac.actor(o), ac.critic(co))
            loss, surrogate_loss, value_loss, ent, kl_mean = fused_ppo_loss(
                mu, std_p, value, *small, self.clip_param, self.value_loss_coef, self.entropy_coef,
                self.use_clipped_value_loss, idx=idx, std_is_log=std_is_log, adv_stats=None if mb_stats is None else mb_stats[i])
            # the 1-float KL all-reduce starts here and its host read waits until the backward pass is enqueued: the collective's
            # latency (and the host round trip of the learning-rate rule, ppo.py:273-281) hides under the backward GEMMs; the
            # decision still precedes this step's optimizer update, as in the reference
            kl_handle = self.dist.all_reduce_mean_begin(kl_mean.detach().clone()) if self._adaptive else None
            self._zero_grad()
            loss.backward()
            if self._adaptive:
                self._apply_kl(self.dist.all_reduce_mean_end(kl_handle), reduced=True)
            self._optim_step()
            stats = stats + torch.stack((value_loss, surrogate_loss, ent.detach()))
        n = self.num_learning_epochs * self.num_mini_batches
        sv, ss, se = (stats / n).tolist()
        if pair is not None and pair.domain_violated():
            self._warn_mlp_domain()
        st.clear()
        return sv, ss, se, None, None

    def _direct_update(self, pair, split_buckets: bool = True):
        """The update of the plain ActorCritic on the GPU with NO host read between its minibatch steps and no autograd graph.  The
        skeleton it shares with `_direct_encoder_update`, `_direct_recurrent_update` and `_direct_rnn_encoder_update`: `_direct_begin` (device state, std, bucket
        views, [`lt_adv_stats`]); per step a forward, `_direct_loss_and_rule` - ONE loss launch that also writes d loss / d (mu, value,
        std) (csrc/lt_ppo.hip) and the adaptive-KL learning-rate rule as a one-lane launch on a device scalar (`lt_ppo_lr_rule`,
        ppo.py:273-281) -, the two stacks' backward chains writing their gradients straight into the flat bucket (rl/mlp.py
        `backward_raw`), clip + Adam with the learning rate read from the device (`lt_adam_clip_step_dev`); `_direct_end`: statistics,
        learning rate, saturation count and domain record come back in ONE read.  Arithmetic equal to `_fused_update`
        (tests/test_hip_ppo_graph.py); the host used to wait for the KL of every step - 20 stalls per iteration, ~350 us of idle GPU each.

        This form's own: the rows of both networks gathered through the permutation once per update (with `symmetry_cfg` by
        `lt_sym_gather_rows`, [original; mirrored]: both networks' under augmentation, the actor's alone without), the same rows in the split format, the packed forward on them, and the gradient
        all-reduce of a multi-rank job around the backward pass.  Log-type std and per-minibatch advantage normalisation as in
        `_fused_update`: `log_std` and its slot of the bucket stand where `std` and its slot do, the statistics come from one
        `lt_adv_stats` launch per update and stay per rank in a multi-rank job."""
        ac, fa, sym = self.actor_critic, self._flat_adam, self.symmetry
        # The reference draws ONE permutation per update and reuses it in every epoch (rollout_storage.py:189): the two observation
        # matrices are gathered through it once - minibatch i of every epoch is rows [i mb, (i + 1) mb) of the permuted copies -
        # instead of 2 x 16 us of row gathers in each of the 20 steps.  (The small per-row tensors are read through the index
        # by the loss kernel itself.)
        perm, m = self.storage.mini_batch_permutation(self.num_mini_batches)
        c = self._direct_begin("direct_update", pair, perm, m, symmetric=sym is not None)
        obs, cobs, dev, grad_of = c.obs, c.cobs, c.dev, c.grad_of
        critic_at = fa.offset_of(next(iter(ac.critic.parameters())))
        two_buckets = split_buckets and 0 < critic_at < self._flat_grad.numel()
        sym_args = None
        mirror_only = sym is not None and not sym["use_data_augmentation"]
        if sym is None:
            rows = crows = m  # rows of a minibatch in the actor's and in the critic's forward
            perm_o, perm_co = obs[perm], cobs[perm]
            if perm_o.dtype != torch.float32:  # bf16 observation storage (BASELINE config 5): the update computes in f32
                perm_o, perm_co = perm_o.float(), perm_co.float()
        elif mirror_only:
            # the mirror loss without augmentation, or the symmetry loss for the log alone (include/lt_ppo_mirror.h): the ACTOR runs on
            # [original; mirrored], gathered once as below; the critic, the surrogate and the value loss keep their m rows, and the two
            # networks share launches with a row count each (include/lt_mlp_rows.h)
            rows, crows = 2 * m, m
            tab_o, _, tab_a = self._symmetry_tables(dev, obs.shape[1], None, c.a_dim)
            perm_o, perm_co = self._symmetry_gather(obs, perm, m, tab_o), cobs[perm]
            if perm_co.dtype != torch.float32:
                perm_co = perm_co.float()
            sym_args = ("lt_ppo_loss_mirror", tab_a, float(sym["mirror_loss_coeff"]) if sym["use_mirror_loss"] else 0.0)
        else:
            # the mirror-augmented update (include/lt_ppo_sym.h): ONE gather per network writes every minibatch as 2 m contiguous f32 rows
            # [original; mirrored]; the statistics above are those of the original rows (ppo.py:223-225 runs before the repeat)
            rows = crows = 2 * m
            tab_o, tab_co, tab_a = self._symmetry_tables(dev, obs.shape[1], cobs.shape[1], c.a_dim)
            perm_o, perm_co = (self._symmetry_gather(x, perm, m, t) for x, t in ((obs, tab_o), (cobs, tab_co)))
            sym_args = ("lt_ppo_loss_sym", tab_a, float(sym["mirror_loss_coeff"]) if sym["use_mirror_loss"] else 0.0)
        # with no mirror term in the loss (logged only) the mirrored rows carry no gradient: the actor's backward pass runs on the first m
        # rows, a prefix of every buffer, and both networks have m rows there again
        brows = m if mirror_only and not sym["use_mirror_loss"] else rows
        # the same rows in the MLP kernels' split format (f16 hi | f16 lo): what the first layer's weight gradient multiplies, 20 times
        split_o = (pair.split_rows(perm_o), pair.split_rows(perm_co)) if pair._fused_backward_possible(perm_o[:rows], perm_co[:crows]) else None
        for step_i in range(self.num_learning_epochs * self.num_mini_batches):
            i = step_i % self.num_mini_batches
            idx = perm[i * m:(i + 1) * m]
            o, co = perm_o[i * rows:(i + 1) * rows], perm_co[i * crows:(i + 1) * crows]
            xs = (split_o[0][i * rows:i * rows + brows], split_o[1][i * crows:(i + 1) * crows]) if split_o is not None else None
            (mu, value), acts = pair.forward_raw(o, co)
            dmu, dvalue, acc = self._direct_loss_and_rule(c, mu, value, idx, m, i, sym_args)
            if brows != rows:
                o, dmu, acts = o[:brows], dmu[:brows], ([a[:brows] for a in acts[0]], acts[1])
            if self.dist.world_size > 1 and two_buckets:
                # the bucket in two halves (std + actor | critic): the actor's all-reduce runs on RCCL's stream under the critic's
                # three weight-gradient launches (~105 us at 24 576 rows), only the critic's half stays exposed
                handles = []
                pair.backward_raw(o, co, acts, dmu, dvalue, grad_of, xs, after_first=lambda: handles.append(self.dist.all_reduce_mean_begin(self._flat_grad[:critic_at])),
                                  dy_amax=(acc[20:21], acc[21:22]))
                # (a backward pass on the library path never calls back: the whole bucket then)
                handles.append(self.dist.all_reduce_mean_begin(self._flat_grad[critic_at:] if handles else self._flat_grad))
                for h in handles:
                    self.dist.all_reduce_mean_end(h)
            else:
                pair.backward_raw(o, co, acts, dmu, dvalue, grad_of, xs, dy_amax=(acc[20:21], acc[21:22]))
                if self.dist.world_size > 1:
                    self.dist.all_reduce_mean_(self._flat_grad)  # RCCL all-reduce of the policy gradients over xGMI
            fa.step_dev(self.max_grad_norm, c.lr_dev)
        return self._direct_end(c, with_dx=False)

    def _direct_begin(self, key: str, pair, index, m: int, symmetric: bool = False):
        """What the graph-free updates set up alike, as one namespace: the storage's rows (`obs`, `cobs`, `small` with its
        one-column tensors as vectors), `a_dim`, the device `state` ([0] learning rate, [1..3] sums of (value loss, surrogate, entropy),
        with `symmetric` [4] of the symmetry loss) and its views `lr_dev` and `stats`, the bucket's `grad_of`, the std parameter
        (`std_p`, `std_is_log`, `std_c`), the `stream`, the armed domain check of `pair`, and `mb_stats`: `lt_adv_stats` of the
        minibatches that are consecutive runs of `m` entries of `index` (None without per-minibatch normalisation).  `key` names the
        form in a refusal."""
        from types import SimpleNamespace

        from .fused_loss import adv_stats, std_param

        obs, cobs, small = self._flat_storage()
        small = [t.view(-1) if t.shape[-1] == 1 else t for t in small]
        a_dim = small[0].shape[1]
        if a_dim > 16:
            raise ValueError(f"{key}: the action width is {a_dim}: the loss kernel serves at most 16")
        dev = obs.device
        state = torch.zeros(5 if symmetric else 4, device=dev)
        state[0] = self.learning_rate
        std_p, std_is_log = std_param(self.actor_critic)
        pair.arm_domain_check()
        mb_stats = adv_stats(small[2], index, m, self.num_mini_batches) if self.normalize_advantage_per_mini_batch else None
        return SimpleNamespace(pair=pair, obs=obs, cobs=cobs, small=small, a_dim=a_dim, dev=dev, state=state, lr_dev=state[:1], stats=state[1:4],
                               grad_of=self._flat_adam.grad_views(), std_p=std_p, std_is_log=std_is_log, std_c=std_p.detach(),
                               stream=_abi.stream(dev), mb_stats=mb_stats)

    def _direct_loss_and_rule(self, c, mu, value, idx, m: int, i: int, sym_args=None):
        """One step's loss launch and learning-rate launch, for every graph-free update: -> (dmu, dvalue, acc).  The loss entry reads the
        small per-row tensors through `idx` (m rows; minibatch `i` of the update) and writes d loss / d (mu, value), its sums and the
        gradient maxima acc[20], acc[21]: with `sym_args` = (entry, action table, mirror coefficient) `lt_ppo_loss_sym` on [original; mirrored]
        rows of both networks or `lt_ppo_loss_mirror` on those rows of the actor and the m original rows of the critic, `lt_ppo_loss_opts` for a log-type std or per-minibatch statistics, else `lt_ppo_loss`.  `lt_ppo_lr_rule` then applies the
        adaptive-KL rule (ppo.py:273-281) to the device learning rate, adds the step's statistics to `c.stats` and writes d loss / d std
        into its slot of the bucket."""
        dev = c.dev
        dmu = torch.empty_like(mu)
        dvalue = torch.empty(value.shape[0], 1, device=dev, dtype=torch.float32)
        acc = torch.empty(24, device=dev, dtype=torch.float32)
        out = torch.empty(24, device=dev, dtype=torch.float32)
        rows = (mu, c.std_c, value, *c.small, idx, m, c.a_dim, float(self.clip_param), float(self.value_loss_coef), float(self.entropy_coef),
                int(bool(self.use_clipped_value_loss)))
        opts = (int(c.std_is_log), None if c.mb_stats is None else c.mb_stats[i])
        if sym_args is not None:
            _abi.call(sym_args[0], *rows, *opts, *sym_args[1:], dmu, dvalue, acc, out, c.state[4:5], c.stream)
        elif c.std_is_log or c.mb_stats is not None:
            _abi.call("lt_ppo_loss_opts", *rows, *opts, dmu, dvalue, acc, out, c.stream)
        else:
            _abi.call("lt_ppo_loss", *rows, dmu, dvalue, acc, out, c.stream)
        kl = None
        if self._adaptive:
            kl = out[4:5]
            if self.dist.world_size > 1:  # every rank must take the same decision; the collective is stream-ordered
                kl = self.dist.all_reduce_mean_(kl.clone())
        _abi.call("lt_ppo_lr_rule", kl, float(self.desired_kl or 0.0), 1e-5, 1e-2, 1.5, c.lr_dev, c.stats, out, c.grad_of[c.std_p], c.a_dim, c.stream)
        return dmu, dvalue, acc

    def _direct_stacks_step(self, c, x_a, x_c, idx, m: int, i: int):
        """One step of the two stacks for the forms whose rows `x_a`, `x_c` come out of an encoder or a memory: the packed forward,
        `_direct_loss_and_rule`, both backward chains into the bucket -> (dx_a, dx_c), the gradient w.r.t. those rows (include/lt_mlp_dx.h)."""
        (mu, value), acts = c.pair.forward_raw(x_a, x_c, with_dx=True)
        dmu, dvalue, acc = self._direct_loss_and_rule(c, mu, value, idx, m, i)
        dx = (torch.empty_like(x_a), torch.empty_like(x_c))
        c.pair.backward_raw(x_a, x_c, acts, dmu, dvalue, c.grad_of, dy_amax=(acc[20:21], acc[21:22]), dx_out=dx)
        return dx

    def _direct_end(self, c, with_dx: bool):
        """The end of every graph-free update: ONE host read (the device state, the backward chain's saturation count, the domain record),
        the learning rate written back, the two warnings, the storage cleared -> the update's 5-tuple.  `with_dx`: the backward passes
        were given `dx_out`."""
        pair, state = c.pair, c.state
        sat, dom = pair.saturated(), pair.domain_max
        pair.domain_max = None
        zero = state.new_zeros(1)
        read = torch.cat((state, zero if sat is None else sat, zero if dom is None else dom.view(1))).tolist()  # the update's only host read
        (lr, sv, ss, se), (nsat, dmax) = read[:4], read[-2:]
        if nsat > 0:
            import warnings

            sat.zero_()
            entry = "lt_mlp_backward_pair_dx" if with_dx and pair._dx_kernel_ok() else "lt_mlp_backward_pair"
            warnings.warn(f"{entry}: {int(nsat)} workgroup-layers of the gradient chain reached the f16 image's bound "
                          "(a gradient grew by more than 500x through the layers): those rows were saturated; set LT_FUSED_BACKWARD=0 "
                          "to run the chain as f32 library GEMMs")
        self.learning_rate = lr
        for group in self.optimizer.param_groups:
            group["lr"] = lr
        if dmax >= float(_abi.CONSTS["LT_MLP_INPUT_CLAMP"]):
            self._warn_mlp_domain()
        self.storage.clear()
        n = self.num_learning_epochs * self.num_mini_batches
        return sv / n, ss / n, se / n, None, read[4] / n if state.numel() == 5 else None

    def _symmetry_tables(self, dev, obs_dim: int, critic_obs_dim: int | None, a_dim: int):
        """The packed device tables (policy rows, critic rows, actions) of the env's mirror map, checked on the host by
        `lt_sym_table_pack` and built once per PPO object.  `critic_obs_dim` None: the critic sees no mirrored row (the update without
        augmentation), its table is not packed and stands as None."""
        if self._sym_tables is None:
            from .symmetry import mirror_tables

            tables = mirror_tables(self.symmetry["_env"])
            packed = []
            for kind, width in (("policy", obs_dim), ("critic", critic_obs_dim), ("action", a_dim)):
                if width is None:
                    packed.append(None)
                    continue
                src, sign = tables.of(kind)
                if src.numel() != width:
                    raise ValueError(f"symmetry_cfg: the env's {kind} mirror table covers {src.numel()} columns, the storage's rows have {width}")
                buf = torch.empty(width, device=dev, dtype=torch.int32)
                _abi.call("lt_sym_table_pack", src.contiguous(), sign.contiguous(), width, buf, _abi.stream(dev))
                packed.append(buf)
            self._sym_tables = tuple(packed)
        return self._sym_tables

    @staticmethod
    def _symmetry_gather(storage_rows, perm, m: int, table):
        """f32 [nmb * 2 * m, D]: minibatch b as rows [2 b m, 2 (b + 1) m) = [its m storage rows; their mirror images] (`lt_sym_gather_rows`)."""
        R, D = storage_rows.shape
        nmb = perm.numel() // m
        if storage_rows.dtype not in (torch.float32, torch.bfloat16) or not storage_rows.is_contiguous():
            raise ValueError(f"symmetry_cfg: observation rows are {storage_rows.dtype}, contiguous={storage_rows.is_contiguous()}: f32 or bf16 rows are served")
        out = torch.empty(nmb * 2 * m, D, device=storage_rows.device, dtype=torch.float32)
        _abi.call("lt_sym_gather_rows", storage_rows, int(storage_rows.dtype == torch.bfloat16), R, D, perm, nmb, m, table, out,
                  _abi.stream(storage_rows.device))
        return out

    def _symmetry_direct_ok(self) -> bool:
        """Whether `_direct_update` serves this symmetric update: any of the four modes with this package's `mirror_go1` (the kernels
        mirror through its tables) on the conditions the direct update has without symmetry, on one rank; without augmentation the two
        networks differ in their row counts, which the fused backward pass alone serves.  Everything else runs `_symmetry_update`."""
        from .symmetry import mirror_go1

        sym = self.symmetry
        if not (sym["data_augmentation_func"] is mirror_go1 and self.dist.world_size == 1):
            return False
        if not self._fused_loss_ok(None) or self._one_row_minibatches() or not self._graph_free_ok():
            return False
        pair = self._packed_pair()
        if sym["use_data_augmentation"]:
            return True
        dev = self.storage.observations.device
        return pair._fused_backward_possible(*(torch.empty(0, net.in_features, device=dev) for net in (pair.a, pair.b)))

    def _symmetry_update(self):
        """The reference's update with its `symmetry_cfg` branch as a chain of torch ops (ppo.py:216-337), on any device: per-minibatch
        advantage normalisation BEFORE the repeat; observations and actions augmented by `data_augmentation_func` ([original; mirrored]);
        old log-prob, advantages, returns and target values repeated; entropy, mu, sigma and the KL of the learning-rate rule on the first
        B rows; surrogate and value loss as means over all num_aug * B rows; the symmetry loss MSE(mean_actions[B:],
        mirror(mean_actions[:B]).detach()[B:]), part of the loss with `mirror_loss_coeff` under `use_mirror_loss`, else detached for the log.
        sigma is not permuted: the mirrored actions are scored under Normal(mu(mirrored obs), std) with std in its own order."""
        ac, sym = self.actor_critic, self.symmetry
        func, env = sym["data_augmentation_func"], sym["_env"]
        sums = [0.0, 0.0, 0.0, 0.0]
        for b in self.storage.mini_batches(self.num_mini_batches, self.num_learning_epochs):
            B = b.obs.shape[0]
            obs, critic_obs, actions = b.obs, b.critic_obs, b.actions
            old_log_prob, adv, returns, target_values = b.log_prob, b.advantages, b.returns, b.values
            num_aug = 1
            if self.normalize_advantage_per_mini_batch:
                with torch.no_grad():
                    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            if sym["use_data_augmentation"]:
                obs, actions = func(obs=obs, actions=actions, env=env, is_critic=False)
                critic_obs, _ = func(obs=critic_obs, actions=None, env=env, is_critic=True)
                num_aug = int(obs.shape[0] / B)
                old_log_prob, target_values = old_log_prob.repeat(num_aug, 1), target_values.repeat(num_aug, 1)
                adv, returns = adv.repeat(num_aug, 1), returns.repeat(num_aug, 1)
            ac.act(obs)
            log_prob = ac.get_actions_log_prob(actions)
            value = ac.evaluate(critic_obs)
            mu, sigma, entropy = ac.action_mean[:B], ac.action_std[:B], ac.entropy[:B]
            if self._adaptive:
                self._adapt_learning_rate(mu, sigma, b.mu, b.sigma)
            loss, surrogate_loss, value_loss = self._op_chain_loss(log_prob, value, old_log_prob, adv, returns, target_values, entropy.mean())
            if not sym["use_data_augmentation"]:
                obs, _ = func(obs=obs, actions=None, env=env, is_critic=False)
                num_aug = int(obs.shape[0] / B)
            mean_actions = ac.act_inference(obs.detach().clone())
            _, mirrored = func(obs=None, actions=mean_actions[:B], env=env, is_critic=False)
            symmetry_loss = torch.nn.functional.mse_loss(mean_actions[B:], mirrored.detach()[B:])
            if sym["use_mirror_loss"]:
                loss = loss + sym["mirror_loss_coeff"] * symmetry_loss
            else:
                symmetry_loss = symmetry_loss.detach()
            self._zero_grad()
            loss.backward()
            self._optim_step()
            for k, v in enumerate((value_loss, surrogate_loss, entropy.mean(), symmetry_loss)):
                sums[k] += v.item()
        n = self.num_learning_epochs * self.num_mini_batches
        self.storage.clear()
        return sums[0] / n, sums[1] / n, sums[2] / n, None, sums[3] / n

    def _warn_mlp_domain(self) -> None:
        import warnings

        self.mlp_domain_violations = getattr(self, "mlp_domain_violations", 0) + 1
        warnings.warn("an observation or hidden activation reached the MLP kernel's saturation bound (|x| >= LT_MLP_INPUT_CLAMP, "
                      "include/lt_env.h): the fused forward computes MLP(clamp(x)) there, unlike the fp32 reference; "
                      "construct PPO(..., packed_forward=False) and FusedRollout(..., use_packed_mlp=False) to run the fp32 GEMM path")

    @property
    def _adaptive(self) -> bool:
        return self.desired_kl is not None and self.schedule == "adaptive"

    def _op_chain_loss(self, log_prob, value, old_log_prob, adv, returns, old_values, entropy_mean):
        """(loss, surrogate loss, value loss) of the reference as torch ops (ppo.py:284-302), for every update that runs the op chain."""
        ratio = torch.exp(log_prob - torch.squeeze(old_log_prob))
        a = torch.squeeze(adv)
        surrogate_loss = torch.max(-a * ratio, -a * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)).mean()
        if self.use_clipped_value_loss:
            clipped = old_values + (value - old_values).clamp(-self.clip_param, self.clip_param)
            value_loss = torch.max((value - returns).pow(2), (clipped - returns).pow(2)).mean()
        else:
            value_loss = (returns - value).pow(2).mean()
        return surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy_mean, surrogate_loss, value_loss

    def _adapt_learning_rate(self, mu, sigma, old_mu, old_sigma) -> None:
        with torch.inference_mode():
            kl = torch.sum(torch.log(sigma / old_sigma + 1.0e-5)
                           + (torch.square(old_sigma) + torch.square(old_mu - mu)) / (2.0 * torch.square(sigma)) - 0.5, dim=-1)
            self._apply_kl(torch.mean(kl))

    def _apply_kl(self, kl_mean, reduced: bool = False) -> None:
        with torch.inference_mode():
            if self.dist.world_size > 1 and not reduced:
                kl_mean = self.dist.all_reduce_mean_(kl_mean.clone())
            kl_mean = float(kl_mean)  # host decision, as in the reference (ppo.py:273-281)
        if kl_mean > self.desired_kl * 2.0:
            self.learning_rate = max(1e-5, self.learning_rate / 1.5)
        elif self.desired_kl / 2.0 > kl_mean > 0.0:
            self.learning_rate = min(1e-2, self.learning_rate * 1.5)
        for group in self.optimizer.param_groups:
            group["lr"] = self.learning_rate

    def update(self):
        form = self._update_form()
        return form(self._packed_pair()) if form == self._direct_update else form()  # (the one form that is handed its stacks)

    def _update_form(self):
        """The update that serves this policy, its keys and its storage, as a bound method; the whole decision is here.  An opt-in key
        runs its form or was refused at construction; with `symmetry_cfg` and without, the graph-free update where its conditions hold;
        for the plain class otherwise the fused update; everything else the minibatch loop of `_eager_update`."""
        if self.direct_rnn_encoder_update:
            return self._direct_rnn_encoder_update
        if self.fused_encoder_policy:
            return self._direct_encoder_update
        if self.direct_recurrent_update:
            return self._direct_recurrent_update
        if self.fused_recurrent_update:
            return self._recurrent_update
        if self.symmetry is not None:  # (never a recurrent policy: refused at construction)
            return self._direct_update if self._symmetry_direct_ok() else self._symmetry_update
        if self._fused_loss_ok(None) and not getattr(self.actor_critic, "is_recurrent", False) and not self._one_row_minibatches():
            return self._direct_update if self._graph_free_ok() else self._fused_update
        return self._eager_update

    def _one_row_minibatches(self) -> bool:
        """Per-minibatch advantage normalisation rides on the fused and the graph-free update too; minibatches of one row, whose std is
        NaN in the reference, keep the op chain."""
        return self.normalize_advantage_per_mini_batch and (self.storage.num_envs * self.storage.num_steps) // self.num_mini_batches < 2

    def _graph_free_ok(self) -> bool:
        """What `_direct_update` needs of the PPO object, with `symmetry_cfg` and without: the key, the flat bucket its gradients are
        written into, a std whose gradient the learning-rate launch writes there, and the two stacks as a PackedPair."""
        from .fused_loss import std_param

        return self.direct_update and self._flat_adam is not None and std_param(self.actor_critic)[0].requires_grad and self._packed_pair() is not None

    def _direct_stacks_unsupported(self):
        """What the encoder and recurrent graph-free updates need of the optimizer, the two stacks and std -> (why, None), or, with all of
        it there, (None, the ids of the parameters whose gradients the shared steps write); builds `self._pair`."""
        from .fused_loss import std_param
        from .mlp import PackedPair, describe

        ac = self.actor_critic
        if self._flat_adam is None:
            return "there is no FlatAdam (fused_adam=False): the gradients are written in place into its flat bucket", None
        if not self.packed_forward:
            return "packed_forward is off: the two MLPs run through rl/mlp.py PackedPair", None
        for name, seq in (("actor", ac.actor), ("critic", ac.critic)):
            if describe(seq) is None:
                return f"the MLP kernel does not serve the {name} stack (rl/mlp.py describe: Linear/activation stack, hidden widths <= 512)", None
        try:
            self._pair = PackedPair(ac.actor, ac.critic)
        except ValueError as e:
            return str(e), None
        if self._pair.a.out_features > 16:
            return f"the action width is {self._pair.a.out_features}: the loss kernel serves at most 16", None
        std_p, _ = std_param(ac)
        if not std_p.requires_grad:
            return "std has no gradient: the learning-rate launch writes d loss / d std into its slot of the bucket", None
        return None, {id(std_p)} | {id(p) for seq in (ac.actor, ac.critic) for p in seq.parameters()}

    def _unwritten_gradient(self, written) -> str | None:
        for name, p in self.actor_critic.named_parameters():
            if p.requires_grad and id(p) not in written:
                return f"the parameter {name} has a gradient this form does not write"
        return None

    def _direct_encoder_unsupported(self) -> str | None:
        """What `_direct_encoder_update` needs beyond a GPU and one rank (None: it is all there)."""
        from . import encoder

        ac = self.actor_critic
        if type(ac).__name__ != "ActorCriticEncoder":
            return f"the policy is a {type(ac).__name__}, not an ActorCriticEncoder"
        why, written = self._direct_stacks_unsupported()
        if why is not None:
            return why
        encoders = [("actor_encoder", ac.actor_encoder, ac.actor_flatten_obs_dim)]
        if ac.critic_with_encoder:
            encoders.append(("critic_encoder", ac.critic_encoder, ac.critic_flatten_obs_dim))
        for name, enc, flat in encoders:
            try:  # (the rows' width is the storage's to say: here the narrowest row that holds both parts)
                desc, linears = encoder.describe(enc, flat + enc.model[0].in_features, flat)
            except ValueError as e:
                return f"{name}: {e}"
            if len(linears) > 1 and desc.activation != _abi.CONSTS["LT_ACT_ELU"]:
                return f"{name}: the backward chain of its hidden layers serves ELU (rl/mlp.py backward_chain)"
            written |= {id(p) for p in enc.parameters()}
        return self._unwritten_gradient(written)

    @staticmethod
    def _final_activation_grad(g: torch.Tensor, pre: torch.Tensor, emb: torch.Tensor, kind: int) -> torch.Tensor:
        """g * f'(pre) for the encoder's final activation f (emb = f(pre)): the gradient w.r.t. the pre-activation embedding."""
        C = _abi.CONSTS
        if kind == C["LT_ACT_TANH"]:
            return g * (1.0 - emb * emb)
        if kind == C["LT_ACT_ELU"]:
            return g * torch.where(pre > 0, torch.ones_like(pre), torch.exp(pre))
        return g * (pre > 0).to(g.dtype)  # LT_ACT_RELU

    def _direct_encoder_update(self):
        """The update of an `ActorCriticEncoder` on the GPU with NO autograd graph and NO host read between its minibatch steps, as
        `_direct_update` is for the plain class and on its skeleton.  What the encoders add.  Once per update: their input columns of
        the permuted rows laid out contiguously (what their first layers' weight gradients multiply).  Per step: `lt_encoder_forward` in
        the training form on the minibatch's rows (include/lt_encoder.h: the rows the stacks read, the encoders' hidden activations,
        the pre-activation embedding) in front of the packed forward; behind the loss, both stacks' backward chains with the gradient
        w.r.t. their input rows (`PackedPair.backward_raw(dx_out=...)`), the final activation's derivative on dx[:, flat_dim:] and
        `backward_chain` of each encoder from that gradient - every gradient written in place into the flat bucket, so the clip norm
        covers the encoders as `clip_grad_norm_(actor_critic.parameters())` does."""
        from .encoder import EncoderPair
        from .mlp import SumJobs, backward_chain

        ac, st, fa, pair = self.actor_critic, self.storage, self._flat_adam, self._pair
        if st.observations.dtype != torch.float32:
            raise ValueError("fused_encoder_policy: bf16 observation rows: the encoder launch reads f32 rows")
        if self._encoders is None:
            try:
                self._encoders = EncoderPair(ac, st.observations.shape[-1], st.privileged_observations.shape[-1])
            except ValueError as e:
                raise ValueError(f"fused_encoder_policy: {e}") from None
        enc = self._encoders
        none = _abi.CONSTS["LT_ACT_NONE"]
        nmb = self.num_mini_batches
        perm, m = st.mini_batch_permutation(nmb)
        c = self._direct_begin("fused_encoder_policy", pair, perm, m)
        dev, grad_of = c.dev, c.grad_of
        perm_o, perm_co = c.obs[perm], c.cobs[perm]
        nets = [(enc.a_desc, enc.a_linears, perm_o)]  # the networks with an encoder
        if enc.c_desc is not None:
            nets.append((enc.c_desc, enc.c_linears, perm_co))
        tails = [rows[:, d.obs_dim - d.enc_in:].contiguous() for d, _, rows in nets]
        for step_i in range(self.num_learning_epochs * nmb):
            i = step_i % nmb
            idx = perm[i * m:(i + 1) * m]
            o, co = perm_o[i * m:(i + 1) * m], perm_co[i * m:(i + 1) * m]
            x_a = torch.empty(m, enc.a_width, device=dev, dtype=torch.float32)
            x_c = torch.empty(m, enc.c_width, device=dev, dtype=torch.float32) if enc.c_desc is not None else co
            enc_acts = enc.forward(o, co, x_a, x_c if enc.c_desc is not None else None, train=True)
            dx = self._direct_stacks_step(c, x_a, x_c, idx, m, i)
            sums = SumJobs()
            for k, (d, linears, _) in enumerate(nets):
                L, flat = d.num_layers, d.flat_dim
                g = dx[k][:, flat:].contiguous()
                if d.final_activation != none:
                    g = self._final_activation_grad(g, enc_acts[k][L - 1], (x_a, x_c)[k][:, flat:], d.final_activation)
                backward_chain([lin.weight for lin in linears], [grad_of[lin.bias] for lin in linears], [grad_of[lin.weight] for lin in linears],
                               tails[k][i * m:(i + 1) * m], enc_acts[k][:L - 1], g, sums)
            sums.launch()
            fa.step_dev(self.max_grad_norm, c.lr_dev)
        return self._direct_end(c, with_dx=True)

    def _direct_recurrent_unsupported(self) -> str | None:
        """What `_direct_recurrent_update` needs beyond `_recurrent_update_unsupported`, a GPU and one rank (None: it is all there)."""
        from .memory_seq import _params

        ac = self.actor_critic
        why, written = self._direct_stacks_unsupported()
        if why is not None:
            return why
        written |= {id(p) for mem in (ac.memory_a, ac.memory_c) for p in _params(mem)}
        return self._unwritten_gradient(written)

    @staticmethod
    def _block_row_index(T: int, N: int, num_mini_batches: int, device=None) -> torch.Tensor:
        """int64 [num_mini_batches, T * per]: idx[i, t * per + j] = t * N + i * per + j, the row of the flattened storage behind row
        t * per + j of env block i (per = N // num_mini_batches; the leftover envs belong to no block, as in the reference's dealing)."""
        per = N // num_mini_batches
        ar = lambda n, *shape: torch.arange(n, device=device, dtype=torch.int64).view(*shape)  # noqa: E731
        return (ar(T, 1, T, 1) * N + ar(num_mini_batches, num_mini_batches, 1, 1) * per + ar(per, 1, 1, per)).reshape(num_mini_batches, T * per)

    def _env_blocks(self, key: str, tails=None):
        """The env blocks of the two graph-free whole-rollout updates, laid out once per update -> (m = T * per, `_block_row_index`,
        per block (observation rows, critic rows, dones as bytes, actor states, critic states at step 0 as [per, H])): the rows contiguous
        [T, per, D], or with `tails` = (width, width) of the RNN-encoder form as [m, D] with their tail columns [T, per, width] as two
        more entries behind them.  `key` names the form in a refusal."""
        from .memory_seq import _dones_bytes

        st, nmb = self.storage, self.num_mini_batches
        if st.saved_hidden_states_a is None or st.saved_hidden_states_c is None:
            raise ValueError(f"{key}: the storage holds no saved hidden states (no rollout of a recurrent policy filled it)")
        T, N = st.num_steps, st.num_envs
        per = N // nmb
        m = T * per
        if per < 1 or (self.normalize_advantage_per_mini_batch and m < 2):
            raise ValueError(f"{key}: {nmb} minibatches of {N} envs x {T} steps leave a block of {m} rows")
        H = self.actor_critic.memory_a.rnn.hidden_size
        idx_all = self._block_row_index(T, N, nmb, st.observations.device)
        dones = _dones_bytes(st.dones.view(T, N))
        blocks = []
        for i in range(nmb):
            sl = (slice(None), slice(i * per, (i + 1) * per))
            states = [tuple(h[0][sl].reshape(per, H) for h in hs) for hs in (st.saved_hidden_states_a, st.saved_hidden_states_c)]
            rows = [st.observations[sl].contiguous(), st.privileged_observations[sl].contiguous()]
            if tails is not None:
                rows = [r.view(m, -1) for r in rows] + [r[..., r.shape[-1] - width:].contiguous() for r, width in zip(rows, tails)]
            blocks.append((*rows, dones[sl], *states))
        return m, idx_all, blocks

    def _direct_recurrent_update(self):
        """`_recurrent_update` with NO autograd graph and NO host read between its steps, as `_direct_update` is to `_fused_update` and
        on its skeleton.  What the memories add.  Once per update: the env blocks' observation rows laid out contiguously, their states
        at step 0, and the row index of every block into the flattened storage - the minibatch index of the loss launch and of
        `lt_adv_stats`.  Per optimizer step: the cell's `seq_forward` (rl/memory_seq.py `direct_forward`) in front of the packed forward
        on its [T * per, H] outputs; behind the loss, both stacks' backward chains with the gradient w.r.t. their input rows
        (`PackedPair.backward_raw(dx_out=...)`, include/lt_mlp_dx.h), the cell's `seq_backward` from those rows and the memories' eight
        parameter gradients (`direct_backward`) - every gradient written in place into the flat bucket."""
        why = self._recurrent_update_unsupported()  # (with the storage now: the observation rows' dtype)
        if why is not None:
            raise ValueError(f"direct_recurrent_update: {why}")
        from .memory_seq import cell_of, direct_backward, direct_forward

        ac, fa, nmb = self.actor_critic, self._flat_adam, self.num_mini_batches
        m, idx_all, blocks = self._env_blocks("direct_recurrent_update")
        cell = cell_of(ac.memory_a, self.fused_gru_memories)
        H = ac.memory_a.rnn.hidden_size
        c = self._direct_begin("direct_recurrent_update", self._pair, idx_all.view(-1), m)
        for step_i in range(self.num_learning_epochs * nmb):
            i = step_i % nmb
            obs, cobs, d, hc_a, hc_c = blocks[i]
            recs = direct_forward(cell, ac.memory_a, ac.memory_c, obs, cobs, d, hc_a, hc_c)
            dx = self._direct_stacks_step(c, recs[0]["out"].view(m, H), recs[1]["out"].view(m, H), idx_all[i], m, i)
            direct_backward(cell, ac.memory_a, ac.memory_c, obs, cobs, d, recs, dx, c.grad_of)
            fa.step_dev(self.max_grad_norm, c.lr_dev)
        return self._direct_end(c, with_dx=True)

    def _direct_rnn_encoder_unsupported(self) -> str | None:
        """What `_direct_rnn_encoder_update` needs beyond the class with an encoder in its critic, a GPU and one rank (None: it is all there)."""
        from . import encoder
        from .memory_seq import _params, memories_unsupported

        ac = self.actor_critic
        why, written = self._direct_stacks_unsupported()
        if why is not None:
            return why
        why = memories_unsupported(ac.memory_a, ac.memory_c, gru_memories=True, layer_count=True)
        if why is not None:
            return why
        try:  # (the rows' width is the storage's to say: here the narrowest row that holds both parts)
            encoder.RnnEncoderPair(ac, ac.actor_flatten_obs_dim + ac.actor_encoder_obs_dim, ac.critic_flatten_obs_dim + ac.critic_encoder_obs_dim)
        except ValueError as e:
            return str(e)
        written |= {id(p) for mem in (ac.memory_a, ac.memory_c) for p in _params(mem)}
        written |= {id(p) for enc in (ac.actor_encoder, ac.critic_encoder) for p in enc.parameters()}
        return self._unwritten_gradient(written)

    def _direct_rnn_encoder_update(self):
        """The update of an `ActorCriticRNNEncoder` on the GPU with NO autograd graph, NO padded trajectories and NO host read between its
        steps: `_direct_recurrent_update` with the encoders between the memories and the stacks, on the same skeleton and the same env
        blocks.  Once per update and block: the observation rows laid out contiguously (their head columns are read in place), their tail
        columns as [T, per, enc_in] (what the sequence kernels and dW_ih read), the dones as bytes, the states saved at step 0.  Per
        optimizer step: the cell's `seq_forward` on the tails; `lt_rnn_encoder_forward_train` on the memories' outputs (the rows the
        stacks read, the encoders' activations); the packed forward; the loss and the learning-rate rule; both stacks' backward chains
        with the gradient w.r.t. their input rows; `lt_rnn_encoder_backward` from the embedding columns of those rows (ONE launch:
        every layer's dz and the gradient w.r.t. the memories' outputs) and the encoders' weight and bias gradients
        (`RnnEncoderPair.backward`); the cell's `seq_backward` from that gradient and the memories' eight parameter gradients
        (`direct_backward`) - every gradient written in place into the flat bucket.  LSTM and GRU memories alike, as the rollout key."""
        from .encoder import RnnEncoderPair
        from .memory_seq import cell_of, direct_backward, direct_forward

        ac, st, fa, nmb = self.actor_critic, self.storage, self._flat_adam, self.num_mini_batches
        if st.observations.dtype != torch.float32 or st.privileged_observations.dtype != torch.float32:
            raise ValueError("direct_rnn_encoder_update: bf16 observation rows: the memories and the encoder launch read f32 rows")
        if self._rnn_encoders is None:
            try:
                self._rnn_encoders = RnnEncoderPair(ac, st.observations.shape[-1], st.privileged_observations.shape[-1])
            except ValueError as e:
                raise ValueError(f"direct_rnn_encoder_update: {e}") from None
        enc = self._rnn_encoders
        m, idx_all, blocks = self._env_blocks("direct_rnn_encoder_update", tails=(ac.actor_encoder_obs_dim, ac.critic_encoder_obs_dim))
        cell = cell_of(ac.memory_a, True)
        H = ac.memory_a.rnn.hidden_size
        c = self._direct_begin("direct_rnn_encoder_update", self._pair, idx_all.view(-1), m)
        dev, grad_of = c.dev, c.grad_of
        for step_i in range(self.num_learning_epochs * nmb):
            i = step_i % nmb
            rows_a, rows_c, tail_a, tail_c, d, hc_a, hc_c = blocks[i]
            recs = direct_forward(cell, ac.memory_a, ac.memory_c, tail_a, tail_c, d, hc_a, hc_c)
            hs = (recs[0]["out"].view(m, H), recs[1]["out"].view(m, H))
            x_a = torch.empty(m, enc.a_width, device=dev, dtype=torch.float32)
            x_c = torch.empty(m, enc.c_width, device=dev, dtype=torch.float32)
            enc_acts = enc.forward_train(rows_a, rows_c, *hs, x_a, x_c)
            dx = self._direct_stacks_step(c, x_a, x_c, idx_all[i], m, i)
            dh = enc.backward(dx, (x_a, x_c), enc_acts, grad_of, hs)
            direct_backward(cell, ac.memory_a, ac.memory_c, tail_a, tail_c, d, recs, dh, grad_of)
            fa.step_dev(self.max_grad_norm, c.lr_dev)
        return self._direct_end(c, with_dx=True)

    def _recurrent_update_unsupported(self) -> str | None:
        """Why `_recurrent_update` does not serve this policy / storage (None: it does)."""
        from .memory_seq import unsupported
        from .modules import ActorCriticRecurrent

        ac = self.actor_critic
        if type(ac) is not ActorCriticRecurrent:
            return f"the policy is a {type(ac).__name__}: only a plain ActorCriticRecurrent is served"
        st = getattr(self, "storage", None)  # (None at construction: the observation rows' dtype is checked at the first update)
        return unsupported(ac.memory_a, ac.memory_c, *((None, None) if st is None else (st.observations, st.privileged_observations)),
                           gru_memories=self.fused_gru_memories)

    def _recurrent_update(self):
        """The update of an `ActorCriticRecurrent` with LSTM (with `fused_gru_memories`: or GRU) memories on WHOLE ROLLOUTS of env blocks (rl/memory_seq.py: why this equals
        the padded trajectories of `_eager_update`): no `split_and_pad_trajectories`, no `recurrent_mini_batches`, no boolean indexing.
        Per optimizer step: the env block [e0, e1) of the reference's dealing (per = N // num_mini_batches, leftover envs dropped), both
        memories over its T steps from the states saved at step 0 (`memory_rollout_sequence`; on the GPU csrc/lt_memory.hip), the two
        MLPs on the [T, per, H] outputs, the loss (one launch, csrc/lt_ppo.hip, where its conditions hold; else the op chain of
        `_eager_update`), the learning-rate rule, backward, clip + Adam.  The statistics stay on the device until the last step."""
        why = self._recurrent_update_unsupported()
        if why is not None:
            raise ValueError(f"fused_recurrent_update: {why}")
        from .memory_seq import memory_rollout_sequence

        ac, st = self.actor_critic, self.storage
        if st.saved_hidden_states_a is None or st.saved_hidden_states_c is None:
            raise ValueError("fused_recurrent_update: the storage holds no saved hidden states (no rollout of a recurrent policy filled it)")
        T, N = st.num_steps, st.num_envs
        per = N // self.num_mini_batches
        dones = st.dones.view(T, N)  # uint8 [T, N]
        fused = (self.fused_loss and st.observations.is_cuda and getattr(ac, "noise_std_type", "scalar") == "scalar" and st.actions.shape[-1] <= 16)
        if fused:
            from .fused_loss import fused_ppo_loss
        # the env blocks are the same in every epoch: their observation rows are laid out contiguously ONCE per update (what the weight
        # gradient dW_ih = dgates^T X multiplies); everything else of a block is a view of the storage
        blocks = []
        for i in range(self.num_mini_batches):
            sl = (slice(None), slice(i * per, (i + 1) * per))
            blocks.append((sl, st.observations[sl].contiguous(), st.privileged_observations[sl].contiguous()))
        stats = torch.zeros(3, device=st.observations.device, dtype=st.values.dtype)
        for _ in range(self.num_learning_epochs):
            for sl, obs, cobs in blocks:
                hc_a = tuple(h[0][sl] for h in st.saved_hidden_states_a)
                hc_c = tuple(h[0][sl] for h in st.saved_hidden_states_c)
                out_a, out_c = memory_rollout_sequence(ac.memory_a, ac.memory_c, obs, cobs, dones[sl], hc_a, hc_c,
                                                       gru_memories=self.fused_gru_memories)
                adv = st.advantages[sl]
                if self.normalize_advantage_per_mini_batch:
                    with torch.no_grad():
                        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
                old_mu, old_sigma, old_values, returns = st.mu[sl], st.sigma[sl], st.values[sl], st.returns[sl]
                if fused:
                    f = lambda t: t.reshape(T * per, -1)  # noqa: E731  (row t * per + e, the order of the memories' outputs)
                    loss, surrogate_loss, value_loss, ent, kl_mean = fused_ppo_loss(
                        ac.actor(out_a.view(T * per, -1)), ac.std, ac.critic(out_c.view(T * per, -1)), f(st.actions[sl]),
                        f(st.actions_log_prob[sl]), f(adv), f(returns), f(old_values), f(old_mu), f(old_sigma), self.clip_param,
                        self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss)
                    if self._adaptive:
                        self._apply_kl(kl_mean)
                    ent = ent.detach()
                else:
                    ac.update_distribution(out_a)
                    log_prob = ac.get_actions_log_prob(st.actions[sl])
                    value = ac.critic(out_c)
                    mu, sigma, ent = ac.action_mean, ac.action_std, ac.entropy.mean()
                    if self._adaptive:
                        self._adapt_learning_rate(mu, sigma, old_mu, old_sigma)
                    loss, surrogate_loss, value_loss = self._op_chain_loss(log_prob, value, st.actions_log_prob[sl], adv, returns, old_values, ent)
                self._zero_grad()
                loss.backward()
                self._optim_step()
                stats = stats + torch.stack((value_loss.detach(), surrogate_loss.detach(), ent.detach())).to(stats.dtype)
        n = self.num_learning_epochs * self.num_mini_batches
        sv, ss, se = (stats / n).tolist()  # the statistics' only host read
        st.clear()
        return sv, ss, se, None, None

    def _eager_update(self):
        """The reference's minibatch loop (ppo.py:216-337) on any device and for every class: a recurrent policy on padded whole
        trajectories, the loss as one launch where `_fused_loss_ok` holds, else as the op chain."""
        ac = self.actor_critic
        sum_value = sum_surr = sum_ent = 0.0
        stats = None
        recurrent = getattr(ac, "is_recurrent", False)
        batches = (self.storage.recurrent_mini_batches(self.num_mini_batches, self.num_learning_epochs) if recurrent
                   else self.storage.mini_batches(self.num_mini_batches, self.num_learning_epochs))
        for raw in batches:
            if recurrent:  # padded whole trajectories + the hidden states saved at their first steps (ppo.py:195-196,251-256)
                from .storage import Batch

                b, (hid_a, hid_c), masks = Batch(*raw[:9]), raw[9], raw[10]
            else:
                b, hid_a, hid_c, masks = raw, None, None, None
            adv = b.advantages
            if self.normalize_advantage_per_mini_batch:
                with torch.no_grad():
                    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            if self._fused_loss_ok(b):
                # GPU: log-prob, KL, surrogate, value loss, entropy and their gradients in one launch (csrc/lt_ppo.hip)
                from .fused_loss import fused_ppo_loss, std_param

                std_p, std_is_log = std_param(ac)
                loss, surrogate_loss, value_loss, ent, kl_mean = fused_ppo_loss(
                    ac.actor(b.obs), std_p, ac.critic(b.critic_obs), b.actions, b.log_prob, adv, b.returns, b.values, b.mu, b.sigma,
                    self.clip_param, self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss, std_is_log=std_is_log)
                if self._adaptive:
                    self._apply_kl(kl_mean)
                if stats is None:
                    stats = torch.zeros(3, device=loss.device)
                self._zero_grad()
                loss.backward()
                self._optim_step()
                stats = stats + torch.stack((value_loss, surrogate_loss, ent.detach()))  # read once, after the last step
                continue
            if recurrent:
                ac.act(b.obs, masks=masks, hidden_states=hid_a)
                log_prob = ac.get_actions_log_prob(b.actions)
                value = ac.evaluate(b.critic_obs, masks=masks, hidden_states=hid_c)
            else:
                ac.act(b.obs)
                log_prob = ac.get_actions_log_prob(b.actions)
                value = ac.evaluate(b.critic_obs)
            mu, sigma, entropy = ac.action_mean, ac.action_std, ac.entropy
            if self._adaptive:
                self._adapt_learning_rate(mu, sigma, b.mu, b.sigma)
            loss, surrogate_loss, value_loss = self._op_chain_loss(log_prob, value, b.log_prob, adv, b.returns, b.values, entropy.mean())
            self._zero_grad()
            loss.backward()
            self._optim_step()
            sum_value += value_loss.item()
            sum_surr += surrogate_loss.item()
            sum_ent += entropy.mean().item()
        n = self.num_learning_epochs * self.num_mini_batches
        if stats is not None:
            sv, ss, se = stats.tolist()
            sum_value, sum_surr, sum_ent = sum_value + sv, sum_surr + ss, sum_ent + se
        self.storage.clear()
        return sum_value / n, sum_surr / n, sum_ent / n, None, None

    def _zero_grad(self) -> None:
        if self._flat_adam is not None:
            self._flat_adam.zero_grad()
        elif self._flat_grad is not None:
            self._flat_grad.zero_()
        else:
            self.optimizer.zero_grad()

    def _optim_step(self) -> None:
        """All-reduce of the gradients (multi-rank), clip_grad_norm_, Adam (ppo.py:318-319)."""
        if self._flat_adam is not None:
            self._flat_adam.gather_grads()               # one multi-tensor copy into the flat bucket
        if self.dist.world_size > 1:
            self.dist.all_reduce_mean_(self._flat_grad)  # RCCL all-reduce of the policy gradients over xGMI
        if self._flat_adam is not None:
            self._flat_adam.step(self.max_grad_norm, gathered=True)  # clip + Adam in two launches (csrc/lt_ppo.hip)
        else:
            nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
            self.optimizer.step()
