"""Fused rollout step on the GPU, semantically one iteration of the reference's rollout loop
(loco_rl/loco_rl/runners/on_policy_runner.py:154-199):
`actions = alg.act(obs, critic_obs); obs, rew, dones, infos = env.step(actions); alg.process_env_step(rew, dones, infos)`.

Packed path (network shapes lt_mlp.hip covers - every LocoTouch agent config): launches on ONE stream,
    [lt_rollout_policy_value: actor + critic MLPs, sampling, log-prob, storage writes of actions/mu/sigma/values/log-prob]
 -> [lt_env_step_rollout: env step, observation rows written into storage slot t+1, bootstrapped reward + dones into slot t;
     the one-wave population pass of the PREVIOUS step (curriculum decision / population gate) rides in this launch, on an idle
     wave beside the physics (lt_env_defer_gate mode 2); one explicit pass closes the rollout]
with no host sync, so a whole 24-step rollout captures into one hipGraph.  The chain is kept linear on purpose: forked
streams turn graph edges into cross-queue dependencies that cost more than the overlap returns (measured again with the
population pass on a side branch beside the next policy launch, lt_env_defer_gate: 99.8 us per step against 86.3 us linear).

Torch path (shapes outside lt_mlp's limits): torch GEMMs -> lt_rollout_act -> lt_env_step_rows -> lt_rollout_record, with the
critic on a side stream.

Log-type std (`ActorCritic(noise_std_type="log")`): the policy launches read sigma from a [12] buffer of this object, which ONE
`lt_std_from_log` launch at the head of every rollout refreshes from `log_std` (include/lt_ppo_opts.h) - inside a captured region, so a
replayed graph follows the optimizer.  The launches of a step are the same two.

What a kind of policy adds to a step stands in ONE class per kind, a "front" (`_Front` and its subclasses: their docstrings describe the step).
"""
from __future__ import annotations


import torch

from .. import _abi
from .memory_seq import cell_of, memories_unsupported


def recurrent_unsupported(ac, storage, gru_memories: bool = False) -> str | None:
    """Why the fused rollout does not serve this recurrent policy (None: it does): include/lt_memory.h covers two single-layer f32 LSTM
    memories with biases of one hidden size, a multiple of 64 in [64, 512], on f32 observation rows.  `gru_memories=True` (the opt-in
    `fused_gru_memories`): two GRUs of the same description are served as well (include/lt_memory_gru.h), an LSTM beside a GRU is not."""
    mems = (getattr(ac, "memory_a", None), getattr(ac, "memory_c", None))
    if any(m is None for m in mems):
        return "the policy has no memory_a / memory_c"
    why = memories_unsupported(*mems, gru_memories=gru_memories)  # (the checks rl/memory_seq.py `unsupported` makes as well)
    if why is not None:
        return why
    for name, m in zip(("memory_a", "memory_c"), mems):
        if m.rnn.weight_ih_l0.dtype != torch.float32:
            return f"{name} is not f32"
    if storage.observations.dtype != torch.float32:
        return "bf16 observation rows: the memory step reads f32 rows"
    return None


def encoder_policy_unsupported(alg, normalizers: bool, use_packed_mlp: bool = True) -> str | None:
    """Why the fused rollout does not serve this policy behind `fused_encoder_policy` (None: it does): an `ActorCriticEncoder` on a GPU
    whose encoders include/lt_encoder.h serves and whose stacks lt_mlp serves, on f32 observation rows, without normalisers."""
    from .encoder import EncoderPair
    from .mlp import describe

    ac, st = alg.actor_critic, alg.storage
    if torch.device(alg.device).type != "cuda":
        return f"the device is {alg.device!r}: its kernels run on a GPU only"
    if type(ac).__name__ != "ActorCriticEncoder":
        return f"the policy is a {type(ac).__name__}, not an ActorCriticEncoder"
    if normalizers:
        return "empirical_normalization is not served together with an encoder policy: the normaliser would have to feed the encoder launch"
    if st.observations.dtype != torch.float32:
        return "bf16 observation rows: the encoder launch reads f32 rows"
    if not use_packed_mlp or describe(ac.actor) is None or describe(ac.critic) is None:
        return "the actor or the critic stack is outside lt_mlp's limits (rl/mlp.py describe), or use_packed_mlp is off"
    try:
        EncoderPair(ac, st.observations.shape[-1], st.privileged_observations.shape[-1])
    except ValueError as e:
        return str(e)
    return None


def rnn_encoder_policy_unsupported(alg, normalizers: bool, use_packed_mlp: bool = True) -> str | None:
    """Why the fused rollout does not serve this policy behind `fused_rnn_encoder_policy` (None: it does): an `ActorCriticRNNEncoder` on a
    GPU with an encoder on both networks, two single-layer f32 memories of one kind (LSTM or GRU) and one hidden size within
    include/lt_memory.h's limits, encoders include/lt_rnn_encoder.h serves and stacks lt_mlp serves, on f32 observation rows, without
    normalisers."""
    from .encoder import RnnEncoderPair
    from .mlp import describe

    ac, st = alg.actor_critic, alg.storage
    if torch.device(alg.device).type != "cuda":
        return f"the device is {alg.device!r}: its kernels run on a GPU only"
    if type(ac).__name__ != "ActorCriticRNNEncoder":
        return f"the policy is a {type(ac).__name__}, not an ActorCriticRNNEncoder"
    if not ac.critic_with_encoder:
        return "the critic has no encoder (critic_encoder_hidden_dims=None): the step's launches serve two memories and two encoders"
    if normalizers:
        return "empirical_normalization is not served together with an RNN-encoder policy: the normaliser would have to feed the memory launch"
    if st.observations.dtype != torch.float32:
        return "bf16 observation rows: the memory step and the encoder launch read f32 rows"
    why = memories_unsupported(ac.memory_a, ac.memory_c, gru_memories=True, layer_count=True)
    if why is not None:
        return why
    for name, m in (("memory_a", ac.memory_a), ("memory_c", ac.memory_c)):
        if m.rnn.weight_ih_l0.dtype != torch.float32:
            return f"{name} is not f32"
    if not use_packed_mlp or describe(ac.actor) is None or describe(ac.critic) is None:
        return "the actor or the critic stack is outside lt_mlp's limits (rl/mlp.py describe), or use_packed_mlp is off"
    try:
        RnnEncoderPair(ac, st.observations.shape[-1], st.privileged_observations.shape[-1])
    except ValueError as e:
        return str(e)
    return None


def normalizers_unsupported(alg, actor_norm, critic_norm) -> str | None:
    """Why the fused rollout does not serve these running normalisers (None: it does): both networks' or neither's, on f32 observation
    rows, with the buffers of rl/normalizer.py on the rollout's device and one `eps` and `until` (the same launches serve both)."""
    if (actor_norm is None) != (critic_norm is None):
        return "FusedRollout takes both obs_normalizer and critic_obs_normalizer, or neither"
    st = alg.storage
    if st.observations.dtype == torch.bfloat16:
        return "observation normalisers and bf16 observation rows are not served together: the normaliser kernels read and write f32 rows"
    for nm, d in zip((actor_norm, critic_norm), (st.observations.shape[-1], st.privileged_observations.shape[-1])):
        bufs = (nm._mean, nm._var, nm._std)
        if any(b.shape != (1, d) or b.dtype != torch.float32 or b.device != st.observations.device or not b.is_contiguous() for b in bufs):
            return f"normaliser buffers must be contiguous f32 [1, {d}] tensors on {st.observations.device}"
        if nm.count.dtype != torch.int64 or nm.count.device != st.observations.device:
            return "normaliser count must be an int64 scalar on the rollout's device"
    if float(actor_norm.eps) != float(critic_norm.eps) or actor_norm.until != critic_norm.until:
        return "both normalisers are served by the same launches: they must share eps and until"
    return None


def rollout_unsupported(alg, obs_normalizer=None, critic_obs_normalizer=None, fused_gru_memories: bool = False,
                        fused_encoder_policy: bool = False, use_packed_mlp: bool = True, fused_rnn_encoder_policy: bool = False,
                        kind_only: bool = False) -> str | None:
    """Why `FusedRollout` does not serve this policy with these normalisers and keys (None: it does), in the words its constructor raises:
    the one statement of what is served, which the runner's `_make_fused` asks as well.  The kind's reason comes first (behind the
    encoder keys nothing else is reached: their checks refuse any normaliser), then the normalisers' own, which `kind_only=True` leaves out."""
    ac = alg.actor_critic
    norms = obs_normalizer is not None or critic_obs_normalizer is not None
    if fused_encoder_policy:  # (first: what the key needs is refused by name, whatever else is wrong)
        why = encoder_policy_unsupported(alg, norms, use_packed_mlp)
        return None if why is None else f"fused_encoder_policy: {why}"
    if fused_rnn_encoder_policy:  # (the same rule for this key)
        why = rnn_encoder_policy_unsupported(alg, norms, use_packed_mlp)
        return None if why is None else f"fused_rnn_encoder_policy: {why}"
    if type(ac).__name__ == "ActorCriticRNNEncoder":
        return "FusedRollout does not serve ActorCriticRNNEncoder without fused_rnn_encoder_policy: its memories read the rows' tail columns"
    if getattr(ac, "is_recurrent", False):
        why = recurrent_unsupported(ac, alg.storage, gru_memories=fused_gru_memories)
        if why is None and obs_normalizer is not None:
            why = "observation normalisers are not served together with a recurrent policy"
        if why is not None:
            return f"FusedRollout does not serve this recurrent policy: {why}"
    elif type(ac).__name__ == "ActorCriticEncoder":
        return "FusedRollout does not serve ActorCriticEncoder: its encoders are not part of the fused step"
    return normalizers_unsupported(alg, obs_normalizer, critic_obs_normalizer) if norms and not kind_only else None


def _obs_norm_workspace(n: int, d: int, device, have: torch.Tensor | None = None) -> torch.Tensor:
    """The workspace of one normaliser on [n, d] rows (`have` when it still fits), zeroed: it carries the recurrence's f64 state (lt_obs_norm.h)."""
    import ctypes

    floats = ctypes.c_size_t()
    _abi.call("lt_obs_norm_ws_floats", n, d, ctypes.byref(floats))
    if have is not None and have.numel() == floats.value and have.device == device:
        return have
    return torch.zeros(floats.value, device=device)


def normalize_rows(normalizer, rows: torch.Tensor, out: torch.Tensor | None = None, snapshot: torch.Tensor | None = None) -> torch.Tensor:
    """`normalizer(rows)` of ONE EmpiricalNormalization on the device path (csrc/lt_obs_norm.hip): in training mode the rows are
    merged into the module's buffers in place (no host read), then normalised.  `snapshot` ([2, D]) receives (mean, 1 / (std + eps)).
    FusedRollout serves both networks of a rollout with the same launches; this is the single-module form for tools and tests."""
    n, d = rows.shape
    if rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError("normalize_rows takes contiguous f32 rows")
    out = torch.empty_like(rows) if out is None else out
    snapshot = torch.empty(2, d, device=rows.device) if snapshot is None else snapshot
    ws = normalizer._lt_obs_norm_ws = _obs_norm_workspace(n, d, rows.device, getattr(normalizer, "_lt_obs_norm_ws", None))
    _abi.call("lt_obs_norm_update", n, int(normalizer.training), -1 if normalizer.until is None else int(normalizer.until),
              float(normalizer.eps), rows, d, normalizer._mean, normalizer._var, normalizer._std, normalizer.count, snapshot, out, ws,
              None, 0, None, None, None, None, None, None, None, _abi.stream(rows.device))
    return out


class _Front:
    """What ONE kind of policy puts in front of the policy + value launch of a step and around a rollout; `FusedRollout` holds exactly one
    and knows a kind through these hooks alone (DESIGN.md "Kinds of policy" says when each is called).  This base is the plain
    feed-forward policy: no launch, the stacks read the slot's rows, every other hook does nothing."""
    launches = 0  # the launches it adds to a step
    cell = encoders = normalizers = norm_rows = None

    def __init__(self, fr: "FusedRollout", *kind):  # (every front is built as kind(fr, actor_norm, critic_norm, gru_memories))
        self.env, self.alg, self.device, self.rows_in_storage = fr.env, fr.alg, fr.device, fr.rows_in_storage
        self.last_critic_obs = fr.env.obs_critic  # the critic rows behind the last step as the critic sees them (for `compute_returns`)

    begin = ready = open = after_env_step = finish = close = normalize_storage = lambda self, *args: None

    def rows(self, t: int, obs, cobs, launch: bool = True):
        """The rows the two stacks read at step t, behind what this kind launches in front of them (`launch=False`: as that launch left them)."""
        return obs, cobs


class _NormalizerFront(_Front):
    """Observation normalisation (the runner's `empirical_normalization`, rl/normalizer.py): with normalisers a step is
        [policy + value on the NORMALISED rows of slot t] -> [env step: raw rows into slot t + 1] -> [lt_obs_norm_update: merge the new raw
        rows of both networks into the running statistics, snapshot (mean, 1 / (std + eps)) for slot t + 1, normalised rows into two
        scratch buffers - two launches, one in evaluation mode]
    still on the one stream.  The storage slots stay RAW during the rollout (the step kernel shifts its observation history from slot t
    to slot t + 1), `normalize_storage()` rewrites them in place through the per-slot snapshots before the update reads them."""

    def __init__(self, fr, actor_norm, critic_norm, *_):
        super().__init__(fr)
        st, n = self.alg.storage, self.env.num_envs
        dims = (st.observations.shape[-1], st.privileged_observations.shape[-1])
        # running observation normalisers (rl/normalizer.py): their buffers ARE the device state the kernels update in place
        self.normalizers = (actor_norm, critic_norm)
        # rows the networks read: the normalised rows of the current slot (the slots themselves stay raw until normalize_storage())
        self.norm_rows = (torch.zeros(n, dims[0], device=self.device), torch.zeros(n, dims[1], device=self.device))
        self.last_critic_obs = self.norm_rows[1]
        # per-slot snapshots (mean, 1 / (std + eps)) of both networks, one row per slot: [T + 1][2 * Da + 2 * Dc]; slot 0 of a rollout
        # takes the snapshot behind the last step of the one before (`_carry`), or the one of begin()
        self._snaps = torch.zeros(st.observations.shape[0] + 1, 2 * (dims[0] + dims[1]), device=self.device)
        self._carry = torch.zeros(2 * (dims[0] + dims[1]), device=self.device)
        self._snap_off = (0, 2 * dims[0])
        self._norm_ws = [_obs_norm_workspace(n, d, self.device) for d in dims]
        self._primed = False

    @property
    def launches(self) -> int:
        return 2 if self.normalizers[0].training else 1  # column statistics, merge + snapshot + normalise

    def snapshots(self, which: int) -> torch.Tensor:
        """[T + 1, 2, D] view of the per-slot snapshots (mean, 1 / (std + eps)) of network `which` (0 policy, 1 critic)."""
        d = self.norm_rows[which].shape[1]
        return self._snaps[:, self._snap_off[which]:self._snap_off[which] + 2 * d].unflatten(1, (2, d))

    def _normalize(self, rows, critic_rows, snap_row: torch.Tensor) -> None:
        """Merge the raw rows of both networks into the running statistics (training mode only: normalizer.py `forward`), write the
        snapshots into `snap_row` and the normalised rows into `norm_rows` - two launches, one in evaluation mode."""
        a, c = self.normalizers
        nets = []
        for nm, x, off, out, ws in zip((a, c), (rows, critic_rows), self._snap_off, self.norm_rows, self._norm_ws):
            nets += [x, x.shape[1], nm._mean, nm._var, nm._std, nm.count, snap_row[off:], out, ws]
        _abi.call("lt_obs_norm_update", self.env.num_envs, int(a.training), -1 if a.until is None else int(a.until), float(a.eps), *nets,
                  _abi.stream(self.device))

    def begin(self) -> None:
        """The env's current rows are merged once and normalised (the runner's eager loop does the same before its first step).  Later
        rollouts carry the rows and the snapshot behind their last step over; a rollout calls this itself when nobody has - call it
        yourself before capturing a rollout into a graph, or the replays merge these rows again."""
        with torch.inference_mode():
            self._normalize(self.env.obs_policy, self.env.obs_critic, self._carry)
        self._primed = True

    def ready(self) -> None:
        if not self._primed:
            self.begin()

    def open(self) -> None:
        self._snaps[0].copy_(self._carry)

    def rows(self, t: int, obs, cobs, launch: bool = True):
        return self.norm_rows

    def after_env_step(self, t: int, last: bool) -> None:
        """The raw rows step t has just produced (slot t + 1, or the env's rows) -> statistics, snapshot t + 1, normalised rows."""
        st = self.alg.storage
        if self.rows_in_storage and not last:
            self._normalize(st.observations[t + 1], st.privileged_observations[t + 1], self._snaps[t + 1])
        else:
            self._normalize(self.env.obs_policy, self.env.obs_critic, self._snaps[t + 1])

    def close(self, num_steps: int) -> None:
        self._carry.copy_(self._snaps[num_steps])

    def normalize_storage(self) -> None:
        """Rewrite the storage's observation rows in place through the per-slot snapshots (one launch per network): every update
        path then consumes normalised rows without knowing.  Once per rollout, after its last step; the next rollout refills slot 0
        from the env's rows, which stay raw."""
        st = self.alg.storage
        steps, n = st.step, self.env.num_envs
        with torch.inference_mode():
            for rows, off in zip((st.observations, st.privileged_observations), self._snap_off):
                _abi.call("lt_obs_norm_apply", rows, steps * n, rows.shape[-1], self._snaps[0, off:], self._snaps.shape[1], n, rows,
                          _abi.stream(self.device))


class _MemoryFront(_Front):
    """Recurrent policies (`ActorCriticRecurrent` with two single-layer memories of one kind - LSTM, or GRU with `fused_gru_memories=True`; the
    runner's `fused_recurrent_rollout`): a step is
        [the cell's `step`: both memories - reset mask of the previous step's dones, the pre-step state into the storage's
         `saved_hidden_states` slot t, the cell on the observation rows of slot t, the new raw state into a ping-pong buffer]
     -> [policy + value on the two h buffers] -> [env step]
    and one launch of the cell's `finish` behind the last step leaves where(dones[T-1], 0, state) in the modules' `hidden_states` (DESIGN.md
    4 "Recurrent rollout step").  What differs between the kinds stands in the `Cell` table of rl/memory_seq.py: the state is (h, c) or h
    alone, the launches are `lt_memory_step` / `lt_memory_finish` (csrc/lt_memory.hip) or `lt_memory_gru_step` / `lt_memory_gru_finish`
    (csrc/lt_memory_gru.hip) - both a cell on the one row-block kernel of csrc/lt_memory_tile.h."""
    launches = 1  # both memories in one launch

    def __init__(self, fr, actor_norm, critic_norm, gru_memories: bool):
        super().__init__(fr)
        st, ac, n = self.alg.storage, self.alg.actor_critic, self.env.num_envs
        self.cell = cell_of(ac.memory_a, gru_memories)  # the memories' kind (rl/memory_seq.py `LSTM` / `GRU`)
        hid = ac.memory_a.rnn.hidden_size
        steps = st.observations.shape[0]
        rows = n + (-n) % 64  # (the MLP launch reads whole row tiles)
        ns = len(self.cell.state)  # state tensors per memory: (h, c), or h alone
        # _hc[parity][network] = (h, c), or (h,): step t reads parity (t - 1) & 1 - at t = 0 the modules' own state - and writes parity t & 1
        self._hc = [[tuple(torch.zeros(rows, hid, device=self.device) for _ in range(ns)) for _ in range(2)] for _ in range(2)]
        for name in ("saved_hidden_states_a", "saved_hidden_states_c"):
            saved = getattr(st, name)
            if saved is None:
                setattr(st, name, [torch.zeros(steps, 1, n, hid, device=self.device) for _ in range(ns)])
            elif len(saved) != ns or any(s.shape != (steps, 1, n, hid) or s.dtype != torch.float32 or not s.is_contiguous() for s in saved):
                raise ValueError(f"storage.{name} must be [{', '.join(f[0] for f in self.cell.state)}] of contiguous f32 ({steps}, 1, {n}, {hid}) tensors")
        self._state = None  # the modules' state tensors of both memories, adopted by begin()

    def _adopt_state(self) -> None:
        """The modules' `hidden_states` become the rollout's state tensors (zeros when a memory has none yet): step 0 reads them,
        the cell's `finish` writes them."""
        ac, n = self.alg.actor_critic, self.env.num_envs
        ns = len(self.cell.state)
        one = ns == 1  # a module with one state tensor holds the tensor itself, as its nn module takes it, not a 1-tuple
        state = []
        for name, mem in (("memory_a", ac.memory_a), ("memory_c", ac.memory_c)):
            hid = mem.rnn.hidden_size
            if mem.hidden_states is None:
                zeros = tuple(torch.zeros(1, n, hid, device=self.device) for _ in range(ns))
                mem.hidden_states = zeros[0] if one else zeros
            hc = (mem.hidden_states,) if one else mem.hidden_states
            if (not isinstance(hc, tuple) or len(hc) != ns
                    or any(not torch.is_tensor(x) or x.shape != (1, n, hid) or x.dtype != torch.float32 or x.device != self._hc[0][0][0].device
                           for x in hc)):
                raise ValueError(f"{name}.hidden_states must be {'the tensor' if one else 'a tuple'} ({', '.join(f[0] for f in self.cell.state)}) "
                                 f"of f32 [1, {n}, {hid}] on {self.device}")
            if not all(x.is_contiguous() for x in hc):
                hc = tuple(x.contiguous() for x in hc)
                mem.hidden_states = hc[0] if one else hc
            state.append(hc)
        self._state = state

    # at the head of every rollout too, for the tensors the modules hold NOW: `compute_returns` advances the critic memory by one evaluate,
    # which rebinds its state (a captured rollout keeps the addresses it was captured with: replay it only while the modules keep them)
    begin = ready = _adopt_state

    def _memory_step(self, t: int, obs, cobs) -> None:
        """Step t of both memories in one launch; the h buffers of parity t & 1 are then the input rows of the MLPs."""
        ac, st = self.alg.actor_critic, self.alg.storage
        src = self._state if t == 0 else self._hc[(t - 1) & 1]
        dst = self._hc[t & 1]
        nets = []
        for k, (mem, x, saved) in enumerate(((ac.memory_a, obs, st.saved_hidden_states_a), (ac.memory_c, cobs, st.saved_hidden_states_c))):
            rnn = mem.rnn
            # the structure's fields in order: x, I, the four parameters, h_in[, c_in], h_out[, c_out], saved_h[, saved_c]
            nets.append(self.cell.step_net(x.data_ptr(), x.shape[1], rnn.weight_ih_l0.data_ptr(), rnn.weight_hh_l0.data_ptr(),
                                           rnn.bias_ih_l0.data_ptr(), rnn.bias_hh_l0.data_ptr(), *(s.data_ptr() for s in src[k]),
                                           *(d.data_ptr() for d in dst[k]), *(s[t].data_ptr() for s in saved)))
        _abi.call(self.cell.step, nets[0], nets[1], st.dones[t - 1] if t > 0 else None, self.env.num_envs, ac.memory_a.rnn.hidden_size,
                  _abi.stream(self.device))

    def _memory_rows(self, t: int):
        """The rows the MLPs of step t read: the new h of both memories."""
        n = self.env.num_envs
        return self._hc[t & 1][0][0][:n], self._hc[t & 1][1][0][:n]

    def rows(self, t: int, obs, cobs, launch: bool = True):
        if launch:
            self._memory_step(t, obs, cobs)
        return self._memory_rows(t)

    def finish(self, num_steps: int) -> None:
        """h_a[, c_a], h_c[, c_c] of the last step, masked by its dones, into the modules' state tensors in the same order."""
        raw, st = self._hc[(num_steps - 1) & 1], self.alg.storage
        _abi.call(self.cell.finish, *raw[0], *raw[1], st.dones[num_steps - 1], self.env.num_envs,
                  self.alg.actor_critic.memory_a.rnn.hidden_size, *self._state[0], *self._state[1], _abi.stream(self.device))


class _EncoderFront(_Front):
    """Encoder policies (`ActorCriticEncoder`, behind `fused_encoder_policy=True`: the noise comes from the kernels' Philox stream): a step is
        [lt_encoder_forward: storage slot t -> the rows the stacks read, [head columns | embedding of the tail columns], for the actor and,
         when it has an encoder, the critic (include/lt_encoder.h; it reads the live parameters, nothing is packed)]
     -> [policy + value on those rows (a critic without an encoder reads its slot as ever)] -> [env step]
    three launches on the one stream; the storage keeps the raw rows, `compute_returns` stays the eager `evaluate`."""
    launches = 1  # the encoders of both networks in one launch

    def __init__(self, fr, *_):
        from .encoder import EncoderPair

        super().__init__(fr)
        st, n = self.alg.storage, self.env.num_envs
        if fr.actor_mlp is None:
            raise ValueError("fused_encoder_policy: the env has no 12 actions: the policy launch samples 12")
        # the descriptors of the policy's encoders, and the rows the stacks read: [head columns | embedding] per network
        self.encoders = EncoderPair(self.alg.actor_critic, st.observations.shape[-1], st.privileged_observations.shape[-1])
        rows = n + (-n) % 64  # (the MLP launch reads whole row tiles)
        self._enc_rows = (torch.zeros(rows, self.encoders.a_width, device=self.device),
                          torch.zeros(rows, self.encoders.c_width, device=self.device) if self.encoders.c_desc is not None else None)

    def rows(self, t: int, obs, cobs, launch: bool = True):
        """One launch: the rows of this step's slot -> the rows the two stacks read."""
        if launch:
            self.encoders.forward(obs, cobs, *self._enc_rows)
        n = self.env.num_envs
        out_a, out_c = self._enc_rows
        return out_a[:n], cobs if out_c is None else out_c[:n]


class _RnnEncoderFront(_MemoryFront):
    """RNN-encoder policies (`ActorCriticRNNEncoder`, behind `fused_rnn_encoder_policy=True`: the noise comes from the kernels' Philox
    stream): a step is
        [the cell's strided step (include/lt_rnn_encoder.h): both memories on the TAIL columns of storage slot t, read in place; reset
         mask, saved slot and ping-pong as `_MemoryFront`'s step]
     -> [lt_rnn_encoder_forward: [head columns of slot t | encoder of the new h] for the actor and the critic, one launch]
     -> [policy + value on those rows] -> [env step]
    four launches on the one stream, and the cell's `finish` behind the last step.  LSTM and GRU memories are both served by the key
    alone.  The state handling (adopting the modules' tensors, the saved slots, `finish`) is `_MemoryFront`'s; the storage keeps the raw
    rows, `compute_returns` stays the eager `evaluate` on the state `finish` left."""
    launches = 2  # both memories in one launch, both encoders in one launch

    def __init__(self, fr, *_):
        from .encoder import RnnEncoderPair

        super().__init__(fr, None, None, True)
        st, n = self.alg.storage, self.env.num_envs
        if fr.actor_mlp is None:
            raise ValueError("fused_rnn_encoder_policy: the env has no 12 actions: the policy launch samples 12")
        self.encoders = RnnEncoderPair(self.alg.actor_critic, st.observations.shape[-1], st.privileged_observations.shape[-1])
        self._strided_step = "lt_memory_gru_step_strided" if self.cell.nn is torch.nn.GRU else "lt_memory_step_strided"
        rows = n + (-n) % 64  # (the MLP launch reads whole row tiles)
        self._enc_rows = (torch.zeros(rows, self.encoders.a_width, device=self.device), torch.zeros(rows, self.encoders.c_width, device=self.device))

    def _memory_step(self, t: int, obs, cobs) -> None:
        """Step t of both memories in one launch, each on the last `input_size` columns of its rows."""
        ac, st = self.alg.actor_critic, self.alg.storage
        src = self._state if t == 0 else self._hc[(t - 1) & 1]
        dst = self._hc[t & 1]
        lstm = len(self.cell.state) == 2
        nets = []
        for k, (mem, x, saved) in enumerate(((ac.memory_a, obs, st.saved_hidden_states_a), (ac.memory_c, cobs, st.saved_hidden_states_c))):
            rnn, m = mem.rnn, _abi.LtRnnEncoderMemory()
            if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or x.shape[1] < rnn.input_size:
                raise ValueError("the memory step reads f32 rows with unit column stride that hold the memory's input columns")
            m.x, m.x_stride, m.I = x.data_ptr() + 4 * (x.shape[1] - rnn.input_size), x.stride(0), rnn.input_size
            m.w_ih, m.w_hh, m.b_ih, m.b_hh = (p.data_ptr() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0))
            m.h_in, m.h_out, m.saved_h = src[k][0].data_ptr(), dst[k][0].data_ptr(), saved[0][t].data_ptr()
            if lstm:
                m.c_in, m.c_out, m.saved_c = src[k][1].data_ptr(), dst[k][1].data_ptr(), saved[1][t].data_ptr()
            nets.append(m)
        _abi.call(self._strided_step, nets[0], nets[1], st.dones[t - 1] if t > 0 else None, self.env.num_envs, ac.memory_a.rnn.hidden_size,
                  _abi.stream(self.device))

    def rows(self, t: int, obs, cobs, launch: bool = True):
        """Two launches: the memories on the slot's tail columns, then the rows the two stacks read."""
        if launch:
            self._memory_step(t, obs, cobs)
            h_a, h_c = self._memory_rows(t)
            self.encoders.forward(obs, cobs, h_a, h_c, *self._enc_rows)
        n = self.env.num_envs
        return self._enc_rows[0][:n], self._enc_rows[1][:n]


class FusedRollout:
    """Drives a LocoTouchVecEnv and a PPO instance through rollout steps without leaving the device (module docstring).

    The env writes observation rows straight into the storage slots (slot t+1 from slot t; the last step writes the arena
    rows), so nothing copies observations."""

    def __init__(self, env, alg, use_packed_mlp: bool = True, obs_normalizer=None, critic_obs_normalizer=None,
                 fused_gru_memories: bool = False, fused_encoder_policy: bool = False, fused_rnn_encoder_policy: bool = False):
        from ..env import LocoTouchVecEnv

        served = (alg, obs_normalizer, critic_obs_normalizer, fused_gru_memories, fused_encoder_policy, use_packed_mlp, fused_rnn_encoder_policy)
        keyed = fused_encoder_policy or fused_rnn_encoder_policy  # (an encoder key: its own check is the whole statement of support)
        if keyed and (why := rollout_unsupported(*served)) is not None:  # (first: refused by name, whatever else is wrong)
            raise ValueError(why)
        if not isinstance(env, LocoTouchVecEnv):
            raise TypeError("FusedRollout drives a LocoTouchVecEnv (HIP env)")
        ac = alg.actor_critic
        # noise_std_type="log": the policy launches read sigma from a buffer of this object, refreshed from `log_std` by one
        # `lt_std_from_log` launch at the head of every rollout (inside a captured region: a replay sees the last update's log_std)
        self._std_buf = torch.zeros(12, device=env.device) if getattr(ac, "noise_std_type", "scalar") == "log" else None
        if self._std_buf is not None and ac.log_std.shape != (12,):
            raise ValueError("FusedRollout: log_std must hold the env's 12 actions")
        if not keyed and (why := rollout_unsupported(*served, kind_only=True)) is not None:
            raise ValueError(why)
        self.env, self.alg = env, alg
        self.device = env.device
        self.actions = torch.zeros(env.num_envs, 12, device=self.device)
        # Philox key of the policy noise: the kernels key the draws by the LOCAL row index, so rank r (env_index_offset = r * N) gets its
        # own key - with the population's seed alone every rank would explore with the same noise on its env i (offset 0: the seed itself)
        self._noise_seed = (int(env.cfg.seed) + 0x9E3779B97F4A7C15 * int(env.cfg.env_index_offset)) & 0xFFFFFFFFFFFFFFFF
        self.side = torch.cuda.Stream(device=self.device)
        # policy-noise RNG key: a copy of the env's common step counter (refreshed at every rollout start, advanced by
        # lt_rollout_record) so that lt_rollout_act never has to wait for the overlapped post kernel
        self._act_counter = env.counters[:1].clone()
        # rows written in place into the storage need whole 16-env wave tiles (npad == n)
        self.rows_in_storage = env.num_envs % 16 == 0
        # single-launch MLPs (lt_mlp.hip) when the stacks fit its shape limits, else the torch modules
        self.actor_mlp = self.critic_mlp = None
        if use_packed_mlp:
            from .mlp import PackedMLP, describe

            if describe(ac.actor) is not None and describe(ac.critic) is not None and env.num_actions == 12:
                self.actor_mlp, self.critic_mlp = PackedMLP(ac.actor), PackedMLP(ac.critic)
        # bf16 observation rows (BASELINE config 5): the storage slots hold bf16 rows; the env kernel reads slot t and writes slot
        # t + 1 as bf16 (the newest frame rounded once, older frames carried bit for bit), the policy kernel widens them in LDS.
        # The rows behind the LAST step go to two extra bf16 buffers and from there to the arena's f32 rows (exact).
        self.obs_dtype = alg.storage.observations.dtype
        self._tail_rows = None
        if self.obs_dtype == torch.bfloat16:
            if self.actor_mlp is None or not self.rows_in_storage:
                raise ValueError("bf16 observation rows need the packed MLP path and num_envs % 16 == 0")
            self.actor_mlp.set_input_format(torch.bfloat16)
            self.critic_mlp.set_input_format(torch.bfloat16)
            st = alg.storage
            self._tail_rows = (torch.zeros_like(st.observations[0]), torch.zeros_like(st.privileged_observations[0]))
        if not keyed and (why := rollout_unsupported(*served)) is not None:  # (the normalisers' own: behind the bf16 check, as ever)
            raise ValueError(why)
        self.recurrent = bool(getattr(ac, "is_recurrent", False))
        kind = _EncoderFront if fused_encoder_policy else _RnnEncoderFront if fused_rnn_encoder_policy else _MemoryFront if self.recurrent else _NormalizerFront if obs_normalizer is not None else _Front
        front = self.front = kind(self, obs_normalizer, critic_obs_normalizer, fused_gru_memories)
        self.gru = front.cell is not None and front.cell.nn is torch.nn.GRU

    def __getattr__(self, name: str):
        """What the front owns is read under its own name here: `begin()` (the start of a `learn()` call), `normalize_storage()`,
        `last_critic_obs`, `snapshots(which)`, `cell`, `encoders`, `normalizers`, `norm_rows`, and its private state."""
        return getattr(self.__dict__["front"], name) if "front" in self.__dict__ else object.__getattribute__(self, name)

    def step(self, t: int, last: bool) -> None:
        if self.actor_mlp is not None:
            self._step_packed(t, last)
        else:
            self._step_torch(t, last)
        self.alg.storage.step = t + 1
        if getattr(self.env, "telemetry", None) is not None:  # telemetry.Telemetry: one record launch on this stream, before the frame that charts it
            self.env.telemetry.record()
        if getattr(self.env, "episode_stats", None) is not None:  # episode_stats.EpisodeStats: one launch over all envs on this stream
            self.env.episode_stats.step()
        if self.env.recorder is not None:  # video.VideoRecorder: a render launch on this stream, between two step launches
            self.env.recorder.after_step()

    def _rows(self, t: int, last: bool):
        """(obs, critic obs, their pointers when they are storage slots, next obs ptr, next critic obs ptr) of step t."""
        env, st = self.env, self.alg.storage
        if not self.rows_in_storage:
            return env.obs_policy, env.obs_critic, 0, 0, 0, 0
        if last and self._tail_rows is not None:
            nxt = (self._tail_rows[0].data_ptr(), self._tail_rows[1].data_ptr())
        else:
            nxt = (0, 0) if last else (st.observations[t + 1].data_ptr(), st.privileged_observations[t + 1].data_ptr())
        obs, cobs = st.observations[t], st.privileged_observations[t]
        return obs, cobs, obs.data_ptr(), cobs.data_ptr(), nxt[0], nxt[1]

    @property
    def launches_per_step(self) -> int:
        """Kernel launches of one rollout step (the reference-shaped eager loop needs ~30)."""
        base = 2 if self.actor_mlp is not None else 11  # policy + value, env step (the population pass rides in the next step's launch)
        return base + self.front.launches

    def policy_value_launch(self, t: int) -> None:
        """The MLP launch of step t alone (bench.py times it for the MFMA roofline entry), on the rows the front has at hand: the slot's
        for the plain policy, else the rows its launches left - valid for the step that ran last (memory, encoder: no later step has
        overwritten its buffers).  NOT valid for that step with a normaliser front: its rows are by then those of the slot BEHIND it."""
        obs, cobs = self._rows(t, True)[:2]  # (last: no slot behind t is asked for, so t may be the storage's last one)
        self._policy_value(t, *self.front.rows(t, obs, cobs, launch=False))

    def _sigma(self) -> torch.Tensor:
        """The state-independent sigma the policy launches read: the `std` parameter, or the buffer `rollout()` refreshed from `log_std`."""
        return self.alg.actor_critic.std.data if self._std_buf is None else self._std_buf

    def _policy_value(self, t: int, obs, cobs) -> None:
        st = self.alg.storage
        _abi.call("lt_rollout_policy_value", self.actor_mlp.desc, self.actor_mlp.packed, obs, self.critic_mlp.desc, self.critic_mlp.packed,
                  cobs, st.values[t], self.env.num_envs, self._noise_seed, self._act_counter, t, self._sigma(),
                  st.actions[t], st.mu[t], st.sigma[t], st.actions_log_prob[t], self.actions, _abi.stream(self.device))

    def _step_packed(self, t: int, last: bool) -> None:
        """Launches on ONE stream (a linear graph: cross-queue edges of a forked graph cost more than they return on this stack):
        [what the front puts first] -> [actor + critic MLPs + sampling] -> [env step + storage record (+ the previous step's population
        pass on an idle wave)] -> [what the front puts behind]."""
        env, alg, st = self.env, self.alg, self.alg.storage
        obs, cobs, prev_p, prev_c, nxt_p, nxt_c = self._rows(t, last)
        if not self.rows_in_storage:
            st.observations[t].copy_(obs)
            st.privileged_observations[t].copy_(cobs)
        self._policy_value(t, *self.front.rows(t, obs, cobs))
        env.step_rollout_raw(self.actions.data_ptr(), prev_p, prev_c, nxt_p, nxt_c, st.values[t].data_ptr(), float(alg.gamma),
                             st.rewards[t].data_ptr(), st.dones[t].data_ptr())
        self.front.after_env_step(t, last)

    def _step_torch(self, t: int, last: bool) -> None:
        """torch modules for the networks (shapes outside lt_mlp's limits): GEMMs -> lt_rollout_act -> env step -> record,
        critic and post pass on forked streams."""
        env, alg, st = self.env, self.alg, self.alg.storage
        ac = alg.actor_critic
        main = torch.cuda.current_stream(self.device)
        stream = _abi.stream(self.device)
        n = env.num_envs
        obs, cobs, prev_p, prev_c, nxt_p, nxt_c = self._rows(t, last)
        seen, cseen = self.front.rows(t, obs, cobs)  # what the networks read
        mu = ac.actor(seen)
        rows = (None, None, None, None) if self.rows_in_storage else (obs, cobs, st.observations[t], st.privileged_observations[t])
        _abi.call("lt_rollout_act", n, env.num_obs, self._noise_seed, self._act_counter, mu, self._sigma(), None, *rows,
                  st.actions[t], st.mu[t], st.sigma[t], None, st.actions_log_prob[t], self.actions, stream)
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            value = ac.critic(cseen)
        env.step_rows_raw(self.actions.data_ptr(), prev_p, prev_c, nxt_p, nxt_c)
        main.wait_stream(self.side)
        value.record_stream(main)
        _abi.call("lt_rollout_record", n, float(alg.gamma), env.reward_buf, env.dones_buf, env.time_out_buf, value,
                  st.rewards[t], st.dones[t], st.values[t], self._act_counter, stream)
        self.front.after_env_step(t, last)

    def rollout(self, num_steps: int) -> None:
        """`num_steps` consecutive steps into storage slots 0.. (inference mode, capturable)."""
        env, st, front = self.env, self.alg.storage, self.front
        front.ready()
        st.clear()
        with torch.inference_mode():
            self._act_counter.copy_(env.counters[:1])
            if self._std_buf is not None:  # sigma = exp(log_std) as the optimizer left it: one launch per rollout (include/lt_ppo_opts.h)
                log_std = self.alg.actor_critic.log_std.data
                _abi.call("lt_std_from_log", log_std, log_std.numel(), self._std_buf, _abi.stream(self.device))
            front.open()
            if self.actor_mlp is not None:  # the optimizer has stepped since the last rollout
                self.actor_mlp.pack()
                self.critic_mlp.pack()
            if self.rows_in_storage:
                st.observations[0].copy_(env.obs_policy)
                st.privileged_observations[0].copy_(env.obs_critic)
            # chained steps (lt_env_defer_gate mode 2): the one-wave population pass of step t runs inside the launch of step t + 1,
            # beside its physics, so a rollout step is two launches; the pass of the last step closes the chain
            chain = not env.tactile  # (the tactile kernel keys its draws by the step counter, which lags inside a chain)
            if chain:
                env.defer_gate(2)
            if self._tail_rows is not None:
                env.set_row_format(torch.bfloat16)
            try:
                for t in range(num_steps):
                    self.step(t, last=t == num_steps - 1)
                front.finish(num_steps)
            finally:
                if chain:
                    env.gate_update()
                    env.defer_gate(0)
                front.close(num_steps)
                if self._tail_rows is not None:
                    env.set_row_format(torch.float32)
                    env.obs_policy.copy_(self._tail_rows[0])
                    env.obs_critic.copy_(self._tail_rows[1])
