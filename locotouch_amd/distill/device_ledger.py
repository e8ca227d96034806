"""Opt-in device form of the trajectory bookkeeping of `ReplayBuffer.collect_data` / `evaluate`: the episode ledger behind the C ABI
(include/lt_ledger.h, csrc/lt_ledger.hip) - one HIP launch behind each env step instead of a blocking copy of `[check_every][N]` rewards
and dones and a replay of the rules in numpy.

`DeviceEpisodeLedger(device, num_envs, window)` owns the ledger's state and its lists (finished episodes: f64 reward, length; kept
trajectories: env, first step, end step) and is driven as

    begin(reward_sums, keep_target=None, episode_target=None)
    step(reward, done_mask)         behind every env step: one launch, nothing else
    head = poll()                   whenever the caller likes: a NON-BLOCKING look at the ledger's 64-byte head, one call late
    rewards, lengths, trajs = drain(head)
    end(reward_sums_out)

`poll()` issues an asynchronous copy of the head into pinned memory plus an event and returns the copy the PREVIOUS call issued (None on
the first call of a run), so a loop that polls every k steps learns of a stop between k and 2 k - 1 steps late and never drains the launch
queue; it waits only if the device has fallen a whole poll interval behind.  What the loop learns is exact: the ledger stops ITSELF on
the step the host rules would have stopped on, and every later `step` leaves it bit for bit.

The lists hold `window * num_envs` entries, so `window` steps can never overflow them.  `step` keeps count: before a launch that could
overflow by what the host knows (the last head it has seen plus one full done list per step issued since), it reads the lists away with
one blocking drain - with a loop that polls every `window // 4` steps this happens only when the lists are really more than half full.
An overflow the device reports all the same is an error, never a silent loss.
A non-CUDA device raises `ValueError`: there is no fall-back to the host rules.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import torch

from .. import _abi

_FIELDS = ("step", "kept_steps", "episodes", "trajs", "stopped_at", "overflow", "keep_target", "episode_target")
assert [_abi.LEDGER_CONSTS["LT_LEDGER_" + f.upper()] for f in _FIELDS] == list(range(_abi.LEDGER_CONSTS["LT_LEDGER_HEAD_FIELDS"]))
LedgerHead = namedtuple("LedgerHead", _FIELDS)


class DeviceEpisodeLedger:
    def __init__(self, device, num_envs: int, window: int):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceEpisodeLedger: the ledger runs in HIP kernels and needs a CUDA device, got {device!r} "
                             "(keep the books on the host there)")
        if int(num_envs) < 1 or int(window) < 1:
            raise ValueError("DeviceEpisodeLedger: num_envs and window must be at least 1")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs, self.window = int(num_envs), int(window)
        self.capacity = self.window * self.num_envs
        size = ctypes.c_size_t()
        _abi.call("lt_ledger_state_bytes", self.num_envs, ctypes.byref(size))
        assert size.value == 64 + 16 * self.num_envs
        self._state = torch.zeros(size.value // 8, dtype=torch.int64, device=self.device)  # head | reward_sum | start (lt_ledger.h)
        assert self._state.data_ptr() % 16 == 0
        self._ep_reward = torch.zeros(self.capacity, dtype=torch.float64, device=self.device)
        self._ep_length = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self._traj = torch.zeros(self.capacity, 3, dtype=torch.int64, device=self.device)
        self._pinned = [torch.zeros(8, dtype=torch.int64).pin_memory() for _ in range(2)]

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            _abi.call(name, *args, _abi.stream(self.device))

    def _check(self, name: str, x, dtypes) -> None:
        if (not isinstance(x, torch.Tensor) or x.dtype not in dtypes or x.device != self.device or x.shape != (self.num_envs,)
                or not x.is_contiguous()):
            raise TypeError(f"DeviceEpisodeLedger: {name} must be a contiguous [{self.num_envs}] tensor of "
                            f"{' or '.join(str(t) for t in dtypes)} on {self.device}")

    # ---- a run --------------------------------------------------------------------------------------------------------------
    def begin(self, reward_sums: torch.Tensor | None, keep_target: int | None = None, episode_target: int | None = None,
              with_trajs: bool = True) -> None:
        """Starts a run from the carried f32 reward sums (None: zeros).  `keep_target`: stop once the kept trajectories hold that many
        steps (collect_data); `episode_target`: stop once that many episodes have finished (evaluate); None: no such target.
        `with_trajs=False`: no trajectory list is kept (every finished env still starts a new trajectory)."""
        if reward_sums is not None:
            self._check("reward_sums", reward_sums, (torch.float32,))
        self._call("lt_ledger_begin", self._state, self.num_envs, reward_sums, -1 if keep_target is None else max(0, int(keep_target)),
                   -1 if episode_target is None else max(0, int(episode_target)))
        self._with_trajs = bool(with_trajs)
        self._ep_first = self._traj_first = 0          # entries read away so far: the number of the entry in slot 0 of each list
        self._issued = self._step_seen = self._fill_seen = 0
        self._pending, self._flip = None, 0
        self._spilled = ([], [], [])

    def step(self, reward: torch.Tensor, done_mask: torch.Tensor) -> None:
        """One env step's bookkeeping: one launch, no host read (but see the module text on a run that fills the lists)."""
        self._check("reward", reward, (torch.float32,))
        self._check("done_mask", done_mask, (torch.bool, torch.uint8))
        # what the lists can hold at most behind this launch, by the last head seen: a full done list per step issued since
        if self._fill_seen + (self._issued + 1 - self._step_seen) * self.num_envs > self.capacity:
            self._spill()
        traj = self._traj if self._with_trajs else None
        self._call("lt_ledger_step", self._state, self.num_envs, reward, done_mask, self._ep_reward, self._ep_length, self._ep_first,
                   self.capacity, traj, self._traj_first, self.capacity if self._with_trajs else 0)
        self._issued += 1

    def _seen(self, head: LedgerHead) -> LedgerHead:
        if head.overflow:
            raise RuntimeError(f"DeviceEpisodeLedger: {head.overflow} list entries did not fit into {self.capacity} slots "
                               f"(window {self.window} x {self.num_envs} envs)")
        if head.stopped_at:  # (every later step is ignored on the device: nothing more is appended)
            self._step_seen, self._fill_seen = self._issued, head.episodes - self._ep_first
        elif head.step >= self._step_seen:  # (a running ledger's step is the number of launches in front of the copy; an older head
            self._step_seen, self._fill_seen = head.step, head.episodes - self._ep_first  # than the last spill says nothing new)
        return head

    def poll(self) -> LedgerHead | None:
        """Issues an asynchronous copy of the head and returns the head the previous call's copy brought (None on a run's first call)."""
        prev = self._pending
        buf = self._pinned[self._flip]
        self._flip ^= 1
        with torch.cuda.device(self.device):
            buf.copy_(self._state[:8], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        self._pending = (buf, ev)
        if prev is None:
            return None
        prev[1].synchronize()  # (returns at once unless the device is a whole poll interval behind)
        return self._seen(LedgerHead(*prev[0].tolist()))

    def read_head(self) -> LedgerHead:
        """The head as it is behind everything issued so far: one BLOCKING 64-byte copy."""
        return self._seen(LedgerHead(*self._state[:8].tolist()))

    def _read_lists(self, head: LedgerHead):
        k, m = head.episodes - self._ep_first, (head.trajs - self._traj_first) if self._with_trajs else 0
        assert 0 <= k <= self.capacity and 0 <= m <= self.capacity
        if k == 0 and m == 0:
            return [], [], []
        # one packed copy: rewards (as their bits), lengths, triples
        packed = torch.cat([self._ep_reward[:k].view(torch.int64), self._ep_length[:k], self._traj[:m].reshape(-1)]).cpu()
        rewards = packed[:k].view(torch.float64).tolist()
        lengths = packed[k:2 * k].tolist()
        trajs = [tuple(t) for t in packed[2 * k:].view(m, 3).tolist()]
        self._ep_first, self._traj_first = head.episodes, head.trajs if self._with_trajs else 0
        self._fill_seen = 0
        return rewards, lengths, trajs

    def _spill(self) -> None:
        part = self._read_lists(self.read_head())  # (blocking: behind it the lists are empty and every issued step is accounted for)
        self._step_seen = self._issued
        for acc, new in zip(self._spilled, part):
            acc.extend(new)

    def drain(self, head: LedgerHead | None = None):
        """(rewards, lengths, trajs) appended since the last drain, in list order.  `head`: a head `poll()` returned whose ledger had
        stopped (it is final: no blocking head read is needed, the one blocking copy is that of the lists); None: the head is read
        behind everything issued so far."""
        if head is None or not head.stopped_at:
            head = self.read_head()
        part = self._read_lists(head)
        out = tuple(acc + new for acc, new in zip(self._spilled, part))
        self._spilled = ([], [], [])
        return out

    def end(self, reward_sums_out: torch.Tensor) -> None:
        """`reward_sums_out` (f32 [num_envs]) receives the f32 roundings of the ledger's f64 sums: what the next run carries on from."""
        self._check("reward_sums_out", reward_sums_out, (torch.float32,))
        self._call("lt_ledger_end", self._state, self.num_envs, reward_sums_out)
