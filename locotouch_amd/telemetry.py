"""Per-step telemetry of chosen envs, kept on the device (include/lt_telemetry.h, csrc/lt_telemetry.hip).

A `Telemetry` copies chosen stored scalars of chosen envs into a device ring with ONE small launch per env step - no host read, so it
runs inside a captured rollout - and is read out once, at the end:

    tel = Telemetry(env, {"vx": "cmd.vx", "torque": "applied_torque.FR_calf", "a0": (actions, 0)}, env_ids=(0, 3))
    env.telemetry = tel          # env.step and the fused rollout call tel.record() behind every step, before the video recorder
    ...
    data = tel.read()            # float32 [T, E, C], oldest record first; one host sync
    tel.save("run/telemetry/play.npz")

A channel is a key of `env.telemetry_channels()` or `(tensor, index)` for a caller's device tensor [N, ...] (float32, int32, int64 or
uint8).  The scripts' flags (`add_telemetry_args`, `telemetry_for`, `save_for`) are here too; the strip charts of `--video_telemetry`
are render.TelemetryChart / LocoTouchVecEnv.draw_telemetry_chart.  There is no CPU path: a CPU env or tensor raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _abi

T = _abi.TELEMETRY_CONSTS
_DTYPE_CODES = {torch.float32: 0, torch.int64: 1, torch.uint8: 2, torch.int32: 3}  # lt_view's codes
DEFAULT_CHANNELS = ("cmd", "joint_pos", "applied_torque", "foot_force", "obj_pos", "reward", "dones")
CHART_CHANNELS = ("cmd", "foot_force", "reward")  # what render.default_chart plots


def resolve_names(known, names) -> list[str]:
    """Channel names of `names`: each a key of `known` or a group (the part of the keys before the first "."), in `known`'s order inside
    a group and without repeats.  ValueError with the known names for any other."""
    known, out = list(known), []
    for name in names:
        hit = [name] if name in known else [k for k in known if k.split(".", 1)[0] == name]
        if not hit:
            groups = sorted({k.split(".", 1)[0] for k in known})
            raise ValueError(f"unknown telemetry channel {name!r}; known groups: {', '.join(groups)}; known channels: {', '.join(known)}")
        out += [k for k in hit if k not in out]
    return out


class Telemetry:
    def __init__(self, env, channels, env_ids=(0,), capacity: int = 4096):
        """`channels`: an ordered mapping name -> spec; a spec is a key of `env.telemetry_channels()` or `(tensor, index)`: element
        `index` (an int or a tuple, into the dimensions behind the first) of every row of a caller's device tensor [N, ...]."""
        self.env, self.device = env, torch.device(env.device)
        if self.device.type != "cuda":
            raise RuntimeError("Telemetry needs a HIP device (the ring is written by a HIP kernel; there is no CPU path)")
        if not channels:
            raise ValueError("Telemetry needs at least one channel")
        self.names = list(channels)
        self.env_ids = [int(e) for e in (env_ids.tolist() if hasattr(env_ids, "tolist") else env_ids)]
        self.capacity = int(capacity)
        self.step_dt = float(getattr(env, "step_dt", 0.0))
        own = None
        table = (_abi.LtTelemetryChannel * len(self.names))()
        self._sources = []  # the tensors the plan points into stay alive with it
        for row, (name, spec) in zip(table, channels.items()):
            if isinstance(spec, str):
                own = env.telemetry_channels() if own is None else own
                if spec not in own:
                    resolve_names(own, [spec])  # raises, with the known names
                tensor, offset = own[spec]
            else:
                tensor, offset = self._caller_tensor(name, *spec)
            if self.env_ids and (min(self.env_ids) < 0 or max(self.env_ids) >= tensor.shape[0]):
                raise ValueError(f"Telemetry: channel {name!r} holds {tensor.shape[0]} envs; env ids {self.env_ids} do not all lie below that")
            row.base, row.dtype, row.env_stride, row.offset = tensor.data_ptr(), _DTYPE_CODES[tensor.dtype], tensor.stride(0), int(offset)
            self._sources.append(tensor)
        ids = (ctypes.c_int32 * max(1, len(self.env_ids)))(*self.env_ids)
        nbytes = ctypes.c_size_t()
        _abi.call("lt_telemetry_plan_bytes", len(self.names), len(self.env_ids), ctypes.byref(nbytes))
        if not 1 <= self.capacity <= T["LT_TELEMETRY_MAX_CAPACITY"]:
            raise ValueError(f"Telemetry: capacity must be in 1 ... {T['LT_TELEMETRY_MAX_CAPACITY']}, got {self.capacity}")
        with torch.cuda.device(self.device):
            self.plan = torch.zeros(nbytes.value, dtype=torch.uint8, device=self.device)  # (torch's allocations are 256-byte aligned)
            self.ring = torch.zeros(self.capacity, len(self.env_ids), len(self.names), dtype=torch.float32, device=self.device)
            self.head = torch.zeros(2, dtype=torch.int64, device=self.device)
            _abi.call("lt_telemetry_plan", table, len(self.names), ids, len(self.env_ids), self.capacity, self.plan, nbytes.value,
                      _abi.stream(self.device))

    def _caller_tensor(self, name, tensor, index=()):
        if not isinstance(tensor, torch.Tensor) or tensor.dtype not in _DTYPE_CODES:
            kind = tensor.dtype if isinstance(tensor, torch.Tensor) else type(tensor).__name__
            raise TypeError(f"Telemetry: channel {name!r} is {kind}; float32, int32, int64 and uint8 device tensors are served")
        if tensor.device != self.device:
            raise TypeError(f"Telemetry: channel {name!r} lives on {tensor.device}, the env on {self.device}")
        index = (int(index),) if not isinstance(index, (tuple, list)) else tuple(int(i) for i in index)
        if tensor.dim() < 1 or len(index) != tensor.dim() - 1 or any(not 0 <= i < n for i, n in zip(index, tensor.shape[1:])):
            raise ValueError(f"Telemetry: channel {name!r}: index {index} does not name one element of a row of shape {tuple(tensor.shape[1:])}")
        if any(s < 0 for s in tensor.stride()):
            raise ValueError(f"Telemetry: channel {name!r} has a negative stride")
        return tensor, sum(i * s for i, s in zip(index, tensor.stride()[1:]))

    def record(self) -> None:
        """One launch on the env's current stream: the channels as they stand now go into the next slot of the ring."""
        with torch.cuda.device(self.device):
            _abi.call("lt_telemetry_record", self.plan, self.ring, self.head, _abi.stream(self.device))

    @property
    def count(self) -> int:
        """Records written so far (a host read: waits for the stream)."""
        return int(self.head[0])

    def reset(self) -> None:
        self.head.zero_()
        self.ring.zero_()

    def read(self) -> torch.Tensor:
        """float32 [T, E, C] on the device, oldest record first, T = min(count, capacity).  One host sync."""
        count = self.count
        if count <= self.capacity:
            return self.ring[:count].clone()
        return torch.roll(self.ring, -(count % self.capacity), dims=0)

    def save(self, path: str) -> str:
        """`.npz`: data [T, E, C], names [C], env_ids [E], step_dt, first_step (the record index of data[0]) and dropped (records the
        wrap overwrote: the same number)."""
        count = self.count
        data = self.read().cpu().numpy()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        dropped = count - data.shape[0]
        np.savez(path, data=data, names=np.array(self.names), env_ids=np.array(self.env_ids, dtype=np.int64), step_dt=np.float64(self.step_dt),
                 first_step=np.int64(dropped), dropped=np.int64(dropped))
        return path

    def slot_of(self, env_id: int) -> int:
        """The index of `env_id` in the env list: what a chart calls the slot."""
        try:
            return self.env_ids.index(int(env_id))
        except ValueError:
            raise ValueError(f"env {env_id} is not recorded by this Telemetry (its envs: {self.env_ids})") from None


# ---- the scripts' flags --------------------------------------------------------------------------------------------------
def add_telemetry_args(ap) -> None:
    """--telemetry, --telemetry_envs, --telemetry_channels (`--video_telemetry` is video.add_video_args')."""
    ap.add_argument("--telemetry", action="store_true",
                    help="record chosen scalars of chosen envs behind every env step into a device ring (include/lt_telemetry.h) and write "
                         "<run>/telemetry/<play|train>.npz at exit")
    ap.add_argument("--telemetry_envs", default="0", help="comma-separated env ids to record (at most 32)")
    ap.add_argument("--telemetry_channels", default=",".join(DEFAULT_CHANNELS),
                    help="comma-separated channel names or groups of LocoTouchVecEnv.telemetry_channels() (at most 64 channels)")
    ap.add_argument("--telemetry_capacity", type=int, default=4096, help="records the ring holds; older ones are overwritten")


def telemetry_for(env, args, video_env: int = 0):
    """The Telemetry the script arguments ask for, attached as `env.telemetry`, or None without --telemetry and --video_telemetry.
    With --video_telemetry the channels of the default chart and the recorded env `video_env` are added where they are missing."""
    chart = bool(getattr(args, "video_telemetry", False))
    if not getattr(args, "telemetry", False) and not chart:
        return None
    names = [n for n in str(args.telemetry_channels).split(",") if n]
    env_ids = [int(e) for e in str(args.telemetry_envs).split(",") if e.strip()]
    if chart:
        names += [n for n in CHART_CHANNELS if n not in names]
        if video_env not in env_ids:
            env_ids.append(video_env)
    names = resolve_names(env.telemetry_channels(), names)
    tel = Telemetry(env, {n: n for n in names}, env_ids=env_ids, capacity=int(args.telemetry_capacity))
    env.telemetry = tel
    return tel


def save_for(tel, args, run_dir: str, mode: str):
    """Write <run_dir>/telemetry/<mode>.npz where --telemetry was given (a Telemetry that only feeds --video_telemetry is not saved)."""
    if tel is None or not getattr(args, "telemetry", False):
        return None
    path = tel.save(os.path.join(run_dir, "telemetry", mode + ".npz"))
    print(f"[Telemetry] wrote {path}")
    return path


__all__ = ["Telemetry", "resolve_names", "add_telemetry_args", "telemetry_for", "save_for", "DEFAULT_CHANNELS", "CHART_CHANNELS"]
