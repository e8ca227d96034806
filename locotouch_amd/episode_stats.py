"""Statistics over the finished episodes of ALL envs, kept on the device (include/lt_episode_stats.h, csrc/lt_episode_stats.hip).

An `EpisodeStats` accumulates chosen per-step terms of every env with ONE launch per env step - no host read, so it runs inside a
captured rollout - folds every finished episode into per-env float64 accumulators, and is read once:

    stats = EpisodeStats(env)            # default_metrics(env); or metrics=[Metric("power", [...], "abs_product", "mean"), ...]
    env.episode_stats = stats            # env.step and the fused rollout call stats.step() behind every step
    stats.begin()
    ...
    table = stats.summary()              # {metric: {episodes, mean, std, min, max}, "termination": {name: share}}; one host sync
    stats.save("run/episode_stats/play.json")

A channel is a key of `env.episode_stats_channels()` or `(tensor, index)` for a caller's device tensor [N, ...] (float32, int32, int64
or uint8), exactly as `telemetry.Telemetry` takes them.  The scripts' flags (`add_episode_stats_args`, `episode_stats_for`, `report_for`)
are here too.  There is no CPU path: a CPU env or tensor raises.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi

E = _abi.EPISODE_STATS_CONSTS
_DTYPE_CODES = {torch.float32: 0, torch.int64: 1, torch.uint8: 2, torch.int32: 3}  # lt_view's codes
TERMS = {"value": E["LT_EPISODE_STATS_VALUE"], "abs": E["LT_EPISODE_STATS_ABS"], "square": E["LT_EPISODE_STATS_SQUARE"],
         "diff_square": E["LT_EPISODE_STATS_DIFF_SQUARE"], "abs_product": E["LT_EPISODE_STATS_ABS_PRODUCT"]}
REDUCES = {"mean": E["LT_EPISODE_STATS_MEAN"], "sum": E["LT_EPISODE_STATS_SUM"], "max": E["LT_EPISODE_STATS_MAX"],
           "last": E["LT_EPISODE_STATS_LAST"]}
FIELDS = E["LT_EPISODE_STATS_FIELDS"]
CAUSES = E["LT_EPISODE_STATS_CAUSES"]
LENGTH = "length"  # the built-in metric
# counter b < 16 of the causes is bit b of LT_F_TERM_BITS (enum lt_termination, then LT_T_USER and LT_T_USER_TIME_OUT); counter 16 is
# the time_out channel (bits 0 and 8 are its two sources), counter 17 the episodes
_USER_BITS = {_abi.CONSTS["LT_T_USER"]: "user", _abi.CONSTS["LT_T_USER_TIME_OUT"]: "user_time_out"}


@dataclass(frozen=True)
class Metric:
    """`pairs`: a list of channels or of (a, b) channel pairs; `term`: a key of TERMS; `reduce`: a key of REDUCES."""
    name: str
    pairs: tuple
    term: str = "value"
    reduce: str = "mean"
    sqrt: bool = False
    include_done_step: bool = False


def default_table(task_has_object: bool) -> list[Metric]:
    """The default table (README.md): return, velocity tracking, speed, power, torque, joint speed, foot force, root height and, on a
    task with an object, where the object is relative to the robot and how fast it moves over it.  Channel names only: no env is needed."""
    from .env import LEG_NAMES

    joints = [f"{leg}_{part}" for part in ("hip", "thigh", "calf") for leg in LEG_NAMES]
    out = [Metric("return", ("reward",), "value", "sum", include_done_step=True),
           Metric("error_vel_xy", ("cmd_metric.error_vel_xy",), "value", "last"),
           Metric("error_vel_yaw", ("cmd_metric.error_vel_yaw",), "value", "last"),
           Metric("speed_xy_rms", ("root_lin_vel_w.x", "root_lin_vel_w.y"), "square", "mean", sqrt=True),
           Metric("power_mean", tuple((f"applied_torque.{j}", f"joint_vel.{j}") for j in joints), "abs_product", "mean"),
           Metric("torque_rms", tuple(f"applied_torque.{j}" for j in joints), "square", "mean", sqrt=True),
           Metric("joint_vel_rms", tuple(f"joint_vel.{j}" for j in joints), "square", "mean", sqrt=True),
           Metric("total_foot_force_max", tuple(f"foot_force.{leg}" for leg in LEG_NAMES), "abs", "max"),
           Metric("root_height_mean", ("root_pos.z",), "value", "mean")]
    if task_has_object:
        out += [Metric("object_offset_xy_max", tuple((f"obj_pos.{a}", f"root_pos.{a}") for a in "xy"), "diff_square", "max", sqrt=True),
                Metric("object_speed_rel_rms", tuple((f"obj_lin_vel_w.{a}", f"root_lin_vel_w.{a}") for a in "xyz"), "diff_square", "mean", sqrt=True)]
    return out


def default_metrics(env) -> list[Metric]:
    return default_table(int(env.cfg.task) != _abi.CONSTS["LT_TASK_LOCOMOTION"])


def default_metric_names(task_has_object: bool = True) -> list[str]:
    """The names of the default table, the built-in length behind the return."""
    names = [m.name for m in default_table(task_has_object)]
    return names[:1] + [LENGTH] + names[1:]


def chosen_metrics(table, asked: str | None) -> list[Metric]:
    """The metrics of `table` that the comma-separated `asked` names (None or empty: all of them).  ValueError with the known names for
    an unknown one, and for a choice of the length alone: it is built in and always reported, but a plan holds at least one metric."""
    names = [n for n in str(asked or "").split(",") if n]
    if not names:
        return list(table)
    names = resolve_metric_names([m.name for m in table[:1]] + [LENGTH] + [m.name for m in table[1:]], names)
    chosen = [m for m in table if m.name in names]
    if not chosen:
        raise ValueError(f"--episode_stats_metrics: {LENGTH!r} is built in and always reported; name at least one metric beside it")
    return chosen


def resolve_metric_names(known, names) -> list[str]:
    """`names` without repeats; ValueError with the known ones for any other."""
    known, out = list(known), []
    for name in names:
        if name not in known:
            raise ValueError(f"unknown episode-statistics metric {name!r}; known metrics: {', '.join(known)}")
        if name not in out:
            out.append(name)
    return out


class EpisodeStats:
    def __init__(self, env, metrics=None, skip_running: bool = True):
        self.env, self.device = env, torch.device(env.device)
        if self.device.type != "cuda":
            raise RuntimeError("EpisodeStats needs a HIP device (the statistics are kept by HIP kernels; there is no CPU path)")
        self.metrics = list(default_metrics(env) if metrics is None else metrics)
        self.skip_running = bool(skip_running)
        self.num_envs = int(env.num_envs)
        self.names = [m.name for m in self.metrics]
        if len(set(self.names)) != len(self.names) or LENGTH in self.names:
            raise ValueError(f"EpisodeStats: metric names must differ from each other and from the built-in {LENGTH!r}, got {self.names}")
        if not 1 <= len(self.metrics) <= E["LT_EPISODE_STATS_MAX_METRICS"]:
            raise ValueError(f"EpisodeStats: 1 ... {E['LT_EPISODE_STATS_MAX_METRICS']} metrics, got {len(self.metrics)}")
        self._known = None
        self._sources = []  # the tensors the plan points into stay alive with it
        table = (_abi.LtEpisodeStatsMetric * len(self.metrics))()
        for row, m in zip(table, self.metrics):
            if m.term not in TERMS or m.reduce not in REDUCES:
                raise ValueError(f"EpisodeStats: metric {m.name!r}: term is one of {', '.join(TERMS)}, reduce one of {', '.join(REDUCES)}; "
                                 f"got {m.term!r}, {m.reduce!r}")
            if not 1 <= len(m.pairs) <= E["LT_EPISODE_STATS_MAX_PAIRS"]:
                raise ValueError(f"EpisodeStats: metric {m.name!r}: 1 ... {E['LT_EPISODE_STATS_MAX_PAIRS']} channel pairs, got {len(m.pairs)}")
            two = m.term in ("diff_square", "abs_product")
            row.npairs, row.term, row.reduce = len(m.pairs), TERMS[m.term], REDUCES[m.reduce]
            row.take_sqrt, row.include_done_step = int(bool(m.sqrt)), int(bool(m.include_done_step))
            for slot, pair in zip(row.pairs, m.pairs):
                a, b = pair if two else (pair, None)
                if two and b is None:
                    raise ValueError(f"EpisodeStats: metric {m.name!r}: {m.term} reads a second channel of every pair")
                self._fill(slot.a, m.name, a)
                if b is not None:
                    self._fill(slot.b, m.name, b)
        named = (_abi.LtTelemetryChannel * 3)()
        for row, name in zip(named, ("dones", "time_out", "term_bits")):
            self._fill(row, name, name)
        sizes = {}
        for what, args in (("plan", (len(self.metrics),)), ("state", (len(self.metrics), self.num_envs)), ("result", (len(self.metrics),))):
            nbytes = ctypes.c_size_t()
            _abi.call(f"lt_episode_stats_{what}_bytes", *args, ctypes.byref(nbytes))
            sizes[what] = nbytes.value
        with torch.cuda.device(self.device):
            self.plan = torch.zeros(sizes["plan"], dtype=torch.uint8, device=self.device)  # (torch's allocations are 256-byte aligned)
            self.state = torch.zeros(sizes["state"], dtype=torch.uint8, device=self.device)
            self.result = torch.zeros(sizes["result"], dtype=torch.uint8, device=self.device)
            _abi.call("lt_episode_stats_plan_write", table, len(self.metrics), ctypes.byref(named[0]), ctypes.byref(named[1]), ctypes.byref(named[2]),
                      self.num_envs, self.plan, sizes["plan"], _abi.stream(self.device))
        self.begin()

    def _fill(self, row, metric, spec) -> None:
        if isinstance(spec, str):
            if self._known is None:
                self._known = self.env.episode_stats_channels()
            if spec not in self._known:
                raise ValueError(f"EpisodeStats: metric {metric!r}: unknown channel {spec!r}; known channels: {', '.join(self._known)}")
            tensor, offset = self._known[spec]
        else:
            tensor, offset = self._caller_tensor(metric, *spec)
        if tensor.shape[0] < self.num_envs:
            raise ValueError(f"EpisodeStats: metric {metric!r}: a channel holds {tensor.shape[0]} envs, the env {self.num_envs}")
        row.base, row.dtype, row.env_stride, row.offset = tensor.data_ptr(), _DTYPE_CODES[tensor.dtype], tensor.stride(0), int(offset)
        self._sources.append(tensor)

    def _caller_tensor(self, name, tensor, index=()):
        if not isinstance(tensor, torch.Tensor) or tensor.dtype not in _DTYPE_CODES:
            kind = tensor.dtype if isinstance(tensor, torch.Tensor) else type(tensor).__name__
            raise TypeError(f"EpisodeStats: metric {name!r}: a channel is {kind}; float32, int32, int64 and uint8 device tensors are served")
        if tensor.device != self.device:
            raise TypeError(f"EpisodeStats: metric {name!r}: a channel lives on {tensor.device}, the env on {self.device}")
        index = (int(index),) if not isinstance(index, (tuple, list)) else tuple(int(i) for i in index)
        if tensor.dim() < 1 or len(index) != tensor.dim() - 1 or any(not 0 <= i < n for i, n in zip(index, tensor.shape[1:])):
            raise ValueError(f"EpisodeStats: metric {name!r}: index {index} does not name one element of a row of shape {tuple(tensor.shape[1:])}")
        if any(s < 0 for s in tensor.stride()):
            raise ValueError(f"EpisodeStats: metric {name!r}: a channel has a negative stride")
        return tensor, sum(i * s for i, s in zip(index, tensor.stride()[1:]))

    # ---- the launches ----
    def begin(self) -> None:
        """Zero the state and arm every env (skip_running off) or none: one launch on the current stream."""
        with torch.cuda.device(self.device):
            _abi.call("lt_episode_stats_begin", self.state, len(self.metrics), self.num_envs, int(self.skip_running), _abi.stream(self.device))

    def step(self) -> None:
        """One launch on the current stream: the channels as they stand now, behind an env step."""
        with torch.cuda.device(self.device):
            _abi.call("lt_episode_stats_step", self.plan, self.state, len(self.metrics), self.num_envs, _abi.stream(self.device))

    def restart_running(self) -> None:
        """Drop the running episodes (run, count, steps; arming as `begin` leaves it) and keep what has finished: one launch.  `env.reset()`
        calls it: a reset of all envs sets no `dones`, and the episodes it cuts off must not run on into the ones that start."""
        with torch.cuda.device(self.device):
            _abi.call("lt_episode_stats_restart_running", self.state, len(self.metrics), self.num_envs, int(self.skip_running), _abi.stream(self.device))

    def clear_finished(self) -> None:
        with torch.cuda.device(self.device):
            _abi.call("lt_episode_stats_clear_finished", self.state, len(self.metrics), self.num_envs, _abi.stream(self.device))

    def totals(self, clear: bool = False):
        """(float64 [M + 1][5], int64 [18]) on the host: the reduce launch and ONE sync read of the result block."""
        with torch.cuda.device(self.device):
            _abi.call("lt_episode_stats_reduce", self.state, len(self.metrics), self.num_envs, self.result, _abi.stream(self.device))
            if clear:
                self.clear_finished()
        raw = self.result.cpu().numpy()
        cut = 8 * FIELDS * (len(self.metrics) + 1)
        return raw[:cut].view(np.float64).reshape(len(self.metrics) + 1, FIELDS).copy(), raw[cut:].view(np.int64).copy()

    def summary(self, clear: bool = False) -> dict:
        """{metric: {episodes, mean, std, min, max}} over the episodes finished since `begin` (or the last clear) plus "termination":
        {term name | "time_out": share of the episodes}.  A metric without an episode has episodes 0 and no numbers."""
        totals, causes = self.totals(clear)
        out = {}
        for name, (n, s, sq, lo, hi) in zip(self.names + [LENGTH], totals.tolist()):
            if n == 0:
                out[name] = {"episodes": 0}
                continue
            mean = s / n
            out[name] = {"episodes": int(n), "mean": mean, "std": math.sqrt(max(sq / n - mean * mean, 0.0)), "min": lo, "max": hi}
        episodes = int(causes[CAUSES - 1])
        out["termination"] = {name: (int(causes[c]) / episodes if episodes else 0.0) for c, name in self.cause_names().items()}
        return out

    def eval_record(self, clear: bool = True) -> dict:
        """`Eval/<metric>/mean` and `Eval/termination/<name>` of the episodes finished since the last clear, for a training record.
        A metric without an episode logs nothing; without any episode nothing is logged at all."""
        summary = self.summary(clear)
        rec = {f"Eval/{name}/mean": v["mean"] for name, v in summary.items() if name != "termination" and v["episodes"]}
        if summary[LENGTH]["episodes"]:
            rec.update({f"Eval/termination/{name}": share for name, share in summary["termination"].items()})
        return rec

    def cause_names(self) -> dict:
        """cause counter -> name: the enabled termination terms but the time-out, the user bits, and "time_out" (counter 16)."""
        from .env import TERMINATION_NAMES

        cfg = self.env.cfg
        names = {b: n for b, n in enumerate(TERMINATION_NAMES) if b != _abi.CONSTS["LT_T_TIME_OUT"] and cfg.term_enabled[b]}
        names.update(_USER_BITS)
        names[CAUSES - 2] = "time_out"
        return names

    def per_env(self) -> dict:
        """Views of the state (device; they change with the next step): finished float64 [M + 1, 5, N] (n, sum, sumsq, min, max; the
        last metric is the length), run float32 [M, N], count int32 [M, N], steps int32 [N], causes int32 [18, N], armed uint8 [N]."""
        m, n, out, at = len(self.metrics), self.num_envs, {}, 0
        for name, dtype, shape in (("finished", torch.float64, (m + 1, FIELDS, n)), ("run", torch.float32, (m, n)), ("count", torch.int32, (m, n)),
                                   ("steps", torch.int32, (n,)), ("causes", torch.int32, (CAUSES, n)), ("armed", torch.uint8, (n,))):
            nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
            out[name] = self.state[at:at + nbytes].view(dtype).reshape(shape)
            at += nbytes
        return out

    def save(self, path: str, summary: dict | None = None) -> str:
        """JSON: the summary, the metrics' definitions, the env count and whether running episodes were skipped."""
        doc = {"num_envs": self.num_envs, "skip_running": self.skip_running, "summary": self.summary() if summary is None else summary,
               "metrics": {m.name: {"term": m.term, "reduce": m.reduce, "sqrt": bool(m.sqrt), "include_done_step": bool(m.include_done_step),
                                    "pairs": [p if isinstance(p, str) else [c if isinstance(c, str) else "<tensor>" for c in p] for p in m.pairs]}
                           for m in self.metrics}}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
        return path


def format_table(summary: dict) -> str:
    rows = [f"{'metric':<24}{'episodes':>9}{'mean':>13}{'std':>13}{'min':>13}{'max':>13}"]
    for name, v in summary.items():
        if name == "termination":
            continue
        rows.append(f"{name:<24}{v['episodes']:>9}" + ("".join(f"{v[k]:>13.5g}" for k in ("mean", "std", "min", "max")) if v["episodes"] else ""))
    rows.append("termination: " + ", ".join(f"{k}={v:.3f}" for k, v in summary.get("termination", {}).items()))
    return "\n".join(rows)


# ---- the scripts' flags --------------------------------------------------------------------------------------------------
def add_episode_stats_args(ap) -> None:
    ap.add_argument("--episode_stats", action="store_true",
                    help="keep statistics over the finished episodes of all envs on the device (include/lt_episode_stats.h); play and distill "
                         "print a table and write <run>/episode_stats/<play|train>.json at exit, train logs Eval/<metric>/mean per iteration")
    ap.add_argument("--episode_stats_metrics", default=None, help="comma-separated names among the default metrics (default: all of them)")


def refuse_episode_stats_metrics(args) -> None:
    """ValueError naming an unknown metric of --episode_stats_metrics - unknown for the task of `args.task`: a task without an object has
    no object metrics - before anything is built (host only: the task's preset cfg)."""
    if getattr(args, "episode_stats", False) and getattr(args, "episode_stats_metrics", None):
        try:
            has_object = int(_abi.preset_cfg(args.task).task) != _abi.CONSTS["LT_TASK_LOCOMOTION"]
        except (AttributeError, KeyError):  # no or no registered task name: the env's constructor refuses it, by name
            has_object = True
        chosen_metrics(default_table(has_object), args.episode_stats_metrics)


def episode_stats_for(env, args, skip_running: bool = True):
    """The EpisodeStats the script arguments ask for, attached as `env.episode_stats`, or None without --episode_stats."""
    if not getattr(args, "episode_stats", False):
        return None
    stats = EpisodeStats(env, chosen_metrics(default_metrics(env), getattr(args, "episode_stats_metrics", None)), skip_running=skip_running)
    env.episode_stats = stats
    return stats


def report_for(stats, run_dir: str, mode: str):
    """Print the table and write <run_dir>/episode_stats/<mode>.json."""
    if stats is None:
        return None
    summary = stats.summary()
    print(f"[EpisodeStats] {mode}: episodes of {stats.num_envs} envs\n" + format_table(summary))
    path = stats.save(os.path.join(run_dir, "episode_stats", mode + ".json"), summary)
    print(f"[EpisodeStats] wrote {path}")
    return path


__all__ = ["EpisodeStats", "Metric", "default_table", "default_metrics", "default_metric_names", "chosen_metrics", "resolve_metric_names", "format_table", "add_episode_stats_args",
           "refuse_episode_stats_metrics", "episode_stats_for", "report_for", "TERMS", "REDUCES", "LENGTH"]
