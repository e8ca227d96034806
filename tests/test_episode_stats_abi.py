"""include/lt_episode_stats.h: a header of its own, bound by one row of `_abi.HEADERS`; the host-only byte counts against the numpy twin's
formulas; every refusal of lt_episode_stats_plan_write, _begin, _step, _clear_finished and _reduce by its field's name, before anything
is copied or launched (no device is needed: the pointers here are made-up addresses that a refused call never follows); the launch-count
queries; the twin's own arithmetic on hand-worked numbers; and the refusals of the Python front."""
import argparse
import ctypes

import numpy as np
import pytest

from locotouch_amd import _abi
from tests import episode_stats_ref as R

FAKE = 0x10000  # a 256-byte aligned address that is never dereferenced
C = _abi.EPISODE_STATS_CONSTS


def test_header_row_and_constants():
    rows = [r for r in _abi.HEADERS if r[1] == "lt_episode_stats.h"]
    assert len(rows) == 1 and rows[0][0] == "EPISODE_STATS" and rows[0][2] == "lt_telemetry.h"  # the channel is lt_telemetry.h's, not restated
    assert set(rows[0][3]) == {"lt_episode_stats_step_launches", "lt_episode_stats_reduce_launches"}
    assert set(_abi.EPISODE_STATS_SIGNATURES) == {
        "lt_episode_stats_plan_bytes", "lt_episode_stats_state_bytes", "lt_episode_stats_result_bytes", "lt_episode_stats_plan_write",
        "lt_episode_stats_begin", "lt_episode_stats_restart_running", "lt_episode_stats_step", "lt_episode_stats_clear_finished", "lt_episode_stats_reduce",
        "lt_episode_stats_step_launches", "lt_episode_stats_reduce_launches"}
    assert _abi.CONSTS["LT_ABI_VERSION"] == 21 and len(_abi.SIGNATURES) == 67  # lt_env.h is as it was
    assert "typedef struct lt_telemetry_channel" not in open(_abi.EPISODE_STATS_HEADER).read()
    assert (C["LT_EPISODE_STATS_MAX_METRICS"], C["LT_EPISODE_STATS_MAX_PAIRS"], C["LT_EPISODE_STATS_CAUSES"]) == (R.MAX_METRICS, R.MAX_PAIRS, R.CAUSES)
    assert C["LT_EPISODE_STATS_MAX_ENVS"] == R.MAX_ENVS == 16 * 65535 * 16
    assert [C["LT_EPISODE_STATS_" + n] for n in ("VALUE", "ABS", "SQUARE", "DIFF_SQUARE", "ABS_PRODUCT")] == [R.VALUE, R.ABS, R.SQUARE, R.DIFF_SQUARE, R.ABS_PRODUCT]
    assert [C["LT_EPISODE_STATS_" + n] for n in ("MEAN", "SUM", "MAX", "LAST")] == [R.MEAN, R.SUM, R.MAX, R.LAST]
    assert [C["LT_EPISODE_STATS_F_" + n] for n in ("N", "SUM", "SUMSQ", "MIN", "MAX")] == [R.F_N, R.F_SUM, R.F_SUMSQ, R.F_MIN, R.F_MAX]
    assert C["LT_EPISODE_STATS_FIELDS"] == 5
    pair, metric = _abi.LtEpisodeStatsPair, _abi.LtEpisodeStatsMetric
    assert ctypes.sizeof(pair) == 64 and pair.a.offset == 0 and pair.b.offset == 32 and pair._fields_[0][1] is _abi.LtTelemetryChannel
    assert [n for n, _ in metric._fields_] == ["npairs", "term", "reduce", "take_sqrt", "include_done_step", "pairs"]
    assert metric.pairs.offset == 24 and ctypes.sizeof(metric) == 24 + 12 * 64
    lib = _abi.load()
    for name in _abi.EPISODE_STATS_SIGNATURES:
        assert hasattr(lib, name)


def test_byte_counts_match_the_formulas():
    n = ctypes.c_size_t()
    for m in (1, 2, 11, 16):
        _abi.call("lt_episode_stats_plan_bytes", m, ctypes.byref(n))
        assert n.value == R.plan_bytes(m) == 112 + 784 * m
        _abi.call("lt_episode_stats_result_bytes", m, ctypes.byref(n))
        assert n.value == R.result_bytes(m) == 8 * 5 * (m + 1) + 8 * 18
        for nenvs in (1, 37, 4096, 4100, R.MAX_ENVS):
            _abi.call("lt_episode_stats_state_bytes", m, nenvs, ctypes.byref(n))
            assert n.value == R.state_bytes(m, nenvs) == nenvs * (40 * (m + 1) + 4 * m + 4 * m + 4 + 4 * 18 + 1)
            if nenvs <= 4100:  # the twin's own arrays have that many bytes
                assert len(R.Twin([(R.VALUE, R.MEAN, 0, 0)] * m, nenvs, True).state()) == n.value
    assert R.state_bytes(16, R.MAX_ENVS) > 1 << 33  # (counted in size_t, not in int)
    for fn, args, field in (("plan_bytes", (0,), "nmetrics must be in 1 ... 16"), ("plan_bytes", (17,), "nmetrics must be in 1 ... 16"),
                            ("result_bytes", (17,), "nmetrics must be in 1 ... 16"), ("state_bytes", (0, 4), "nmetrics must be in 1 ... 16"),
                            ("state_bytes", (1, 0), "nenvs must be in 1 ... 16776960"), ("state_bytes", (1, R.MAX_ENVS + 1), "nenvs must be in 1 ... 16776960")):
        with pytest.raises(RuntimeError, match=rf"code -22: lt_episode_stats_{fn}: invalid argument: {field}"):
            _abi.call("lt_episode_stats_" + fn, *args, ctypes.byref(n))
    with pytest.raises(RuntimeError, match="lt_episode_stats_plan_bytes: invalid argument: bytes must be non-null"):
        _abi.call("lt_episode_stats_plan_bytes", 1, None)


# ---- the plan ----
def _channel(base=FAKE, dtype=0, env_stride=4, offset=0):
    ch = _abi.LtTelemetryChannel()
    ch.base, ch.dtype, ch.env_stride, ch.offset = base, dtype, env_stride, offset
    return ch


def _metrics(n=1, npairs=1, term=R.VALUE, reduce=R.MEAN, take_sqrt=0, include_done_step=0, a=None, b=None):
    arr = (_abi.LtEpisodeStatsMetric * max(1, n))()
    for m in arr:
        m.npairs, m.term, m.reduce, m.take_sqrt, m.include_done_step = npairs, term, reduce, take_sqrt, include_done_step
        for p in m.pairs:
            p.a = a if a is not None else _channel()
            if b is not None:
                p.b = b
    return arr


def _write(metrics=None, nmetrics=None, dones=(), time_out=(), term_bits=(), nenvs=37, device_plan=FAKE, nbytes=1 << 16):
    metrics = _metrics() if metrics is None else metrics
    named = [None if c is None else (_channel() if c == () else c) for c in (dones, time_out, term_bits)]
    _abi.call("lt_episode_stats_plan_write", metrics, len(metrics) if nmetrics is None else nmetrics, *named, nenvs, device_plan, nbytes, None)


def _later(**fields):
    arr = _metrics(3)
    for k, v in fields.items():
        setattr(arr[2], k, v)
    return arr


PLAN_REFUSALS = {
    "no metrics": (lambda: _write(nmetrics=0), "nmetrics must be in 1 ... 16"),
    "17 metrics": (lambda: _write(_metrics(17)), "nmetrics must be in 1 ... 16"),
    "no pairs": (lambda: _write(_metrics(npairs=0)), r"metrics\[0\].npairs must be in 1 ... 12"),
    "13 pairs": (lambda: _write(_later(npairs=13)), r"metrics\[2\].npairs must be in 1 ... 12"),
    "diff_square without b": (lambda: _write(_metrics(term=R.DIFF_SQUARE)), r"metrics\[0\].pairs\[0\].b.base must be non-null and aligned to its element"),
    "abs_product without b": (lambda: _write(_metrics(2, npairs=3, term=R.ABS_PRODUCT)), r"metrics\[0\].pairs\[0\].b.base must be non-null and aligned to its element"),
    "term 5": (lambda: _write(_metrics(term=5)), r"metrics\[0\].term must be in 0 ... 4 \(VALUE, ABS, SQUARE, DIFF_SQUARE, ABS_PRODUCT\)"),
    "term -1": (lambda: _write(_later(term=-1)), r"metrics\[2\].term must be in 0 ... 4"),
    "reduce 4": (lambda: _write(_metrics(reduce=4)), r"metrics\[0\].reduce must be in 0 ... 3 \(MEAN, SUM, MAX, LAST\)"),
    "sqrt 2": (lambda: _write(_metrics(take_sqrt=2)), r"metrics\[0\].take_sqrt must be in 0 ... 1"),
    "include_done_step -1": (lambda: _write(_metrics(include_done_step=-1)), r"metrics\[0\].include_done_step must be in 0 ... 1"),
    "dtype 4": (lambda: _write(_metrics(a=_channel(dtype=4))), r"metrics\[0\].pairs\[0\].a.dtype must be in 0 ... 3"),
    "null base": (lambda: _write(_metrics(a=_channel(base=None))), r"metrics\[0\].pairs\[0\].a.base must be non-null and aligned to its element"),
    "misaligned f32": (lambda: _write(_metrics(a=_channel(base=FAKE + 2))), r"metrics\[0\].pairs\[0\].a.base must be non-null and aligned to its element"),
    "misaligned i64": (lambda: _write(_metrics(a=_channel(base=FAKE + 4, dtype=1))), r"metrics\[0\].pairs\[0\].a.base must be non-null and aligned to its element"),
    "misaligned b": (lambda: _write(_metrics(term=R.DIFF_SQUARE, b=_channel(base=FAKE + 1, dtype=3))), r"metrics\[0\].pairs\[0\].b.base must be non-null and aligned"),
    "negative stride": (lambda: _write(_metrics(a=_channel(env_stride=-1))), r"metrics\[0\].pairs\[0\].a.env_stride must be non-negative"),
    "negative offset": (lambda: _write(_metrics(a=_channel(offset=-1))), r"metrics\[0\].pairs\[0\].a.offset must be non-negative"),
    "misaligned dones": (lambda: _write(dones=_channel(base=FAKE + 4, dtype=1)), "dones.base must be non-null and aligned to its element"),
    "time_out dtype": (lambda: _write(time_out=_channel(dtype=9)), "time_out.dtype must be in 0 ... 3"),
    "term_bits offset": (lambda: _write(term_bits=_channel(offset=-2)), "term_bits.offset must be non-negative"),
    "null metrics": (lambda: _abi.call("lt_episode_stats_plan_write", None, 1, _channel(), _channel(), _channel(), 4, FAKE, 1 << 16, None), "metrics must be non-null"),
    "null dones": (lambda: _write(dones=None), "dones must be non-null"),
    "null time_out": (lambda: _write(time_out=None), "time_out must be non-null"),
    "null term_bits": (lambda: _write(term_bits=None), "term_bits must be non-null"),
    "no envs": (lambda: _write(nenvs=0), "nenvs must be in 1 ... 16776960"),
    "too many envs": (lambda: _write(nenvs=R.MAX_ENVS + 1), "nenvs must be in 1 ... 16776960"),
    "null plan": (lambda: _write(device_plan=None), "device_plan must be non-null and 16-byte aligned"),
    "misaligned plan": (lambda: _write(device_plan=FAKE + 8), "device_plan must be non-null and 16-byte aligned"),
    "too few bytes": (lambda: _write(_metrics(2), nbytes=R.plan_bytes(2) - 1), "bytes must be at least lt_episode_stats_plan_bytes"),
}


@pytest.mark.parametrize("case", list(PLAN_REFUSALS))
def test_plan_write_refuses_by_field_name_before_the_copy(case):
    call, field = PLAN_REFUSALS[case]
    # LT_EINVAL (-22), not LT_EHIP: the refusal comes from the host-side check, in front of the copy (which has no device here)
    with pytest.raises(RuntimeError, match=r"code -22: lt_episode_stats_plan_write: invalid argument: " + field):
        call()


def test_a_one_operand_term_does_not_look_at_b_and_a_later_pair_is_named():
    arr = _metrics(npairs=12, term=R.DIFF_SQUARE, b=_channel())
    arr[0].pairs[11].b = _channel(base=None)
    with pytest.raises(RuntimeError, match=r"metrics\[0\].pairs\[11\].b.base must be non-null"):
        _write(arr)
    arr[0].term = R.SQUARE  # b is absent in pair 11 and garbage elsewhere: a one-operand term gets as far as the plan's own checks
    arr[0].pairs[3].b = _channel(dtype=77)
    with pytest.raises(RuntimeError, match="device_plan must be non-null"):
        _write(arr, device_plan=None)
    arr[0].pairs[12 - 1].a = _channel(base=FAKE + 1, dtype=2)  # uint8: any address
    arr[0].npairs = 5
    arr[0].pairs[7].a = _channel(dtype=-3)  # behind npairs: ignored
    with pytest.raises(RuntimeError, match="device_plan must be non-null"):
        _write(arr, device_plan=None)


# ---- begin, step, clear, reduce ----
LAUNCH_REFUSALS = {
    "begin: no metrics": ("lt_episode_stats_begin", (FAKE, 0, 4, 1, None), "nmetrics must be in 1 ... 16"),
    "begin: no envs": ("lt_episode_stats_begin", (FAKE, 1, 0, 1, None), "nenvs must be in 1 ... 16776960"),
    "begin: null state": ("lt_episode_stats_begin", (None, 1, 4, 1, None), "state must be non-null and 16-byte aligned"),
    "begin: misaligned state": ("lt_episode_stats_begin", (FAKE + 8, 1, 4, 0, None), "state must be non-null and 16-byte aligned"),
    "begin: skip_running": ("lt_episode_stats_begin", (FAKE, 1, 4, 2, None), "skip_running must be in 0 ... 1"),
    "restart: no envs": ("lt_episode_stats_restart_running", (FAKE, 1, 0, 1, None), "nenvs must be in 1 ... 16776960"),
    "restart: 17 metrics": ("lt_episode_stats_restart_running", (FAKE, 17, 4, 1, None), "nmetrics must be in 1 ... 16"),
    "restart: misaligned state": ("lt_episode_stats_restart_running", (FAKE + 4, 1, 4, 0, None), "state must be non-null and 16-byte aligned"),
    "restart: skip_running": ("lt_episode_stats_restart_running", (FAKE, 1, 4, -1, None), "skip_running must be in 0 ... 1"),
    "step: 17 metrics": ("lt_episode_stats_step", (FAKE, FAKE, 17, 4, None), "nmetrics must be in 1 ... 16"),
    "step: no envs": ("lt_episode_stats_step", (FAKE, FAKE, 1, 0, None), "nenvs must be in 1 ... 16776960"),
    "step: too many envs": ("lt_episode_stats_step", (FAKE, FAKE, 1, R.MAX_ENVS + 1, None), "nenvs must be in 1 ... 16776960"),
    "step: null plan": ("lt_episode_stats_step", (None, FAKE, 1, 4, None), "device_plan must be non-null and 16-byte aligned"),
    "step: misaligned state": ("lt_episode_stats_step", (FAKE, FAKE + 4, 1, 4, None), "state must be non-null and 16-byte aligned"),
    "clear: no envs": ("lt_episode_stats_clear_finished", (FAKE, 1, 0, None), "nenvs must be in 1 ... 16776960"),
    "clear: null state": ("lt_episode_stats_clear_finished", (None, 1, 4, None), "state must be non-null and 16-byte aligned"),
    "reduce: no metrics": ("lt_episode_stats_reduce", (FAKE, 0, 4, FAKE, None), "nmetrics must be in 1 ... 16"),
    "reduce: no envs": ("lt_episode_stats_reduce", (FAKE, 1, 0, FAKE, None), "nenvs must be in 1 ... 16776960"),
    "reduce: null state": ("lt_episode_stats_reduce", (None, 1, 4, FAKE, None), "state must be non-null and 16-byte aligned"),
    "reduce: null result": ("lt_episode_stats_reduce", (FAKE, 1, 4, None, None), "result must be non-null and 8-byte aligned"),
    "reduce: misaligned result": ("lt_episode_stats_reduce", (FAKE, 1, 4, FAKE + 4, None), "result must be non-null and 8-byte aligned"),
}


@pytest.mark.parametrize("case", list(LAUNCH_REFUSALS))
def test_launches_refuse_by_field_name_before_the_launch(case):
    fn, args, field = LAUNCH_REFUSALS[case]
    with pytest.raises(RuntimeError, match=rf"code -22: {fn}: invalid argument: " + field):
        _abi.call(fn, *args)


def test_launch_counts():
    lib = _abi.load()
    assert lib.lt_episode_stats_step_launches(FAKE, FAKE, 11, 4096) == 1
    assert lib.lt_episode_stats_step_launches(FAKE, FAKE, 16, R.MAX_ENVS) == 1
    assert lib.lt_episode_stats_reduce_launches(FAKE, 11, 4096, FAKE) == 1
    assert lib.lt_episode_stats_reduce_launches(FAKE, 1, 1, FAKE + 8) == 1
    assert lib.lt_episode_stats_step_launches(FAKE, FAKE, 1, 0) == _abi.CONSTS["LT_EINVAL"]
    assert b"lt_episode_stats_step_launches: invalid argument: nenvs must be in 1 ... 16776960" in lib.lt_last_error()
    assert lib.lt_episode_stats_step_launches(FAKE + 4, FAKE, 1, 4) == _abi.CONSTS["LT_EINVAL"]
    assert lib.lt_episode_stats_reduce_launches(FAKE, 17, 4, FAKE) == _abi.CONSTS["LT_EINVAL"]
    assert b"lt_episode_stats_reduce_launches: invalid argument: nmetrics must be in 1 ... 16" in lib.lt_last_error()
    for name, args in (("lt_episode_stats_step_launches", (FAKE, FAKE, 1, 4)), ("lt_episode_stats_reduce_launches", (FAKE, 1, 4, FAKE))):
        with pytest.raises(TypeError, match=name):  # a value query is not a status
            _abi.call(name, *args)


# ---- the twin on hand-worked numbers ----
def test_twin_on_two_envs_by_hand():
    f = np.float32
    # env 0: samples 3, 4 then a done step (sample 100: left out by the state metrics, counted by the return); env 1 never finishes
    metrics = [(R.SQUARE, R.MEAN, 1, 0), (R.VALUE, R.SUM, 0, 1), (R.ABS, R.MAX, 0, 0), (R.VALUE, R.LAST, 0, 0)]
    twin = R.Twin(metrics, 2, skip_running=False)
    for a0, d0 in ((3, 0), (4, 0), (100, 1)):
        a = np.array([a0, -a0], f)
        twin.step([[(a, None)]] * 4, np.array([d0, 0]), np.array([d0, 0]), np.array([0b101 * d0, 0]))
    totals, causes = twin.reduce()
    r = float(np.sqrt(12.5))  # sqrt((9 + 16) / 2)
    assert totals[0].tolist() == [1.0, r, r * r, r, r]
    assert totals[1].tolist() == [1.0, 107.0, 107.0 ** 2, 107.0, 107.0]
    assert totals[2].tolist() == [1.0, 4.0, 16.0, 4.0, 4.0]
    assert totals[3].tolist() == [1.0, 100.0, 1e4, 100.0, 100.0]  # LAST reads the done step
    assert totals[4].tolist() == [1.0, 3.0, 9.0, 3.0, 3.0]  # the length counts the done step
    assert causes.tolist() == [1, 0, 1] + [0] * 13 + [1, 1]
    assert twin.run[:, 0].tolist() == [0, 0, 0, 0] and twin.count[:, 0].tolist() == [0, 0, 0, 0] and twin.steps.tolist() == [0, 3]
    assert twin.run[:3, 1].tolist() == [f(9 + 16) + f(1e4), -107.0, 100.0] and twin.count[:3, 1].tolist() == [3, 3, 3]
    # a second episode of env 0 that ends at its first step: no sample for the state metrics, so only return, LAST and length grow
    a = np.array([7, 0], f)
    twin.step([[(a, None)]] * 4, np.array([1, 0]), np.array([0, 0]), np.array([2, 0]))
    totals, causes = twin.reduce()
    assert [t[0] for t in totals.tolist()] == [1.0, 2.0, 1.0, 2.0, 2.0] and totals[4].tolist() == [2.0, 4.0, 10.0, 1.0, 3.0]
    assert causes.tolist() == [1, 1, 1] + [0] * 13 + [1, 2]
    twin.restart_running(skip_running=True)  # a reset of all envs: env 1's running episode is dropped, what finished stays
    assert not twin.run.any() and not twin.count.any() and twin.steps.tolist() == [0, 0] and twin.armed.tolist() == [0, 0]
    assert twin.reduce()[1].tolist() == causes.tolist()
    twin.step([[(a, None)]] * 4, np.array([1, 0]), np.array([0, 0]), np.array([2, 0]))  # with skip_running the next done only arms
    assert twin.reduce()[1].tolist() == causes.tolist() and twin.armed.tolist() == [1, 0] and twin.steps.tolist() == [0, 1]
    twin.clear_finished()
    assert not twin.fin.any() and not twin.causes.any() and twin.steps.tolist() == [0, 1] and twin.count[0].tolist() == [0, 1]


def test_twin_skips_the_running_episode_ignores_nan_in_max_and_sums_in_the_stated_order():
    f = np.float32
    twin = R.Twin([(R.VALUE, R.MAX, 0, 1)], 3, skip_running=True)
    seq = [([1, np.nan, 5], [1, 0, 0]), ([2, 1, np.nan], [0, 0, 0]), ([np.nan, 0, 1], [1, 1, 1])]
    for a, d in seq:
        twin.step([[(np.array(a, f), None)]], np.array(d), np.zeros(3), np.zeros(3))
    # env 0: its first done only armed it, then max(2, nan) = 2; env 1: seeded by NaN, and NaN stays (s > NaN is false); env 2: dropped
    assert twin.fin[0, R.F_N].tolist() == [1, 0, 0] and twin.fin[0, R.F_MAX, 0] == 2.0 and twin.armed.tolist() == [1, 1, 1]
    assert twin.fin[1, R.F_SUM].tolist() == [2, 0, 0] and twin.causes[17].tolist() == [1, 0, 0]
    # the order of the sums: 300 envs, thread 0 takes envs 0 and 256; 1e16 + 1 + 1 differs by where the ones are added
    twin = R.Twin([(R.VALUE, R.SUM, 0, 1)], 300, skip_running=False)
    a = np.ones(300, f)
    a[0] = 1e16
    twin.step([[(a, None)]], np.ones(300), np.zeros(300), np.zeros(300))
    totals, _ = twin.reduce()
    part = np.ones(256)
    part[0] = float(f(1e16)) + 1.0  # env 0 + env 256: the one is lost
    part[1:44] += 1.0  # envs 257 ... 299
    stride = 128
    while stride:
        part[:stride] = part[:stride] + part[stride:2 * stride]
        stride //= 2
    assert totals[0, R.F_SUM] == part[0] and totals[0, R.F_N] == 300.0 and totals[0, R.F_MIN] == 1.0 and totals[0, R.F_MAX] == float(f(1e16))


# ---- the Python front ----
def test_flags_names_and_refusals_of_the_python_front():
    import torch

    from locotouch_amd import episode_stats as ES
    from locotouch_amd.env import LocoTouchVecEnv

    ap = argparse.ArgumentParser()
    ES.add_episode_stats_args(ap)
    off = ap.parse_args([])
    assert (off.episode_stats, off.episode_stats_metrics) == (False, None)
    on = ap.parse_args(["--episode_stats", "--episode_stats_metrics", "return,power_mean"])
    ES.refuse_episode_stats_metrics(off)
    ES.refuse_episode_stats_metrics(on)
    with pytest.raises(ValueError, match=r"unknown episode-statistics metric 'powr'; known metrics: return, length, error_vel_xy, error_vel_yaw, speed_xy_rms"):
        ES.refuse_episode_stats_metrics(ap.parse_args(["--episode_stats", "--episode_stats_metrics", "return,powr"]))
    assert ES.default_metric_names() == ["return", "length", "error_vel_xy", "error_vel_yaw", "speed_xy_rms", "power_mean", "torque_rms", "joint_vel_rms",
                                         "total_foot_force_max", "root_height_mean", "object_offset_xy_max", "object_speed_rel_rms"]
    assert ES.default_metric_names(False)[-1] == "root_height_mean"
    assert [m.name for m in ES.chosen_metrics(ES.default_table(True), "power_mean,length,return")] == ["return", "power_mean"]  # the table's order
    assert ES.chosen_metrics(ES.default_table(False), None) == ES.default_table(False)
    with pytest.raises(ValueError, match="'length' is built in and always reported; name at least one metric beside it"):  # nothing is added silently
        ES.chosen_metrics(ES.default_table(True), "length")
    loco = ["--task", "Isaac-Locomotion-LocoTouch-v1", "--episode_stats", "--episode_stats_metrics", "return,object_offset_xy_max"]
    ap.add_argument("--task", default="Isaac-RandCylinderTransportTeacher-LocoTouch-v1")
    with pytest.raises(ValueError, match=r"unknown episode-statistics metric 'object_offset_xy_max'; known metrics: .*root_height_mean$"):
        ES.refuse_episode_stats_metrics(ap.parse_args(loco))  # a task without an object: refused before an env exists
    ES.refuse_episode_stats_metrics(ap.parse_args(loco[2:]))  # the teacher task has them
    env = object.__new__(LocoTouchVecEnv)  # never constructed (its constructor needs a device): the attributes the front looks at
    env.device, env.num_envs = torch.device("cpu"), 4
    assert env.episode_stats is None  # the hook: a class attribute, off
    assert ES.episode_stats_for(env, off) is None and env.episode_stats is None  # without the flag nothing is built
    with pytest.raises(RuntimeError, match="EpisodeStats needs a HIP device"):  # no fall-back
        ES.EpisodeStats(env, [ES.Metric("x", ((torch.zeros(4, 2), 0),))])
    table = ES.format_table({"return": {"episodes": 2, "mean": 1.5, "std": 0.5, "min": 1.0, "max": 2.0}, "length": {"episodes": 0},
                             "termination": {"time_out": 0.5}})
    assert "return" in table and "1.5" in table and "time_out=0.500" in table
