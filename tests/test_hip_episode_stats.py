"""GPU tests of the episode statistics (csrc/lt_episode_stats.hip) against the numpy twin (tests/episode_stats_ref.py), bit for bit: the
per-step term is float32 with every operation rounded on its own, the finish and the fold are float64 with IEEE division and square
root, and the sums over the envs have one stated order - so there is no tolerance anywhere.  Then the Python front on a real env, inside
a captured graph, and behind a FusedRollout."""
import numpy as np
import pytest

from tests import episode_stats_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TEACHER = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
GUARD = 256  # bytes in front of and behind the state and the result block (the state needs 16-byte alignment)
PATTERN = 0xA5


# ---- the caller's own tensors: all four dtypes ----
def _sources(rng, n, nan_ok=None):
    """Host arrays of the four dtypes, n rows each: a wider f32 tensor (its columns are strided), a quad field [n, 3, 4] laid out as the
    arena lays it out (storage [3][n][4]), i64 values that do not fit a float, u8, and i32 pairs.  Column 4 of `wide` holds a NaN in a
    tenth of the envs of `nan_ok` (those whose running episode has a sample already: a NaN never seeds a maximum here)."""
    src = {"wide": rng.standard_normal((n, 7)).astype(np.float32),
           "quad": (3.0 * rng.standard_normal((3, n, 4))).astype(np.float32),
           "i64": (2 ** 24 + rng.integers(-5, 2 ** 20, size=n)).astype(np.int64) * rng.choice([-1, 1], size=n),
           "u8": rng.integers(0, 256, size=n).astype(np.uint8),
           "i32": rng.integers(-1000, 1000, size=(n, 2)).astype(np.int32)}
    if nan_ok is not None:
        src["wide"][nan_ok & (rng.random(n) < 0.1), 4] = np.nan
    return src


def _value(src, name, index):
    a = src[name]
    return R.as_f32(a[index[0], :, index[1]] if name == "quad" else a[(slice(None),) + tuple(index)])


QUAD = [("quad", (q, lane)) for q in range(3) for lane in range(4)]  # 12 channels
WIDE = [("wide", (c,)) for c in range(7)]
MIXED = [("wide", (1,)), ("i64", ()), ("u8", ()), ("i32", (0,)), ("i32", (1,)), ("quad", (2, 3)), ("wide", (6,)), ("u8", ()), ("i32", (1,)), ("wide", (0,)),
         ("quad", (0, 0)), ("i64", ())]
# (name, a channels, b channels or None, term, reduce, sqrt, include_done_step): every g, every reduce, sqrt on and off,
# include_done_step on and off, 1 and 12 pairs
METRICS = [
    ("sum_value_done", [WIDE[0]], None, R.VALUE, R.SUM, 0, 1),
    ("max_abs_12", QUAD, None, R.ABS, R.MAX, 0, 0),
    ("rms_square_12", QUAD, None, R.SQUARE, R.MEAN, 1, 0),
    ("max_diff_sqrt", [WIDE[1], QUAD[0]], [WIDE[2], ("i32", (0,))], R.DIFF_SQUARE, R.MAX, 1, 0),
    ("mean_product_12", QUAD, MIXED, R.ABS_PRODUCT, R.MEAN, 0, 0),
    ("last_value", [WIDE[3]], None, R.VALUE, R.LAST, 0, 0),
    ("max_with_nan_done", [WIDE[4]], None, R.VALUE, R.MAX, 0, 1),
    ("last_square_sqrt_i64", [("i64", ())], None, R.SQUARE, R.LAST, 1, 1),
    ("sum_abs_ints", [("i32", (1,)), ("u8", ())], None, R.ABS, R.SUM, 0, 0),
    ("mean_value_done", [WIDE[5]], None, R.VALUE, R.MEAN, 0, 1),
    ("mean_diff_12", QUAD, QUAD[5:] + QUAD[:5], R.DIFF_SQUARE, R.MEAN, 0, 0),
    ("max_product_sqrt_done", [("u8", ())], [WIDE[6]], R.ABS_PRODUCT, R.MAX, 1, 1),
    ("sum_square_done", [WIDE[2], ("i32", (0,))], None, R.SQUARE, R.SUM, 1, 1),
]
TERM_NAMES = {v: k for k, v in (("value", R.VALUE), ("abs", R.ABS), ("square", R.SQUARE), ("diff_square", R.DIFF_SQUARE), ("abs_product", R.ABS_PRODUCT))}
REDUCE_NAMES = {R.MEAN: "mean", R.SUM: "sum", R.MAX: "max", R.LAST: "last"}


def _dones(pattern, n, steps, rng):
    """Scripted dones [steps][n]."""
    d = np.zeros((steps, n), np.int64)
    if pattern == "all":
        d[:] = 1
    elif pattern == "mixed":
        d[:] = rng.random((steps, n)) < 0.3
        d[0, ::4] = 1          # at step 0
        d[:, 3] = 0
        d[2:4, 3] = 1          # two in a row for env 3
        d[:, 5] = 0            # env 5 never finishes
        d[:, n - 1] = 0
        d[steps - 1, n - 1] = 1  # the last env: one episode as long as the run
    return d


class _Env:
    """What EpisodeStats looks at of an env, for channels that are all the caller's own tensors."""
    device = DEV

    def __init__(self, n, named):
        self.num_envs, self._named = n, named

    def episode_stats_channels(self):
        return {k: (t, 0) for k, t in self._named.items()}


class _Rig:
    """Device copies of the sources, an EpisodeStats over METRICS on them whose state and result lie between guard bytes, and the twin."""

    def __init__(self, n, skip_running, rng):
        import torch

        from locotouch_amd.episode_stats import EpisodeStats, Metric

        self.n, self.torch = n, torch
        self.host = _sources(rng, n)
        self.host.update(dones=np.zeros(n, np.int64), time_out=np.zeros(n, np.uint8), term_bits=np.zeros(n, np.int32))
        self.dev = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in self.host.items()}
        views = dict(self.dev)
        views["quad"] = self.dev["quad"].permute(1, 0, 2)  # [n, 3, 4] with strides (4, 4 n, 1)
        assert views["quad"].stride() == (4, 4 * n, 1)
        spec = lambda ch: (views[ch[0]], ch[1])  # noqa: E731
        metrics = []
        for name, a, b, term, reduce, sqrt, incl in METRICS:
            pairs = tuple(spec(x) for x in a) if b is None else tuple((spec(x), spec(y)) for x, y in zip(a, b))
            metrics.append(Metric(name, pairs, TERM_NAMES[term], REDUCE_NAMES[reduce], bool(sqrt), bool(incl)))
        env = _Env(n, {k: self.dev[k] for k in ("dones", "time_out", "term_bits")})
        self.stats = stats = EpisodeStats(env, metrics, skip_running=skip_running)
        m = len(METRICS)
        assert stats.state.numel() == R.state_bytes(m, n) and stats.result.numel() == R.result_bytes(m) and stats.plan.numel() == R.plan_bytes(m)
        self.state_buf = torch.full((2 * GUARD + stats.state.numel(),), PATTERN, dtype=torch.uint8, device=DEV)
        self.result_buf = torch.full((2 * GUARD + stats.result.numel(),), PATTERN, dtype=torch.uint8, device=DEV)
        stats.state, stats.result = self.state_buf[GUARD:-GUARD], self.result_buf[GUARD:-GUARD]
        assert stats.state.data_ptr() % 16 == 0 and stats.result.data_ptr() % 8 == 0
        stats.begin()
        self.twin = R.Twin([(term, reduce, sqrt, incl) for _, _, _, term, reduce, sqrt, incl in METRICS], n, skip_running)

    def load(self, fresh):
        for k, v in fresh.items():
            self.host[k] = v
            self.dev[k].copy_(self.torch.from_numpy(v))

    def step(self):
        self.stats.step()
        pairs = [[(_value(self.host, *x), None if b is None else _value(self.host, *y)) for x, y in zip(a, b or a)] for _, a, b, *_ in METRICS]
        self.twin.step(pairs, self.host["dones"], self.host["time_out"], self.host["term_bits"])

    def state(self) -> bytes:
        self.torch.cuda.synchronize()
        return self.stats.state.cpu().numpy().tobytes()

    def check_guards(self):
        for buf in (self.state_buf, self.result_buf):
            raw = buf.cpu().numpy()
            assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all()


def _diff(got: bytes, want: bytes, n, m):
    """Which of the state's arrays differ (for the assertion's message)."""
    names, at, out = (("finished", 8 * 5 * (m + 1) * n), ("run", 4 * m * n), ("count", 4 * m * n), ("steps", 4 * n), ("causes", 72 * n), ("armed", n)), 0, []
    for name, size in names:
        if got[at:at + size] != want[at:at + size]:
            out.append(name)
        at += size
    return out


def _run(n, steps, pattern, skip_running, seed=7):
    """The whole scripted run on a fresh rig, the twin stepped alongside: the device's and the twin's state bytes after every step, the
    result block's bytes, the rig, the dones and how many NaN samples each step held."""
    import torch

    rng = np.random.default_rng(seed)
    rig = _Rig(n, skip_running, rng)
    dones = _dones(pattern, n, steps, rng)
    states, twin_states, nans = [], [], []
    for t in range(steps):
        has_sample = (dones[t - 1] == 0) if t > 0 else np.zeros(n, bool)
        fresh = _sources(rng, n, nan_ok=has_sample)
        fresh.update(dones=dones[t], time_out=(dones[t] * (rng.random(n) < 0.5)).astype(np.uint8),
                     term_bits=(dones[t] * rng.integers(0, 1 << 16, size=n)).astype(np.int32))
        nans.append(int(np.isnan(fresh["wide"][:, 4]).sum()))
        rig.load(fresh)
        rig.step()
        states.append(rig.state())
        twin_states.append(rig.twin.state())
    rig.stats.totals()  # the reduce launch into the guarded result block
    torch.cuda.synchronize()
    return states, twin_states, rig.stats.result.cpu().numpy().tobytes(), rig, dones, nans


@pytest.mark.parametrize("skip_running", [True, False])
@pytest.mark.parametrize("pattern", ["none", "all", "mixed"])
@pytest.mark.parametrize("n,steps", [(37, 12), (4100, 6)])  # one ragged wave; several workgroups and the reduce's strided walk
def test_state_and_result_match_the_twin_bit_for_bit(n, steps, pattern, skip_running):
    from locotouch_amd import _abi

    m = len(METRICS)
    states, twin_states, result, rig, dones, nans = _run(n, steps, pattern, skip_running)
    twin = rig.twin
    lib = _abi.load()
    assert lib.lt_episode_stats_step_launches(rig.stats.plan.data_ptr(), rig.stats.state.data_ptr(), m, n) == 1
    assert lib.lt_episode_stats_reduce_launches(rig.stats.state.data_ptr(), m, n, rig.stats.result.data_ptr()) == 1
    for t in range(steps):  # running state, per-env accumulators and cause counters after every step
        assert states[t] == twin_states[t], (t, _diff(states[t], twin_states[t], n, m))
    assert result == twin.result()
    totals, causes = twin.reduce()
    episodes = int(dones.sum()) - (int((dones.sum(axis=0) > 0).sum()) if skip_running else 0)
    assert causes[17] == episodes == totals[m, R.F_N] and (episodes > 0) == (pattern != "none")
    if pattern == "mixed":
        assert twin.fin[m, R.F_N, 5] == 0 and twin.steps[5] == steps  # the env that never finishes
        assert twin.fin[m, R.F_MIN, 3] == 1.0  # two dones in a row: an episode of one step
        assert twin.fin[m, R.F_MAX, n - 1] == (0.0 if skip_running else steps)  # one episode as long as the run: dropped when running ones are
        assert sum(nans) > 0 and not np.isnan(totals).any()  # NaN samples were there, and the maximum ignored them
    rig.check_guards()
    # clear_finished leaves running episodes alone
    rig.stats.clear_finished()
    twin.clear_finished()
    assert rig.state() == twin.state()
    assert rig.stats.per_env()["steps"].cpu().numpy().tolist() == twin.steps.tolist()
    rig.stats.totals()
    rig.torch.cuda.synchronize()
    assert rig.stats.result.cpu().numpy().tobytes() == twin.result() == bytes(R.result_bytes(m))
    rig.check_guards()
    for k, v in rig.host.items():  # the sources are only read
        assert np.array_equal(rig.dev[k].cpu().numpy().view(np.uint8), v.view(np.uint8)), k


def test_two_runs_give_the_same_bits():
    a = _run(4100, 6, "mixed", False)
    b = _run(4100, 6, "mixed", False)
    assert a[0] == b[0] and a[2] == b[2]


@pytest.mark.parametrize("skip_running", [True, False])
def test_restart_running_drops_the_running_episodes_and_keeps_the_finished(skip_running):
    """lt_episode_stats_restart_running between two steps, bit for bit against the twin: run, count and steps are zero behind it, the
    arming is begin's, the accumulators and cause counters are untouched, the guards too."""
    n, steps = 300, 8
    rng = np.random.default_rng(3)
    rig = _Rig(n, skip_running, rng)
    dones = _dones("mixed", n, steps, rng)
    for t in range(steps):
        fresh = _sources(rng, n)
        fresh.update(dones=dones[t], time_out=dones[t].astype(np.uint8), term_bits=(dones[t] * 5).astype(np.int32))
        rig.load(fresh)
        rig.step()
        if t == 4:
            before = rig.twin.fin.copy(), rig.twin.causes.copy()
            assert rig.twin.steps.any() and rig.twin.count.any() and before[0].any()
            rig.stats.restart_running()
            rig.twin.restart_running(skip_running)
            assert rig.state() == rig.twin.state()
            per = rig.stats.per_env()
            assert not per["run"].any() and not per["count"].any() and not per["steps"].any() and bool((per["armed"] == (0 if skip_running else 1)).all())
            assert np.array_equal(per["finished"].cpu().numpy(), before[0]) and np.array_equal(per["causes"].cpu().numpy(), before[1])
        assert rig.state() == rig.twin.state(), t
    assert rig.twin.fin[len(METRICS), R.F_MAX].max() <= 5  # no episode runs across the restart (5 steps before it, 3 behind)
    rig.check_guards()


def test_a_plan_for_other_counts_makes_the_step_do_nothing():
    import torch

    from locotouch_amd import _abi

    rig = _Rig(37, False, np.random.default_rng(0))
    before = rig.state()
    _abi.call("lt_episode_stats_step", rig.stats.plan, rig.stats.state, len(METRICS) - 1, 37, _abi.stream(torch.device(DEV)))
    _abi.call("lt_episode_stats_step", rig.stats.plan, rig.stats.state, len(METRICS), 36, _abi.stream(torch.device(DEV)))
    _abi.call("lt_episode_stats_step", torch.zeros(R.plan_bytes(len(METRICS)), dtype=torch.uint8, device=DEV), rig.stats.state, len(METRICS), 37,
              _abi.stream(torch.device(DEV)))
    assert rig.state() == before
    rig.check_guards()


# ---- the Python front on a real env ----
def test_real_env_lengths_returns_and_causes_equal_the_hosts():
    """64 envs, max_episode_length 10, 40 random-action steps.  `length` totals equal the host's count from `dones`; `return` equals a
    host float32 running sum of reward_buf per episode, bit for bit; the time-out count equals the host's; the cause counters sum to
    the episodes plus, for every episode that ended with more than one bit of LT_F_TERM_BITS set (the time-out is bit 0 of that word,
    and two terms can fire in one step), its further bits - counted on the host from the same word, so where every episode has one cause
    the sum IS the episodes."""
    import torch

    from locotouch_amd.env import make
    from locotouch_amd.episode_stats import EpisodeStats, Metric, default_metrics

    n = 64
    env = make(TEACHER, num_envs=n, device=DEV, seed=3, max_episode_length=10)
    assert env.episode_stats is None
    stats = env.episode_stats = EpisodeStats(env, skip_running=False)  # the env was reset just now
    names = [m.name for m in default_metrics(env)]
    assert names == ["return", "error_vel_xy", "error_vel_yaw", "speed_xy_rms", "power_mean", "torque_rms", "joint_vel_rms", "total_foot_force_max",
                     "root_height_mean", "object_offset_xy_max", "object_speed_rel_rms"]
    g = torch.Generator(device="cpu").manual_seed(0)
    run = np.zeros(n, np.float32)
    length = np.zeros(n, np.int64)
    returns, lengths = [[] for _ in range(n)], [[] for _ in range(n)]
    time_outs = extra_bits = 0
    bit_counts = np.zeros(16, np.int64)
    snapshots = [[] for _ in range(n)]
    for _ in range(40):
        _, rew, dones, _ = env.step((1.2 * torch.randn(n, 12, generator=g)).to(DEV))
        rew, dones = rew.cpu().numpy(), dones.cpu().numpy()
        to, bits = env.time_out_buf.cpu().numpy(), env.view(env_bits_field()).cpu().numpy()
        last = env.field("LT_F_LAST_CMD_METRICS")[:, 0, 0].cpu().numpy()
        run = (run + (np.float32(0) + rew)).astype(np.float32)
        length += 1
        for e in np.nonzero(dones)[0]:
            returns[e].append(run[e])
            lengths[e].append(length[e])
            snapshots[e].append(last[e])
            time_outs += int(to[e] != 0)
            word = int(bits[e]) & 0xFFFF
            bit_counts += [(word >> b) & 1 for b in range(16)]
            extra_bits += bin(word).count("1") - 1
            run[e], length[e] = 0, 0
    episodes = sum(len(r) for r in returns)
    assert episodes >= n  # max_episode_length 10: every env finished some
    totals, causes = stats.totals()
    per = {k: v.cpu().numpy() for k, v in stats.per_env().items()}
    m = len(names)
    assert totals[m, R.F_N] == episodes == causes[17] and totals[m, R.F_SUM] == sum(sum(x) for x in lengths)
    assert totals[m, R.F_MAX] == max(max(x) for x in lengths if x) and totals[m, R.F_MIN] == min(min(x) for x in lengths if x)
    assert per["steps"].tolist() == length.tolist()
    for e in range(n):  # the return of every episode is the host's float32 running sum: n, sum (in episode order), min, max bit for bit
        want = np.array(returns[e], np.float64)
        acc = np.float64(0)
        for v in want:
            acc = acc + v
        got = per["finished"][0, :, e]
        assert got[R.F_N] == len(want) and got[R.F_SUM].tobytes() == acc.tobytes(), e
        if len(want):
            assert got[R.F_MIN] == want.min() and got[R.F_MAX] == want.max(), e
        snap = np.array(snapshots[e], np.float64)  # LAST reads the reset snapshot of the episode that finished
        assert per["finished"][1, R.F_N, e] == len(snap) and per["finished"][1, R.F_SUM, e] == sum(snap, np.float64(0)), e
    assert causes[16] == time_outs
    assert causes[:16].tolist() == bit_counts.tolist()
    assert int(causes[:16].sum()) == episodes + extra_bits
    summary = stats.summary()
    assert set(summary) == set(names) | {"length", "termination"} and summary["return"]["episodes"] == episodes
    assert all(np.isfinite([v[k] for k in ("mean", "std", "min", "max")]).all() for name, v in summary.items() if name != "termination" and v["episodes"])
    assert summary["termination"]["time_out"] == time_outs / episodes and {"user", "user_time_out"} < set(summary["termination"])
    assert summary["power_mean"]["min"] > 0 and summary["root_height_mean"]["mean"] > 0
    rec = stats.eval_record(clear=True)
    assert rec["Eval/length/mean"] == summary["length"]["mean"] and "Eval/termination/time_out" in rec
    assert stats.eval_record() == {}  # cleared: an iteration in which no episode finished logs nothing
    # without the attribute nothing is launched
    env.episode_stats = None
    before = stats.state.clone()
    env.step(torch.zeros(n, 12, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(stats.state, before)
    with pytest.raises(ValueError, match="unknown channel 'cmd.v'; known channels: root_pos.x"):
        EpisodeStats(env, [Metric("x", ("cmd.v",))])


def test_env_reset_between_steps_does_not_merge_episodes():
    """`env.reset()` resets every env without a `dones` (the DAgger loop calls it in front of every collection).  With the attribute set
    it restarts the running part of the statistics: the host, which drops its running episodes at the reset, counts the same episodes
    with the same lengths and float32 returns, and no length exceeds max_episode_length."""
    import torch

    from locotouch_amd.env import make
    from locotouch_amd.episode_stats import EpisodeStats

    n, limit = 64, 10
    env = make(TEACHER, num_envs=n, device=DEV, seed=4, max_episode_length=limit)
    stats = env.episode_stats = EpisodeStats(env, skip_running=False)
    g = torch.Generator(device="cpu").manual_seed(1)
    run, length = np.zeros(n, np.float32), np.zeros(n, np.int64)
    returns, lengths = [[] for _ in range(n)], [[] for _ in range(n)]
    for t in range(30):
        if t in (7, 19):  # mid-episode for most envs
            assert int(stats.per_env()["steps"].sum()) > 0
            env.reset()
            run[:], length[:] = 0, 0
        _, rew, dones, _ = env.step((1.2 * torch.randn(n, 12, generator=g)).to(DEV))
        run = (run + (np.float32(0) + rew.cpu().numpy())).astype(np.float32)
        length += 1
        for e in np.nonzero(dones.cpu().numpy())[0]:
            returns[e].append(run[e])
            lengths[e].append(length[e])
            run[e], length[e] = 0, 0
    per = {k: v.cpu().numpy() for k, v in stats.per_env().items()}
    m = len(stats.metrics)
    host_max = max(max(x) for x in lengths if x)
    assert per["finished"][m, R.F_MAX].max() == host_max <= limit  # merged episodes would be longer than the host's and than the limit
    assert per["steps"].tolist() == length.tolist() and sum(len(x) for x in lengths) > n
    for e in range(n):
        acc = np.float64(0)
        for v in returns[e]:
            acc = acc + np.float64(v)
        assert per["finished"][m, R.F_N, e] == len(lengths[e]) and per["finished"][m, R.F_SUM, e] == sum(lengths[e]), e
        assert per["finished"][0, R.F_SUM, e].tobytes() == acc.tobytes(), e


def env_bits_field():
    from locotouch_amd import _abi

    return _abi.CONSTS["LT_F_TERM_BITS"]


def _graph_rig(n):
    import torch

    from locotouch_amd.episode_stats import EpisodeStats, Metric

    src = torch.linspace(-2.0, 3.0, n * 3, device=DEV).reshape(n, 3).contiguous()
    named = {"dones": torch.zeros(n, dtype=torch.int64, device=DEV), "time_out": torch.zeros(n, dtype=torch.uint8, device=DEV),
             "term_bits": torch.zeros(n, dtype=torch.int32, device=DEV)}
    k = torch.zeros(n, dtype=torch.int64, device=DEV)
    idx = torch.arange(n, dtype=torch.int64, device=DEV)
    metrics = [Metric("a", ((src, 0), (src, 2)), "square", "mean", sqrt=True), Metric("b", (((src, 1), (src, 0)),), "abs_product", "max", include_done_step=True),
               Metric("c", ((src, 2),), "value", "sum", include_done_step=True), Metric("d", ((src, 1),), "value", "last")]
    stats = EpisodeStats(_Env(n, named), metrics, skip_running=True)

    def step():  # one "env step" on the current stream: new values, new dones, then the statistics
        k.add_(1)
        src.mul_(-1.03125).add_(0.25)
        done = (k + idx) % 5 == 0
        named["dones"].copy_(done)
        named["time_out"].copy_(done & (idx % 2 == 0))
        named["term_bits"].copy_(done * (idx % 7 + 1))
        stats.step()

    return stats, step


def test_four_captured_steps_replayed_three_times_equal_twelve_eager_steps():
    import torch

    n = 300
    eager, step = _graph_rig(n)
    for _ in range(12):
        step()
    torch.cuda.synchronize()
    want = eager.state.cpu().numpy().tobytes()
    assert eager.totals()[1][17] > n  # episodes finished
    stats, step = _graph_rig(n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):  # one stream: no parallel branches
            for _ in range(4):
                step()
    torch.cuda.synchronize()
    assert int(stats.per_env()["steps"].sum()) == 0  # a capture launches nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert stats.state.cpu().numpy().tobytes() == want


def test_fused_rollout_with_the_attribute_leaves_the_storage_as_without_it():
    import torch

    from locotouch_amd.env import LocoTouchVecEnv
    from locotouch_amd.episode_stats import EpisodeStats
    from locotouch_amd.rl import PPO, ActorCritic, FusedRollout

    n, T = 64, 8
    runs = []
    for attach in (False, True):
        env = LocoTouchVecEnv(TEACHER, num_envs=n, device=DEV, seed=42, max_episode_length=5)  # (every env finishes an episode inside the rollout)
        torch.manual_seed(1234)
        ac = ActorCritic(env.num_obs, env.num_obs, 12, init_noise_std=1.0, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128],
                         activation="elu")
        alg = PPO(ac, device=DEV)
        alg.init_storage(n, T, [env.num_obs], [env.num_obs], [12])
        stats = None
        if attach:
            stats = env.episode_stats = EpisodeStats(env, skip_running=False)
        fused = FusedRollout(env, alg)
        fused.rollout(T)
        torch.cuda.synchronize()
        st = alg.storage
        runs.append([t.clone() for t in (st.observations, st.privileged_observations, st.actions, st.rewards, st.dones, st.values)])
        if attach:
            per = stats.per_env()
            lengths = per["finished"][len(stats.metrics), R.F_SUM].to(torch.int64)
            assert torch.equal(lengths + per["steps"], torch.full((n,), T, dtype=torch.int64, device=DEV))  # every step of every env was counted
            assert int(per["causes"][17].sum()) == int(st.dones.sum()) > 0
        del fused, alg, ac
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- the script ----
def test_play_script_writes_the_table_and_refuses_an_unknown_metric_by_name(tmp_path):
    """scripts/play.py --episode_stats on 16 envs, in a fresh child process: the JSON holds the default metrics' keys with finite numbers;
    an unknown metric name is refused by name before anything is built."""
    import json
    import os
    import subprocess
    import sys

    import torch

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.env import make
    from locotouch_amd.episode_stats import default_metric_names
    from locotouch_amd.rl import OnPolicyRunner
    from locotouch_amd.scripts.train import dump_params

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    task = "Isaac-RandCylinderTransportTeacher-LocoTouch-Play-v1"
    base = [sys.executable, "-m", "locotouch_amd.scripts.play", "--task", task, "--num_envs", "16", "--device", DEV, "--steps", "1010", "--episode_stats"]
    # (1010 steps: the play task's episodes time out after 1000 at the latest, so episodes finish whatever the untrained policy does)
    kw = dict(cwd=repo, env=dict(os.environ, PYTHONPATH=repo), capture_output=True, text=True, timeout=120)
    r = subprocess.run(base + ["--episode_stats_metrics", "return,powr", "--checkpoint", str(tmp_path / "none.pt")], **kw)
    assert r.returncode != 0 and "unknown episode-statistics metric 'powr'; known metrics: return, length" in r.stderr, r.stderr[-2000:]
    assert "Loading experiment" not in r.stdout  # refused before anything was looked up or built
    cfg = train_cfg(task)
    env = make(task, num_envs=16, device=DEV, seed=1)
    runner = OnPolicyRunner(env, cfg, log_dir=None, device=DEV)
    run = tmp_path / "run"
    run.mkdir()
    runner.save(str(run / "model_0.pt"))
    dump_params(str(run), {}, cfg)
    del runner, env
    torch.cuda.synchronize()
    r = subprocess.run(base + ["--checkpoint", str(run / "model_0.pt")], **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "[EpisodeStats] play: episodes of 16 envs" in r.stdout and "termination: " in r.stdout, r.stdout[-2000:]
    doc = json.load(open(run / "episode_stats" / "play.json"))
    assert doc["num_envs"] == 16 and doc["skip_running"] is False
    summary = doc["summary"]
    assert set(summary) == set(default_metric_names()) | {"termination"} and set(doc["metrics"]) == set(default_metric_names()) - {"length"}
    assert summary["length"]["episodes"] >= 16 and summary["length"]["max"] <= 1000
    for name, v in summary.items():
        if name != "termination" and v["episodes"]:
            assert all(np.isfinite(v[k]) for k in ("mean", "std", "min", "max")), name
    assert all(0.0 <= share <= 1.0 for share in summary["termination"].values())
