"""The episode ledger in HIP kernels (csrc/lt_ledger.hip behind include/lt_ledger.h, locotouch_amd/distill/device_ledger.py) on the GPU,
against `host_model` below: a plain-Python restatement of the two bookkeeping loops of locotouch_amd/distill/replay_buffer.py
(`collect_data`'s `bookkeeping`, `evaluate`'s window loop).  The kernel is compared with that model, never with itself, and EVERY
comparison is bit for bit: f64 sums are compared as Python floats / int64 bit patterns, there is no tolerance anywhere.

End to end the switch is compared with the host bookkeeping of `ReplayBuffer` itself.  The ledger loop learns of the stop one poll
interval later than the host loop (by design: it never blocks), so the two twins leave their envs in different states; every phase
therefore starts from a fresh, identically seeded env pair, and `evaluate` carries the reward sums its `collect_data` left."""
import collections
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STUDENT = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"
DEV = "cuda:0"
T = 40
CHUNK = 1024  # envs per pass of the step kernel's one workgroup
SIZES = [1, 37, 1024, 1025, 4100]  # a single lane, a partial wave, exactly one chunk, a chunk carry of one env, several chunks


# ---- the host model ---------------------------------------------------------------------------------------------------------------
def host_model(rewards, dones, sums0, keep_target=None, episode_target=None):
    """rewards [T][n] f32, dones [T][n] bool (numpy), sums0 [n] f32 or None.  Python floats are f64, so `sums[e] += float(r)` is the one
    f64 add per env per step of `reward_sums[:] += r[i]`.  Returns the lists, the counters and, per step, (done envs, kept envs)."""
    n = rewards.shape[1]
    sums = [0.0] * n if sums0 is None else [float(x) for x in sums0]
    start = [0] * n
    episodes, trajs, per_step = [], [], []
    kept_steps = stopped_at = step = 0
    for t in range(rewards.shape[0]):
        if stopped_at:
            break
        step = s = t + 1
        for e in range(n):
            sums[e] += float(rewards[t][e])
        done = [e for e in range(n) if dones[t][e]]
        episodes.extend((sums[e], s - start[e]) for e in done)       # rewards_out / lengths_out: `start` as it was
        for e in done:
            sums[e] = 0.0
        kept = []
        for e in done:
            if keep_target is None or kept_steps < keep_target:
                kept_steps += s - start[e]
                trajs.append((e, start[e], s))
                start[e] = s
                kept.append(e)
            else:
                break
        per_step.append((done, kept))
        if (keep_target is not None and kept_steps >= keep_target) or (episode_target is not None and len(episodes) >= episode_target):
            stopped_at = s
    return dict(episodes=episodes, trajs=trajs, kept_steps=kept_steps, stopped_at=stopped_at, step=step, per_step=per_step,
                sums_f32=np.asarray(sums, dtype=np.float64).astype(np.float32), start=start)


@functools.lru_cache(maxsize=None)
def stream(n):
    """Seeded f32 rewards, done flags with probability 0.15 per env-step, carried f32 sums - and the two targets, placed with the
    un-targeted model run: the keep target so that the run stops inside the done list of a step in the middle of the stream (for
    n = 4100: behind a kept env of the third chunk), the episode target inside another step's list."""
    g = np.random.default_rng(1000 + n)
    rewards = g.standard_normal((T, n)).astype(np.float32)
    dones = g.random((T, n)) < 0.15
    sums0 = g.standard_normal(n).astype(np.float32)
    free = host_model(rewards, dones, sums0)
    if n == 1:  # one env: a done list has one entry; stop on the env's third episode
        keep = sum(length for _, length in free["episodes"][:2]) + 1
        ep_target = 2
    else:
        t_stop = next(t for t in range(T // 2, T) if len(free["per_step"][t][0]) >= 3)
        done = free["per_step"][t_stop][0]
        j = (len(done) - 1) // 2 if n < 4100 else next(i for i, e in enumerate(done) if e >= 2 * CHUNK + 7)
        before = [tr for tr in free["trajs"] if tr[2] <= t_stop]
        in_step = [tr for tr in free["trajs"] if tr[2] == t_stop + 1]
        keep = sum(end - s for _, s, end in before) + sum(end - s for _, s, end in in_step[:j]) + 1  # entries 0 .. j of the list are kept
        ep_target = sum(len(d) for d, _ in free["per_step"][:T // 3]) + 2
    return rewards, dones, sums0, keep, ep_target


# ---- the device side ----------------------------------------------------------------------------------------------------------------
class Dev:
    """The raw C ABI: a state and lists of the caller's own."""

    def __init__(self, n, ep_cap, traj_cap, slack=0, fill=-7):
        import torch

        from locotouch_amd import _abi

        self.n, self.ep_cap, self.traj_cap = n, ep_cap, traj_cap
        self.state = torch.zeros(8 + 2 * n, dtype=torch.int64, device=DEV)
        self.ep_reward = torch.full((ep_cap + slack,), float(fill), dtype=torch.float64, device=DEV)
        self.ep_length = torch.full((ep_cap + slack,), fill, dtype=torch.int64, device=DEV)
        self.traj = torch.full((traj_cap + slack, 3), fill, dtype=torch.int64, device=DEV)
        self._abi = _abi

    def begin(self, sums0, keep, ep_target):
        import torch

        s = None if sums0 is None else torch.from_numpy(sums0).to(DEV)
        self._abi.call("lt_ledger_begin", self.state, self.n, s, -1 if keep is None else keep, -1 if ep_target is None else ep_target,
                       self._abi.stream(DEV))

    def step(self, reward, done, with_traj=True):
        self._abi.call("lt_ledger_step", self.state, self.n, reward, done, self.ep_reward, self.ep_length, 0, self.ep_cap,
                       self.traj if with_traj else None, 0, self.traj_cap if with_traj else 0, self._abi.stream(DEV))

    def end(self):
        import torch

        out = torch.full((self.n,), 9.0, device=DEV)
        self._abi.call("lt_ledger_end", self.state, self.n, out, self._abi.stream(DEV))
        return out

    def snapshot(self):
        return [x.clone() for x in (self.state, self.ep_reward, self.ep_length, self.traj)]

    def head(self):
        from locotouch_amd.distill.device_ledger import LedgerHead

        return LedgerHead(*self.state[:8].tolist())


def bits(x):
    """f64 values as their int64 bit patterns."""
    return np.asarray(x, dtype=np.float64).view(np.int64).tolist()


def check_against(model, dev, keep, ep_target, with_traj=True):
    h = dev.head()
    assert (h.step, h.kept_steps, h.stopped_at, h.overflow) == (model["step"], model["kept_steps"], model["stopped_at"], 0), h
    assert h.episodes == len(model["episodes"]) and h.trajs == len(model["trajs"])
    assert (h.keep_target, h.episode_target) == (-1 if keep is None else keep, -1 if ep_target is None else ep_target)
    k = h.episodes
    assert bits(dev.ep_reward[:k].cpu().numpy()) == bits([r for r, _ in model["episodes"]])          # values AND order
    assert dev.ep_length[:k].tolist() == [length for _, length in model["episodes"]]
    if with_traj:
        assert [tuple(t) for t in dev.traj[:h.trajs].tolist()] == model["trajs"]
    assert dev.end().cpu().numpy().view(np.int32).tolist() == model["sums_f32"].view(np.int32).tolist()
    assert dev.state[8 + dev.n:].tolist() == model["start"]
    assert (dev.ep_length[k:] == -7).all() and (dev.traj[h.trajs if with_traj else 0:] == -7).all()  # nothing behind the lists' ends


def run_stream(n, keep, ep_target, carried, with_traj=True):
    """All T steps are issued whatever the ledger does; the state and lists behind the model's stopping step must be the final ones."""
    import torch

    rewards, dones, sums0, _, _ = stream(n)
    sums0 = sums0 if carried else None
    model = host_model(rewards, dones, sums0, keep, ep_target)
    dev = Dev(n, T * n, T * n)
    r_dev, d_dev = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
    dev.begin(sums0, keep, ep_target)
    at_stop = None
    for t in range(T):
        dev.step(r_dev[t], d_dev[t], with_traj)
        if t + 1 == model["stopped_at"]:
            at_stop = dev.snapshot()
    check_against(model, dev, keep, ep_target, with_traj)
    return model, dev, at_stop


@pytest.mark.parametrize("n", SIZES)
def test_keep_target_stream_is_bit_exact_and_stops_mid_list(n):
    import torch

    rewards, dones, sums0, keep, _ = stream(n)
    model, dev, at_stop = run_stream(n, keep, None, carried=True)
    # what the case must exercise, asserted on the host model alone
    per_step = model["per_step"]
    assert 0 < model["stopped_at"] < T - 2 and any(x != 0.0 for x in sums0)
    done, kept = per_step[-1]
    if n == 1:
        assert sum(len(d) for d, _ in per_step) == 3 and model["kept_steps"] >= keep
    else:
        assert any(len(d) >= 3 for d, _ in per_step)
        assert 0 < len(kept) < len(done) and done[:len(kept)] == kept  # the mid-list stop: a kept and an unkept env in one done list
        assert model["start"][done[-1]] != model["stopped_at"]          # (the unkept env's start is left alone)
    if n == 4100:
        assert len({e // CHUNK for e in done}) >= 3 and kept[-1] // CHUNK >= 1 and done[-1] // CHUNK > kept[-1] // CHUNK
    # steps issued after the stop left everything byte-identical
    assert at_stop is not None
    for a, b in zip(at_stop, dev.snapshot()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", SIZES)
def test_episode_target_and_no_target_streams_are_bit_exact(n):
    import torch

    _, _, _, _, ep_target = stream(n)
    model, dev, at_stop = run_stream(n, None, ep_target, carried=False, with_traj=False)   # evaluate's form: NULL sums, no traj list
    done, kept = model["per_step"][-1]
    assert 0 < model["stopped_at"] < T - 2 and len(model["episodes"]) >= ep_target and kept == done
    if n > 1:
        assert len(model["episodes"]) > ep_target  # the stopping step's whole done list is in, past the target
    for a, b in zip(at_stop, dev.snapshot()):
        assert torch.equal(a, b)
    model, dev, at_stop = run_stream(n, None, None, carried=True)
    assert model["stopped_at"] == 0 and at_stop is None and model["step"] == T
    assert len(model["trajs"]) == len(model["episodes"]) > 0


def test_both_targets_together_stop_on_the_earlier_one():
    _, _, _, keep, ep_target = stream(37)
    a = run_stream(37, keep, ep_target, carried=True)[0]
    assert a["stopped_at"] == min(host_model(*stream(37)[:3], keep, None)["stopped_at"], host_model(*stream(37)[:3], None, ep_target)["stopped_at"])


def test_too_small_caps_report_overflow_and_keep_what_fits():
    import torch

    n, steps, ep_cap, traj_cap = 37, 10, 5, 3
    rewards, dones, sums0, _, _ = stream(n)
    model = host_model(rewards[:steps], dones[:steps], sums0)
    assert len(model["episodes"]) > ep_cap + 3 and len(model["trajs"]) > traj_cap + 3
    dev = Dev(n, ep_cap, traj_cap, slack=16)
    r_dev, d_dev = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
    dev.begin(sums0, None, None)
    for t in range(steps):
        dev.step(r_dev[t], d_dev[t])
    h = dev.head()
    assert h.episodes == len(model["episodes"]) and h.trajs == len(model["trajs"]) and h.step == steps
    assert h.overflow == (len(model["episodes"]) - ep_cap) + (len(model["trajs"]) - traj_cap)
    assert bits(dev.ep_reward[:ep_cap].cpu().numpy()) == bits([r for r, _ in model["episodes"][:ep_cap]])
    assert dev.ep_length[:ep_cap].tolist() == [length for _, length in model["episodes"][:ep_cap]]
    assert [tuple(t) for t in dev.traj[:traj_cap].tolist()] == model["trajs"][:traj_cap]
    assert (dev.ep_reward[ep_cap:] == -7.0).all() and (dev.ep_length[ep_cap:] == -7).all() and (dev.traj[traj_cap:] == -7).all()
    assert dev.end().cpu().numpy().view(np.int32).tolist() == model["sums_f32"].view(np.int32).tolist()  # the books themselves are right


def test_python_front_spills_polls_late_and_turns_overflow_into_an_error():
    """A window of 2 steps and no poll in time: `step` reads the lists away (a blocking drain) before they can overflow, `first` moves,
    and what `drain` returns in the end is the model's whole list.  `poll` hands out the head of the call before."""
    import torch

    from locotouch_amd import _abi
    from locotouch_amd.distill import DeviceEpisodeLedger

    n = 37
    rewards, dones, sums0, keep, _ = stream(n)
    model = host_model(rewards, dones, sums0, keep, None)
    led = DeviceEpisodeLedger(DEV, n, window=2)
    r_dev, d_dev = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
    sums = torch.from_numpy(sums0).to(DEV)
    led.begin(sums, keep_target=keep)
    assert led.poll() is None
    heads = []
    for t in range(T):
        led.step(r_dev[t], d_dev[t])
        if (t + 1) % 8 == 0:
            heads.append(led.poll())
    assert led._ep_first > 0 and led._traj_first > 0                     # it did spill
    assert [h.step for h in heads] == [min(s, model["stopped_at"]) for s in (0, 8, 16, 24, 32)]   # each poll: the head of the poll before
    stopped = next(h for h in heads if h.stopped_at)
    rew, lengths, trajs = led.drain(stopped)
    assert bits(rew) == bits([r for r, _ in model["episodes"]]) and lengths == [length for _, length in model["episodes"]]
    assert trajs == model["trajs"] and stopped.kept_steps == model["kept_steps"] and stopped.stopped_at == model["stopped_at"]
    led.end(sums)
    assert sums.cpu().numpy().view(np.int32).tolist() == model["sums_f32"].view(np.int32).tolist()
    # an overflow the device reports is an error: a step launched past the front's own accounting, into lists of one slot
    led.begin(None)
    every = torch.ones(n, dtype=torch.bool, device=DEV)
    _abi.call("lt_ledger_step", led._state, n, r_dev[0], every, led._ep_reward, led._ep_length, 0, 1, led._traj, 0, 1, _abi.stream(DEV))
    with pytest.raises(RuntimeError, match="did not fit"):
        led.read_head()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
N_E2E, CHECK_EVERY = 64, 16


def make_student(tmp, seed=5):
    import torch

    from locotouch_amd.distill import Student, distillation_cfg

    cfg = distillation_cfg(STUDENT)
    cfg.device, cfg.log_dir = DEV, str(tmp)
    torch.manual_seed(seed)
    return Student(cfg, 270, 442, 12, verbose=False).eval()


class CopyLog:
    """Every device-to-host copy torch issues while active, as (bytes, env steps taken so far), seen at the dispatcher."""

    def __init__(self, counter):
        import torch
        from torch.utils._python_dispatch import TorchDispatchMode

        log = self.log = []

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                name = func.overloadpacket.__name__
                src = None
                if name == "copy_" and args[0].device.type == "cpu":
                    src = args[1]
                elif name in ("_to_copy", "_local_scalar_dense") and (name != "_to_copy" or out.device.type == "cpu"):
                    src = args[0]
                if isinstance(src, torch.Tensor) and src.device.type == "cuda":
                    log.append((src.numel() * src.element_size(), counter[0]))
                return out

        self.mode = Mode()


def profiled(fn):
    """(kernel names in launch order, memcpy / memset names) of fn(), counted as tests/test_hip_collect.py counts."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    dev = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA), key=lambda e: e.time_range.start)
    names = [e.name for e in dev]
    return out, [k for k in names if "memcpy" not in k.lower() and "memset" not in k.lower()], [k for k in names if "memcpy" in k.lower()]


_COLLECTED = {}


def student_collection(tmp, switch):
    if switch not in _COLLECTED:  # (computed once, shared by the tests below, never changed)
        _COLLECTED[switch] = _student_collection(tmp, switch)
    return _COLLECTED[switch]


def _student_collection(tmp, switch):
    """A fresh seeded env, the student through `FusedStudent`, the device recorder: `collect_data` under the profiler and the copy log."""
    import torch

    from locotouch_amd.distill import DeviceTactileRecorder, ReplayBuffer
    from locotouch_amd.distill.fused_student import FusedStudent
    from locotouch_amd.env import make

    n = N_E2E
    st = make_student(tmp)
    torch.manual_seed(21)
    env = make(STUDENT, num_envs=n, device=DEV, seed=3)
    env.episode_length_buf = torch.randint(440, 500, (n,), device=DEV)  # episodes end inside the run
    rb = ReplayBuffer(env, DeviceTactileRecorder(DEV, n, 442, 3, 7), 270, check_every=CHECK_EVERY, device_ledger=switch)
    rb._reward_sums.copy_(torch.randn(n, device=DEV))                   # carried sums that are not zero
    fs = FusedStudent.for_student(st)
    steps, real_step = [0], env.step

    def counting_step(a):
        steps[0] += 1
        return real_step(a)

    env.step = counting_step
    copies = CopyLog(steps)
    torch.manual_seed(22)

    def go():
        with copies.mode:
            return rb.collect_data(lambda obs: 0.1 * obs[..., :12], fs, num_steps=600)

    (rewards, lengths), kernels, memcpys = profiled(go)
    (policy, tactile), _ = rb._materialise()
    return dict(rewards=rewards, lengths=lengths, first=list(rb._traj_first), len=list(rb._traj_len), steps_count=rb._steps_count,
                sums=rb._reward_sums.clone(), policy=policy.clone(), tactile=tactile.clone(), env_steps=steps[0], kernels=kernels,
                memcpys=memcpys, copies=list(copies.log), st=st)


def same_collection(want, got, num_steps):
    import torch

    assert bits(got["rewards"]) == bits(want["rewards"]) and got["lengths"] == want["lengths"] and len(want["rewards"]) > 0
    assert all(type(x) is int for x in got["lengths"]) and all(type(x) is float for x in got["rewards"])
    assert got["first"] == want["first"] and got["len"] == want["len"] and len(want["first"]) > 0
    assert got["steps_count"] == want["steps_count"] >= num_steps
    assert torch.equal(got["sums"].view(torch.int32), want["sums"].view(torch.int32))
    assert torch.equal(got["policy"], want["policy"]) and torch.equal(got["tactile"], want["tactile"])


def test_student_collection_is_unchanged_by_the_switch(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ledger")
    want, got = student_collection(tmp, False), student_collection(tmp, True)
    same_collection(want, got, 600)
    # the ledger loop learns of the stop one poll interval later than the host loop, and never more
    assert want["env_steps"] % CHECK_EVERY == 0 and got["env_steps"] == want["env_steps"] + CHECK_EVERY


def test_launches_and_copies_of_the_collection_loop(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ledger")
    off, on = student_collection(tmp, False), student_collection(tmp, True)

    def regular_step(kernels, at_least):
        """The launches between two consecutive env-step kernels: the one list that nearly every step shows (the first step also
        allocates the store, and the host loop's poll intervals end with its `cat`s)."""
        at = [i for i, k in enumerate(kernels) if "lt_step_kernel" in k]
        segments = collections.Counter(tuple(sorted(k.split("<")[0] for k in kernels[a + 1:b])) for a, b in zip(at, at[1:]))
        launches, count = segments.most_common(1)[0]
        assert count >= at_least, segments
        return list(launches)

    T_off, T_on = off["env_steps"], on["env_steps"]
    base = regular_step(off["kernels"], T_off - T_off // CHECK_EVERY - 2)
    with_ledger = regular_step(on["kernels"], T_on - 2)
    print("launches per step, switch off:", 1 + len(base), base)
    print("launches per step, switch on :", 1 + len(with_ledger), with_ledger)
    ledger = [k for k in with_ledger if "lt_ledger_step" in k]
    assert len(ledger) == 1 and with_ledger == sorted(base + ledger)      # exactly one more launch per step
    assert sum("lt_ledger_step" in k for k in on["kernels"]) == on["env_steps"] and not any("lt_ledger" in k for k in off["kernels"])
    # device-to-host copies: the host loop reads [16][N] rewards and dones every window; the ledger loop reads 64 bytes per poll
    # inside the loop and the lists once behind it
    n = N_E2E
    print("d2h copies (bytes, env steps so far), off:", off["copies"])
    print("d2h copies (bytes, env steps so far), on :", on["copies"])
    print("memcpy nodes on:", sorted(set(on["memcpys"])))
    assert sum(b == CHECK_EVERY * n * 4 for b, _ in off["copies"]) == off["env_steps"] // CHECK_EVERY  # (the log sees the host loop's reads)
    in_loop = [b for b, s in on["copies"] if s < T_on]
    assert in_loop and all(b <= 64 for b in in_loop)
    assert len(on["copies"]) <= math.ceil(T_on / CHECK_EVERY) + 2
    d2h = [k for k in on["memcpys"] if "dtoh" in k.lower().replace(" ", "")]
    assert len(d2h) <= math.ceil(T_on / CHECK_EVERY) + 2, d2h


def test_teacher_collection_with_the_eager_recorder_is_unchanged_by_the_switch():
    """The loop's other branch: a teacher of random weights acts, the eager `TactileRecorder` records."""
    import torch

    from locotouch_amd.distill import ReplayBuffer, TactileRecorder
    from locotouch_amd.env import make

    n = N_E2E

    def collect(switch):
        torch.manual_seed(31)
        teacher = torch.nn.Linear(348, 12).to(DEV)
        env = make(STUDENT, num_envs=n, device=DEV, seed=4)
        env.episode_length_buf = torch.randint(440, 500, (n,), device=DEV)
        rb = ReplayBuffer(env, TactileRecorder(DEV, n, 442, 3, 7), 270, check_every=CHECK_EVERY, device_ledger=switch)
        rewards, lengths = rb.collect_data(lambda obs: 0.3 * torch.tanh(teacher(obs)), None, num_steps=500)
        (policy, tactile), _ = rb._materialise()
        return dict(rewards=rewards, lengths=lengths, first=list(rb._traj_first), len=list(rb._traj_len), steps_count=rb._steps_count,
                    sums=rb._reward_sums.clone(), policy=policy.clone(), tactile=tactile.clone())

    same_collection(collect(False), collect(True), 500)


def test_evaluate_is_unchanged_by_the_switch(tmp_path_factory):
    """`evaluate` behind `collect_data`: the sums the collection left are carried in; the env is a fresh twin (module text)."""
    import torch

    from locotouch_amd.distill import DeviceTactileRecorder, ReplayBuffer
    from locotouch_amd.distill.fused_student import FusedStudent
    from locotouch_amd.env import make

    n = N_E2E
    tmp = tmp_path_factory.mktemp("ledger")
    collected = {s: student_collection(tmp, s) for s in (False, True)}
    assert torch.equal(collected[False]["sums"].view(torch.int32), collected[True]["sums"].view(torch.int32)) and collected[True]["sums"].any()

    def evaluate(switch):
        torch.manual_seed(41)
        env = make(STUDENT, num_envs=n, device=DEV, seed=5)
        env.episode_length_buf = torch.randint(440, 500, (n,), device=DEV)
        rb = ReplayBuffer(env, DeviceTactileRecorder(DEV, n, 442, 3, 7), 270, check_every=CHECK_EVERY, device_ledger=switch)
        rb._reward_sums.copy_(collected[switch]["sums"])
        fs = FusedStudent.for_student(collected[switch]["st"])
        assert rb.evaluate(fs, 0) == ([], [])  # (no step is taken)
        rewards, lengths = rb.evaluate(fs, num_trajs=40)
        return rewards, lengths, rb._reward_sums.clone()

    want, got = evaluate(False), evaluate(True)
    assert len(want[0]) >= 40 and bits(got[0]) == bits(want[0]) and got[1] == want[1]
    assert all(type(x) is float for x in got[1])
    assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))
