"""The tactile delay line and the step recording in HIP kernels (csrc/lt_collect.hip behind include/lt_collect.h,
locotouch_amd/distill/device_recorder.py) on the GPU, against the eager `TactileRecorder` (which tests/golden/distill.npz pins to the
reference).  The kernels only move rows, so EVERY comparison here is `torch.equal`: there is no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STUDENT = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"
DEV = "cuda:0"
T = 40
ALL = "all"  # reset(None)


def schedule(n, seed):
    """Reset masks in front of every step's record: step 0 all envs (the None form), step 5 no env, step 9 every env (as a mask), env 0
    alone on the consecutive steps 12 and 13, else random envs (from a generator of their own: the global one only draws delays)."""
    import torch

    g = torch.Generator().manual_seed(seed)
    masks = [(torch.rand(n, generator=g) < 0.15).to(DEV) for _ in range(T)]
    masks[0] = ALL
    masks[5] = torch.zeros(n, dtype=torch.bool, device=DEV)
    masks[9] = torch.ones(n, dtype=torch.bool, device=DEV)
    for t in (12, 13):
        masks[t] = torch.zeros(n, dtype=torch.bool, device=DEV)
        masks[t][0] = True
    return masks


def random_rows(steps, n, d, seed):
    import torch

    return torch.randn(steps, n, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def run(cls, n, d, lo, hi, rows, masks, seed=7):
    """The call sequence of the loops: reset, record, get.  Every step's delayed rows and the final delays."""
    import torch

    torch.manual_seed(seed)
    rec = cls(DEV, n, d, lo, hi)
    outs = []
    for t in range(len(rows)):
        if masks[t] is ALL:
            rec.reset()
        elif masks[t] is not None:
            rec.reset(masks[t])
        rec.record_new_tactile_signals(rows[t])
        outs.append(rec.get_tactile_signals().clone())
    return outs, rec.delay_steps.clone(), rec


# 442: the 8-byte path; 5 and 1: the dword path; 8: the 16-byte path; depth 1: the read always takes the row just pushed; depth 2 and 3
# wrap within the run
@pytest.mark.parametrize("n, d, lo, hi", [(1, 442, 3, 7), (37, 442, 3, 7), (405, 442, 3, 7), (37, 5, 0, 1), (37, 8, 1, 2), (64, 1, 0, 3)])
def test_twin_run_is_bit_exact(n, d, lo, hi):
    import torch

    from locotouch_amd.distill import DeviceTactileRecorder, TactileRecorder

    rows, masks = random_rows(T, n, d, seed=n + d), schedule(n, seed=hi)
    want, want_delay, _ = run(TactileRecorder, n, d, lo, hi, rows, masks)
    got, got_delay, _ = run(DeviceTactileRecorder, n, d, lo, hi, rows, masks)
    assert got_delay.dtype == want_delay.dtype and torch.equal(got_delay, want_delay)
    for t in range(T):
        assert got[t].shape == want[t].shape and torch.equal(got[t], want[t]), t
    assert any(not torch.equal(want[t], rows[t]) for t in range(T)) or hi == 1  # (the delay line did delay something)


def test_call_form_corners():
    import torch

    from locotouch_amd.distill import DeviceTactileRecorder, TactileRecorder

    n, d = 37, 442
    rows = random_rows(8, n, d, seed=1)
    m1 = torch.zeros(n, dtype=torch.bool, device=DEV)
    m1[::3] = True
    m2 = torch.zeros(n, dtype=torch.bool, device=DEV)
    m2[::2] = True
    seen = {}
    for cls in (TactileRecorder, DeviceTactileRecorder):
        torch.manual_seed(3)
        rec = cls(DEV, n, d, 3, 7)
        fresh = rec.get_tactile_signals().clone()               # nothing recorded yet
        for t in range(3):
            rec.record_new_tactile_signals(rows[t])
        rec.reset(m1)
        after_reset = rec.get_tactile_signals().clone()         # between a reset and the next record: zeros for the reset envs
        rec.reset(m2)                                           # two resets, no push between: the last reset that names an env holds
        delays = rec.delay_steps.clone()
        outs = []
        for t in range(3, 8):
            rec.record_new_tactile_signals(rows[t])
            outs.append(rec.get_tactile_signals().clone())
        seen[cls] = (fresh, after_reset, delays, outs, rec.delay_steps.clone())
    want, got = seen[TactileRecorder], seen[DeviceTactileRecorder]
    assert torch.equal(got[0], torch.zeros(n, d, device=DEV)) and torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1]) and not got[1][m1].any() and got[1][~m1].any()
    assert torch.equal(got[2], want[2]) and torch.equal(got[4], want[4])
    for a, b in zip(got[3], want[3]):
        assert torch.equal(a, b)
    # an index tensor is the bool mask
    state = []
    for form in (m1, m1.nonzero().flatten()):
        torch.manual_seed(4)
        rec = DeviceTactileRecorder(DEV, n, d, 3, 7)
        rec.record_new_tactile_signals(rows[0])
        rec.reset(form)
        state.append((rec._state.clone(), rec.get_tactile_signals().clone()))
    assert torch.equal(state[0][0], state[1][0]) and torch.equal(state[0][1], state[1][1])


# rows 8 bytes aligned (the 8-byte path), 4 bytes (the dword path), 16 bytes (still the 8-byte path: 442 is no multiple of 4); the 348-wide
# copy pair is 16-byte aligned throughout: its 16-byte path
@pytest.mark.parametrize("off", [2, 1, 4])
def test_strided_operands_and_three_destinations(off):
    import torch

    from locotouch_amd.distill import DeviceTactileRecorder, TactileRecorder

    n, d, S = 37, 442, 12345.0
    wide = torch.full((n, 1000), S, device=DEV)                 # the env's rows: the tactile columns at an offset, row stride 1000
    view = wide[:, off:off + d]
    assert view.stride(0) == 1000 and view.data_ptr() % 16 == (4 * off) % 16
    out0 = torch.full((n, d), S, device=DEV)
    store = torch.full((n, 900), S, device=DEV)                 # the step store's slot inside wider rows
    out1 = store[:, 6:6 + d]
    src_wide, dst_wide = torch.full((n, 400), S, device=DEV), torch.full((n, 360), S, device=DEV)
    src, dst = src_wide[:, 4:352], dst_wide[:, 8:356]           # the 348-wide policy rows
    rows = random_rows(12, n, d, seed=2)
    pol = random_rows(12, n, 348, seed=3)
    masks = schedule(n, seed=5)[:12]
    torch.manual_seed(6)
    eager, want = TactileRecorder(DEV, n, d, 3, 7), []
    for t in range(12):                                         # (one pass each: both draw their delays from the global generator)
        eager.reset() if masks[t] is ALL else eager.reset(masks[t])
        eager.record_new_tactile_signals(rows[t])
        want.append(eager.get_tactile_signals().clone())
    torch.manual_seed(6)
    rec = DeviceTactileRecorder(DEV, n, d, 3, 7)
    for t in range(12):
        rec.reset() if masks[t] is ALL else rec.reset(masks[t])
        view.copy_(rows[t])
        src.copy_(pol[t])
        assert rec.push(view, out0, store=out1, copy=(src, dst)) is out0
        assert torch.equal(out0, want[t]), t
        assert torch.equal(out1, want[t]), t
        assert torch.equal(dst, pol[t]), t
        assert torch.equal(view, rows[t]) and torch.equal(src, pol[t])                           # inputs are only read
    assert any(not torch.equal(want[t], rows[t]) for t in range(12))
    for buf, lo, hi in ((wide, off, off + d), (store, 6, 6 + d), (src_wide, 4, 352), (dst_wide, 8, 356)):
        assert (buf[:, :lo] == S).all() and (buf[:, hi:] == S).all()                             # the bytes around the slices
    with pytest.raises(RuntimeError, match="out0"):
        rec.push(view, view)
    with pytest.raises(ValueError, match="unit column stride"):
        rec.push(wide[:, 0:2 * d:2], out0)


def test_row_independence_and_the_large_case():
    """Env 36's history gives the same delayed rows last in a 37-env recorder, alone, and at rows 36 and 4111 of a 4112-env recorder
    (4112 x 442 x 7: a 51 MB ring); the 4112-env run also equals the eager class row for row."""
    import torch

    from locotouch_amd import _abi
    from locotouch_amd.distill import DeviceTactileRecorder, TactileRecorder

    N, d, steps = 4112, 442, 12
    rows = random_rows(steps, N, d, seed=8)
    rows[:, N - 1] = rows[:, 36]
    g = torch.Generator().manual_seed(9)
    fresh = [torch.randint(3, 7, (N,), generator=g).to(DEV) for _ in range(steps)]
    masks = [(torch.rand(N, generator=g) < 0.2).to(DEV) for _ in range(steps)]
    masks[0][:] = True
    for t in range(steps):
        fresh[t][N - 1], masks[t][N - 1] = fresh[t][36], masks[t][36]

    def reset_with(rec, mask, delays):  # the delays of the draw are the caller's here: lt_delay_reset itself
        _abi.call("lt_delay_reset", rec._state, rec.env_num, rec.dim, rec.depth, mask.contiguous(), delays.contiguous(), _abi.stream(DEV))

    def history(idx):
        rec = DeviceTactileRecorder(DEV, len(idx), d, 3, 7)
        outs = []
        for t in range(steps):
            reset_with(rec, masks[t][idx], fresh[t][idx])
            outs.append(rec.push(rows[t][idx], torch.empty(len(idx), d, device=DEV)))
        return torch.stack(outs), rec

    every = torch.arange(N, device=DEV)
    big, rec_big = history(every)
    small, _ = history(every[:37])
    alone, _ = history(every[36:37])
    assert torch.equal(small[:, 36], big[:, 36]) and torch.equal(alone[:, 0], big[:, 36]) and torch.equal(big[:, N - 1], big[:, 36])
    eager = TactileRecorder(DEV, N, d, 3, 7)
    for t in range(steps):
        eager.reset(masks[t])
        eager.delay_steps = torch.where(masks[t], fresh[t], eager.delay_steps)
        eager.record_new_tactile_signals(rows[t])
        assert torch.equal(big[t], eager.get_tactile_signals()), t
    assert torch.equal(rec_big.delay_steps, eager.delay_steps)


@pytest.mark.parametrize("mask_dtype", ["bool", "uint8"])
def test_after_step(mask_dtype):
    import torch

    from locotouch_amd import _abi
    from locotouch_amd.distill import DeviceTactileRecorder, TactileRecorder

    n, d = 405, 442
    g = torch.Generator(device=DEV).manual_seed(10)
    rows = random_rows(10, n, d, seed=11)
    dones = torch.randint(0, 3, (n,), device=DEV, generator=g)  # int64: 0, 1 and 2
    reward = torch.randn(n, device=DEV, generator=g)
    assert dones.dtype == torch.int64 and set(dones.unique().tolist()) == {0, 1, 2}
    done_mask = dones != 0
    recs = {}
    for cls in (TactileRecorder, DeviceTactileRecorder):
        torch.manual_seed(12)
        recs[cls] = rec = cls(DEV, n, d, 3, 7)
        for t in range(5):
            rec.record_new_tactile_signals(rows[t])
    eager, rec = recs[TactileRecorder], recs[DeviceTactileRecorder]
    reward_out = torch.full((n,), -7.0, device=DEV)
    done_out = torch.zeros(n, dtype=getattr(torch, mask_dtype), device=DEV)
    torch.manual_seed(13)
    eager.reset(done_mask)
    torch.manual_seed(13)
    rec.after_step(reward, dones, reward_out, done_out)
    assert torch.equal(reward_out, reward) and torch.equal(done_out.bool(), done_mask) and int(done_out.to(torch.uint8).max()) == 1
    assert torch.equal(rec.delay_steps, eager.delay_steps)
    assert torch.equal(rec._ints[1] == 0, done_mask)            # count = 0 exactly for the finished envs
    assert torch.equal(rec.get_tactile_signals(), eager.get_tactile_signals())
    for t in range(5, 10):                                      # ... and the state behaves as the eager one from here on
        eager.record_new_tactile_signals(rows[t]), rec.record_new_tactile_signals(rows[t])
        assert torch.equal(rec.get_tactile_signals(), eager.get_tactile_signals()), t
    # state = NULL: the two copies alone
    before = rec._state.clone()
    reward_out.fill_(-7.0), done_out.zero_()
    _abi.call("lt_collect_after_step", None, n, 0, 0, reward, dones, None, reward_out, done_out, _abi.stream(DEV))
    assert torch.equal(reward_out, reward) and torch.equal(done_out.bool(), done_mask) and torch.equal(rec._state, before)


def short(names):
    return [k.split("<")[0].split("(anonymous namespace)::")[-1].replace("void at::native::", "")[:48] for k in names]


def kernels_of(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return [k for k in dev if "memcpy" not in k.lower() and "memset" not in k.lower()], [k for k in dev if "memcpy" in k.lower() or "memset" in k.lower()]


def test_launch_count():
    import torch

    from locotouch_amd.distill import DeviceTactileRecorder, TactileRecorder

    n, d = 405, 442
    rec = DeviceTactileRecorder(DEV, n, d, 3, 7)
    rows, pol = random_rows(1, n, d, seed=14)[0], random_rows(1, n, 348, seed=15)[0]
    out, store, pol_store = torch.empty(n, d, device=DEV), torch.empty(n, d, device=DEV), torch.empty(n, 348, device=DEV)
    reward, dones = torch.randn(n, device=DEV), torch.randint(0, 2, (n,), device=DEV)
    reward_out, done_out = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV)
    for _ in range(3):                                          # warm
        rec.push(rows, out, store=store, copy=(pol, pol_store))
        rec.after_step(reward, dones, reward_out, done_out)
    kernels, copies = kernels_of(lambda: rec.push(rows, out, store=store, copy=(pol, pol_store)))
    print("kernels of one push:", short(kernels))
    assert len(kernels) == 1 and ("lt_delay" in kernels[0] or "lt_collect" in kernels[0]) and not copies, (kernels, copies)
    kernels, copies = kernels_of(lambda: rec.after_step(reward, dones, reward_out, done_out))
    print("kernels of one after_step:", short(kernels))
    ours = [k for k in kernels if "lt_delay" in k or "lt_collect" in k]
    assert len(kernels) == 2 and len(ours) == 1 and not copies, (kernels, copies)               # + the one randint kernel
    # what the same work costs on the eager path (reported, and only bounded from below: it is the library's business)
    eager = TactileRecorder(DEV, n, d, 3, 7)

    def eager_step():
        pol_store.copy_(pol)
        eager.record_new_tactile_signals(rows)
        store.copy_(eager.get_tactile_signals())
        reward_out.copy_(reward)
        m = dones != 0
        done_out.copy_(m)
        eager.reset(m)

    for _ in range(3):
        eager_step()
    kernels, copies = kernels_of(eager_step)
    print(f"eager recording of one step: {len(kernels)} kernels + {len(copies)} copy nodes:", short(kernels + copies))
    assert len(kernels) + len(copies) > 3


def make_student(tmp, seed=5):
    import torch

    from locotouch_amd.distill import Student, distillation_cfg

    cfg = distillation_cfg(STUDENT)
    cfg.device, cfg.log_dir = DEV, str(tmp)
    torch.manual_seed(seed)
    return Student(cfg, 270, 442, 12, verbose=False).eval()


def test_collection_is_unchanged_by_the_switch(tmp_path):
    """Two student envs from the same seed, the same student through `FusedStudent` on both sides, the same generator state in front of
    `collect_data`: the eager and the device recorder collect the same bits."""
    import torch

    from locotouch_amd.distill import DeviceTactileRecorder, ReplayBuffer, TactileRecorder
    from locotouch_amd.distill.fused_student import FusedStudent
    from locotouch_amd.env import make

    n = 405
    st = make_student(tmp_path)
    teacher = lambda obs: 0.1 * obs[..., :12]  # noqa: E731  (not called: the student acts)

    def collect(cls):
        torch.manual_seed(21)
        env = make(STUDENT, num_envs=n, device=DEV, seed=3)
        env.episode_length_buf = torch.randint(440, 500, (n,), device=DEV)  # episodes end inside the run
        rb = ReplayBuffer(env, cls(DEV, n, 442, 3, 7), 270)
        fs = FusedStudent.for_student(st)
        torch.manual_seed(22)
        rewards, lengths = rb.collect_data(teacher, fs, num_steps=3000)
        (policy, tactile), _ = rb._materialise()
        np.random.seed(23)
        batch = next(rb.to_recurrent_generator(8))
        return rewards, lengths, rb.num_trajs, rb.num_steps, policy.clone(), tactile.clone(), batch

    want, got = collect(TactileRecorder), collect(DeviceTactileRecorder)
    assert want[2] > 0 and want[3] >= 3000
    assert got[0] == want[0] and got[1] == want[1] and got[2:4] == want[2:4]
    assert torch.equal(got[4], want[4]) and torch.equal(got[5], want[5])
    assert set(got[6]) == set(want[6])
    for k in want[6]:
        assert torch.equal(got[6][k], want[6][k]), k


def test_distillation_with_fused_collection_end_to_end(tmp_path):
    import os

    import torch

    from locotouch_amd.agents import train_cfg
    from locotouch_amd.distill import DeviceTactileRecorder, Distillation, TactileRecorder, distillation_cfg
    from locotouch_amd.distill.fused_student import FusedStudent
    from locotouch_amd.env import make
    from locotouch_amd.rl import OnPolicyRunner

    torch.manual_seed(0)
    env = make(STUDENT, num_envs=405, device=DEV, seed=3)
    runner = OnPolicyRunner(env, train_cfg(STUDENT), log_dir=None, device=DEV)
    teacher = runner.get_inference_policy(device=DEV)

    def cfg_for(sub):
        cfg = distillation_cfg(STUDENT)
        cfg.logger, cfg.log_root_path = "tensorboard", str(tmp_path / sub)
        cfg.num_iterations, cfg.bc_data_steps, cfg.dagger_data_steps = 2, 3000, 2000
        cfg.initial_epoches, cfg.incremental_epoches, cfg.batch_steps, cfg.evaluation_trajs_num = 2, 1, 1500, 16
        return cfg

    plain = Distillation(env, cfg_for("plain"), teacher_policy=teacher, verbose=False)
    assert type(plain.tactile_recorder) is TactileRecorder                                         # the default is the eager class
    d = Distillation(env, cfg_for("fused"), teacher_policy=teacher, verbose=False, fused_student_inference=True, fused_collection=True)
    assert isinstance(d.tactile_recorder, DeviceTactileRecorder) and isinstance(d.fused_student, FusedStudent)
    assert d.replay_buffer._tactile_recorder is d.tactile_recorder
    hist = d.train()
    assert [h["iter"] for h in hist] == [0, 1, "eval"]
    for h in hist:
        assert all(np.isfinite(v) for k, v in h.items() if k != "iter"), h
    assert hist[1]["collect/trj_num"] > 0 and hist[2]["collect/trj_num"] >= 16
    ckpt = os.path.join(d.student.log_dir, "model_1.pt")
    assert os.path.exists(ckpt)
    actions = []
    for switch in (False, True):                                # twins: the same seed, env seed and checkpoint
        torch.manual_seed(31)
        env_p = make(STUDENT, num_envs=405, device=DEV, seed=4)
        p = Distillation(env_p, cfg_for(f"play{int(switch)}"), training=False, checkpoint=ckpt, verbose=False, fused_student_inference=True,
                         fused_collection=switch)
        assert isinstance(p.tactile_recorder, DeviceTactileRecorder) == switch
        actions.append(p.play(num_steps=8).clone())
    assert actions[0].shape == (405, 12) and torch.isfinite(actions[0]).all() and torch.equal(actions[0], actions[1])
