"""Every step-kernel instantiation against the double-precision oracle (oracle/_build/liblt_oracle_f64.so).

The parity tests compare two f32 programs, the HIP kernel (CRBA + Schur, contracted FMAs) and the f32 oracle (ABA, no contraction),
inside bands fitted to how far they drift apart.  A kernel that lost precision inside those bands would pass them.  Here one f32
arena goes to the device, the f32 oracle and the f64 oracle each step; both f32 programs must pass today's bands against the f64
answer, and per continuous field the kernel's error may be at most F64_RATIO times the f32 oracle's (plus F64_ULPS f32 ulps of the
field's magnitude), maximum over the steps, outside the envs where either side flipped a thresholded quantity or took an event.

Matrix: one case per instantiation launch_form (locotouch_amd/csrc/lt_env.hip) can pick - task (locomotion, teacher, student) x form
(four-wave: n <= 16 CUs; one-wave: n = 16 (CUs + 1)) x contact-force vectors off / on, the bf16-row kernels of locomotion and teacher
in both forms (state fields only: the rows keep their bf16 check in test_hip_bf16_rows.py), and reset_all per task."""
import numpy as np
import pytest

from locotouch_amd import _abi
from locotouch_amd.layout import Layout
from tests import oracle_lib as O
from tests.parity_util import (F64_RATIO, TOL, Tally, compare_host_arenas, device_arena_to_host, f64_errors, f64_merge,
                               f64_ratio_failures, f64_table)

pytestmark = pytest.mark.gpu
C = _abi.CONSTS
TASKS = {"locomotion": "Isaac-Locomotion-LocoTouch-v1", "teacher": "Isaac-RandCylinderTransportTeacher-LocoTouch-v1",
         "student": "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"}
# Per-field ratio exceptions: measured numbers and a located cause in a comment, capped at 32.  None are needed today.
RATIO_EXCEPTIONS: dict = {}
assert all(r <= 32 for r in RATIO_EXCEPTIONS.values())


def _cus() -> int:
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _n(form: str) -> int:
    return 64 if form == "four" else 16 * (_cus() + 1)


def _make(task, n, **kw):
    import torch
    from locotouch_amd.env import LocoTouchVecEnv

    env = LocoTouchVecEnv(TASKS[task], num_envs=n, device="cuda:0", seed=11, debug_terms=1, **kw)
    torch.cuda.synchronize()
    return env


def _layout(env):
    return Layout(env.num_envs, env.num_obs, int(env.cfg.tactile_enabled))


def _check_ratio(what, e_hip, e_o32, steps):
    print(f64_table(f"{what}: {steps} steps", {"hip": e_hip, "o32": e_o32}))
    bad = f64_ratio_failures(e_hip, e_o32, exceptions=RATIO_EXCEPTIONS)
    assert not bad, f"{what}: the kernel is further from the f64 oracle than {F64_RATIO} x the f32 oracle: " + "; ".join(
        f"{nm} e_hip={ec:.3e} e_o32={eo:.3e} (allowed ratio {r})" for nm, ec, eo, r in bad)


def _fvec_norms_vs_f64(env, o64_arena, L, drop):
    """Newest slot of the world-frame force vectors: |F| == the f64 oracle's |F| history, within the force band."""
    n = env.num_envs
    vec = env.contact_forces_w_history[:, 0].cpu().numpy().astype(np.float64)  # (N, 17, 3) newest sim step
    got = np.linalg.norm(vec, axis=-1)
    fh = L.vec(o64_arena, "LT_F_FORCE_HIST").reshape(n, 3, 16)[:, 0]
    tr = L.vec(o64_arena, "LT_F_TRUNK_FORCE_HIST")[:, :1]
    want = np.concatenate([tr, fh], axis=1).astype(np.float64)
    keep = np.ones(n, bool)
    keep[list(drop)] = False
    atol, rtol = TOL["LT_F_FORCE_HIST"]
    d = np.abs(got - want)[keep]
    assert (d <= atol + rtol * want[keep]).all(), float(d.max())
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("fvec", [False, True], ids=["norms", "fvec"])
@pytest.mark.parametrize("form", ["four", "one"])
@pytest.mark.parametrize("task", list(TASKS))
def test_step_kernel_matches_f64_oracle(task, form, fvec):
    import torch

    n = _n(form)
    env = _make(task, n, contact_force_vectors=fvec)
    o32, o64 = O.OracleEnv(env.cfg), O.OracleEnv(env.cfg, precision="f64")
    o32.reset_all()
    L = _layout(env)
    nth = 16 if n > 1024 else 1
    g = torch.Generator().manual_seed(13)
    for _ in range(40):  # warm-up on the f32 oracle: shifted histories, settled contacts, some envs mid-episode
        o32.step((0.6 * torch.randn(n, 12, generator=g)).numpy(), nthreads=16)
    scale = torch.tensor([0.2, 0.7, 1.5])[torch.arange(n) % 3].unsqueeze(1)  # mixed action scales across envs
    tally, e_hip, e_o32, n_reset, fv_err = Tally(n), {}, {}, 0, 0.0
    steps = 9
    for t in range(steps):
        act = scale * torch.randn(n, 12, generator=g)
        act[t % n, t % 12] = 400.0  # the +-100 raw clip
        if t == 3:  # a caller-requested termination: at least one reset in the window whatever the trajectories do
            L.arr(o32.arena, "LT_F_TERM_BITS")[[0, n - 1]] |= np.int32(1 << C["LT_TERM_REQUEST_BIT"])
        o64.arena[:] = o32.arena
        env._arena_aligned.copy_(torch.from_numpy(o32.arena))
        env.step(act.cuda())
        o32.step(act.numpy(), nthreads=nth)
        o64.step(act.numpy(), nthreads=nth)
        torch.cuda.synchronize()
        hip = device_arena_to_host(env)
        kw = dict(max_flip_frac=0.05, max_event_frac=max(2.0 / n, 1e-3))
        r_hip = compare_host_arenas(env.cfg, hip, o64.arena, what=f"{task} {form} fvec={fvec} step {t} hip vs f64", **kw)
        r_o32 = compare_host_arenas(env.cfg, o32.arena, o64.arena, what=f"{task} {form} step {t} o32 vs f64", **kw)
        tally.add(r_hip)
        drop = set(r_hip["flip_envs"]) | set(r_hip["event_envs"]) | set(r_o32["flip_envs"]) | set(r_o32["event_envs"])
        f64_merge(e_hip, f64_errors(env.cfg, hip, o64.arena, drop))
        f64_merge(e_o32, f64_errors(env.cfg, o32.arena, o64.arena, drop))
        n_reset += int(L.arr(o64.arena, "LT_F_DONES")[:n].sum())
        if fvec:
            fv_err = max(fv_err, _fvec_norms_vs_f64(env, o64.arena, L, drop))
    print(tally.line(f"hip vs f64 oracle, {task} {form}-wave n={n} fvec={fvec}"))
    if fvec:
        print(f"[f64] {task} {form}-wave: newest force-vector norms vs f64 |F| history: max err {fv_err:.3e} N")
    assert n_reset >= 2
    assert tally.events <= max(2, 5e-4 * n * steps), tally.line(task)
    _check_ratio(f"{task} {form}-wave n={n} fvec={fvec}", e_hip, e_o32, steps)


@pytest.mark.parametrize("form", ["four", "one"])
@pytest.mark.parametrize("task", ["locomotion", "teacher"])
def test_bf16_row_kernel_state_matches_f64_oracle(task, form):
    """The bf16-row instantiations (step_rows_raw): state fields only, the rows are held to bf16 rounding elsewhere."""
    import torch

    n = _n(form)
    env = _make(task, n)
    o32, o64 = O.OracleEnv(env.cfg), O.OracleEnv(env.cfg, precision="f64")
    o32.reset_all()
    L = _layout(env)
    g = torch.Generator().manual_seed(17)
    for _ in range(40):
        o32.step((0.6 * torch.randn(n, 12, generator=g)).numpy(), nthreads=16)
    env.set_row_format(torch.bfloat16)
    nxt = [torch.zeros(n, env.num_obs, dtype=torch.bfloat16, device="cuda:0") for _ in range(2)]
    scale = torch.tensor([0.3, 1.2])[torch.arange(n) % 2].unsqueeze(1)
    tally, e_hip, e_o32, n_reset = Tally(n), {}, {}, 0
    steps = 8
    skip = ("LT_F_OBS_POLICY", "LT_F_OBS_CRITIC")
    try:
        for t in range(steps):
            if t == 2:
                L.arr(o32.arena, "LT_F_TERM_BITS")[[1, n - 2]] |= np.int32(1 << C["LT_TERM_REQUEST_BIT"])
            o64.arena[:] = o32.arena
            env._arena_aligned.copy_(torch.from_numpy(o32.arena))
            prev = [torch.from_numpy(L.arr(o32.arena, f)[:n].copy()).cuda().to(torch.bfloat16) for f in skip]
            act = scale * torch.randn(n, 12, generator=g)
            a_dev = act.cuda()
            env.step_rows_raw(a_dev.data_ptr(), prev[0].data_ptr(), prev[1].data_ptr(), nxt[0].data_ptr(), nxt[1].data_ptr())
            o32.step(act.numpy(), nthreads=16 if n > 1024 else 1)
            o64.step(act.numpy(), nthreads=16 if n > 1024 else 1)
            torch.cuda.synchronize()
            hip = device_arena_to_host(env)
            kw = dict(max_flip_frac=0.05, max_event_frac=max(2.0 / n, 1e-3), skip=skip)
            r_hip = compare_host_arenas(env.cfg, hip, o64.arena, what=f"bf16 {task} {form} step {t} hip vs f64", **kw)
            r_o32 = compare_host_arenas(env.cfg, o32.arena, o64.arena, what=f"bf16 {task} {form} step {t} o32 vs f64", **kw)
            tally.add(r_hip)
            drop = set(r_hip["flip_envs"]) | set(r_hip["event_envs"]) | set(r_o32["flip_envs"]) | set(r_o32["event_envs"])
            for acc, arena in ((e_hip, hip), (e_o32, o32.arena)):
                errs = f64_errors(env.cfg, arena, o64.arena, drop)
                f64_merge(acc, {k: v for k, v in errs.items() if k not in skip})
            n_reset += int(L.arr(o64.arena, "LT_F_DONES")[:n].sum())
    finally:
        env.set_row_format(torch.float32)
    print(tally.line(f"bf16 rows hip vs f64 oracle, {task} {form}-wave n={n}"))
    assert n_reset >= 2
    _check_ratio(f"bf16 rows {task} {form}-wave n={n}", e_hip, e_o32, steps)


@pytest.mark.parametrize("task", list(TASKS))
def test_reset_all_matches_f64_oracle(task):
    n = 64
    env = _make(task, n)
    o32, o64 = O.OracleEnv(env.cfg), O.OracleEnv(env.cfg, precision="f64")
    o32.reset_all()
    o64.reset_all()
    hip = device_arena_to_host(env)
    r_hip = compare_host_arenas(env.cfg, hip, o64.arena, what=f"reset_all {task} hip vs f64")
    r_o32 = compare_host_arenas(env.cfg, o32.arena, o64.arena, what=f"reset_all {task} o32 vs f64")
    drop = set(r_hip["flip_envs"]) | set(r_hip["event_envs"]) | set(r_o32["flip_envs"]) | set(r_o32["event_envs"])
    _check_ratio(f"reset_all {task}", f64_errors(env.cfg, hip, o64.arena, drop), f64_errors(env.cfg, o32.arena, o64.arena, drop), 0)

