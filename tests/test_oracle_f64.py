"""The double-precision oracle build (oracle/_build/liblt_oracle_f64.so, -DLT_REAL=double) against the f32 oracle.

Every parity band in parity_util.TOL was fitted to how far two f32 programs (HIP kernel, f32 oracle) drift apart.  The f64 build
says which of them is closer to the exact answer of the same model: here the f32 oracle, resynced to the same f32 state each
step, must sit inside today's bands around it (tests/test_hip_f64_parity.py then holds the HIP kernel to a multiple of this error)."""
import numpy as np
import pytest

from locotouch_amd import _abi
from locotouch_amd.layout import Layout
from tests import oracle_lib as O
from tests.parity_util import Tally, compare_host_arenas, f64_errors, f64_merge, f64_table

C = _abi.CONSTS
TASKS = {"teacher": "Isaac-RandCylinderTransportTeacher-LocoTouch-v1", "locomotion": "Isaac-Locomotion-LocoTouch-v1",
         "student": "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"}


def test_real_bytes_tell_the_builds_apart():
    assert O.load("f32").lt_oracle_real_bytes() == 4
    assert O.load("f64").lt_oracle_real_bytes() == 8
    assert O.load() is O.load("f32")


@pytest.mark.parametrize("task", list(TASKS))
def test_f32_oracle_within_bands_of_f64_oracle(task):
    """reset_all, then 40 resynced steps (f32 arena copied into the f64 oracle before each step) through resets, pushes and
    contacts: the f32 oracle must pass compare_host_arenas against the f64 oracle with today's allowances."""
    n, steps, pre = 64, 40, 120
    cfg = _abi.preset_cfg(TASKS[task], num_envs=n, seed=11)
    cfg.debug_terms = 1
    o32, o64 = O.OracleEnv(cfg), O.OracleEnv(cfg, precision="f64")
    o32.reset_all()
    o64.reset_all()
    compare_host_arenas(cfg, o32.arena, o64.arena, what=f"reset_all {task} f32 vs f64")
    differs = int((o32.arena != o64.arena).sum())
    L = Layout(n, o32.lib.lt_oracle_obs_dim(o32.cfg), int(cfg.tactile_enabled))
    rng = np.random.default_rng(7)
    for _ in range(pre):  # warm-up on the f32 oracle alone, so the window holds shifted histories, pushes and settled contacts
        o32.step((0.6 * rng.standard_normal((n, 12))).astype(np.float32), nthreads=8)
    push_before = L.vec(o32.arena, "LT_F_EVENT_TIMERS")[:, :2].copy()
    tally, acc, n_reset, n_push, n_contact = Tally(n), {}, 0, 0, 0
    for t in range(steps):
        act = ((0.3 if t < 10 else 1.0) * rng.standard_normal((n, 12))).astype(np.float32)
        if t % 13 == 0:
            act[0, 0] = 400.0  # the +-100 raw clip
        o64.arena[:] = o32.arena
        o32.step(act)
        o64.step(act)
        res = compare_host_arenas(cfg, o32.arena, o64.arena, what=f"{task} step {t} f32 vs f64", max_flip_frac=0.05,
                                  max_event_frac=max(2.0 / n, 1e-3))
        tally.add(res)
        f64_merge(acc, f64_errors(cfg, o32.arena, o64.arena, set(res["flip_envs"]) | set(res["event_envs"])))
        differs += int((o32.arena != o64.arena).sum())
        n_reset += int(L.arr(o32.arena, "LT_F_DONES")[:n].sum())
        timers = L.vec(o32.arena, "LT_F_EVENT_TIMERS")[:, :2]
        n_push += int((timers > push_before).sum())
        push_before = timers.copy()
        n_contact += int((L.vec(o32.arena, "LT_F_FORCE_HIST")[:, 12:16] > 1.0).sum())
    print(tally.line(f"f32 oracle vs f64 oracle, {task}"))
    print(f64_table(f"{task} n={n}: f32 oracle vs f64 oracle", {"o32": acc}))
    assert differs > 0, "the f64 build must really compute in double"
    assert n_reset > 0 and n_push > 0 and n_contact > 0, (n_reset, n_push, n_contact)
    assert tally.flips <= 0.01 * n * steps and tally.events <= max(2, 5e-4 * n * steps), tally.line(task)
    # every continuous field moved by the promotion must also stay strictly inside its band
    assert all(frac < 1.0 for _, _, frac in acc.values()), {k: v for k, v in acc.items() if v[2] >= 1.0}
