"""lt_tactile_kernel (csrc/lt_tactile.hip) alone, through lt_env_tactile_update, on planted contact lines: held to the f32 and f64
oracle builds by the judge of tests/tactile_cases.py (continuous channels by the f64 ratio rule, contact bits and levels exactly
outside a capped, reference-derived exclusion set), plus what the whole-env parity runs cannot reach: the aux block offset at
npad != n, the Philox keys at a non-zero env offset and a step counter past 2^32, the untouched rest of the arena, and the entry
point's own contract."""
import numpy as np
import pytest

from tests import tactile_cases as T
from tests.parity_util import device_arena_to_host

pytestmark = pytest.mark.gpu
P, G = "LT_TACTILE_PROCESSED", "LT_TACTILE_ORIGINAL"
SENTINEL = np.float32(-7.5)  # no tactile value: every channel is in [0, 1]
FORMATS = [(P, 3), (G, 3)] + [(f, a) for f, aux in (("LT_TACTILE_BINARY", (0, 2)), ("LT_TACTILE_NORMALIZED", (0, 1)),
                                                    ("LT_TACTILE_DISCRETE", (0, 2)), ("LT_TACTILE_CONTINUOUS", (0, 1))) for a in aux]


def make_env(cfg):
    import torch
    from locotouch_amd.env import LocoTouchVecEnv

    env = LocoTouchVecEnv(cfg=cfg, device="cuda:0")
    torch.cuda.synchronize()
    return env


def device_run(env, cfg, planted):
    """Sentinel into the three tactile blocks (pad rows included), arena to the device, one tactile_update, arena back.  Asserts that
    the launch changed no byte outside the rows it owns and left no sentinel inside them."""
    import torch

    before = planted.copy()
    T.tactile_blocks(cfg, before)[:] = SENTINEL
    env._arena_aligned.copy_(torch.from_numpy(before))
    env.tactile_update()
    torch.cuda.synchronize()
    after = device_arena_to_host(env)
    owned = T.written_mask(cfg)
    blocks = T.tactile_blocks(cfg, after)
    assert (blocks[~owned] == SENTINEL).all(), "wrote outside rows [0, n) of the enabled groups"
    assert (blocks[owned] >= 0).all() and (blocks[owned] <= 1).all(), "left rows unwritten, or values outside [0, 1]"
    rest_a, rest_b = after.copy(), before.copy()
    T.tactile_blocks(cfg, rest_a)[:] = 0
    T.tactile_blocks(cfg, rest_b)[:] = 0
    assert (rest_a == rest_b).all(), "changed bytes outside the tactile blocks"
    return after


def judged_run(env, run, what):
    cfg, planted, o32, o64, thr, groups = T.reference_run(*run)
    cand = device_run(env, cfg, planted)
    res = T.judge(cfg, cand, o32, o64, thr, groups, what=what)
    print("\n".join(res.lines()))
    return cfg, cand


@pytest.mark.parametrize("fmt,aux", FORMATS, ids=[f"{f[11:].lower()}-aux{a}" for f, a in FORMATS])
@pytest.mark.parametrize("params", list(T.PARAM_SETS))
def test_planted_lines_match_oracle(params, fmt, aux):
    """n = 37 (npad 48): the directed lines and 14 random ones, every format and parameter set."""
    run = (37, params, fmt, aux, 0, 1, "mixed")
    judged_run(make_env(T.reference_run(*run)[0]), run, f"kernel n37 {params} {fmt[11:].lower()} aux{aux}")


@pytest.mark.parametrize("n,params,fmt,aux", [(405, "registered", "LT_TACTILE_BINARY", 0), (405, "registered", P, 3), (405, "heavy", P, 3),
                                              (405, "off", G, 3), (1, "alllit", P, 3), (1, "alllit", "LT_TACTILE_NORMALIZED", 0)])
def test_random_lines_match_oracle_at_other_sizes(n, params, fmt, aux):
    """n = 405 (npad 416, the registration's size) on random lines; n = 1 with every taxel lit, where the block minimum is positive
    and the inactive lanes' identity decides it."""
    run = (n, params, fmt, aux, 0, 1, "random")
    cfg, cand = judged_run(make_env(T.reference_run(*run)[0]), run, f"kernel n{n} {params} {fmt[11:].lower()} aux{aux}")
    if params == "alllit":
        assert T.emitted(cfg, cand, 0)["contact"].sum() == n * T.NT


@pytest.mark.parametrize("fmt,aux", [("LT_TACTILE_BINARY", 0), ("LT_TACTILE_CONTINUOUS", 1), ("LT_TACTILE_DISCRETE", 2), (P, 0), (G, 3)])
def test_nothing_else_is_written(fmt, aux):
    """Pad rows [n, npad), disabled groups and, in the two-channel formats, everything past row n's 442 columns keep the sentinel;
    plate samples, counters and policy rows keep their bits (device_run asserts both over the whole arena)."""
    run = (37, "heavy", fmt, aux, 0, 1, "mixed")
    cfg, planted = T.reference_run(*run)[:2]
    after = device_run(make_env(cfg), cfg, planted)
    L = T.layout(cfg)
    blocks = T.tactile_blocks(cfg, after).reshape(3, L.npad * T.WIDE)
    width = L.tactile_dim
    assert (blocks[0, 37 * width:] == SENTINEL).all() and (blocks[0, : 37 * width] != SENTINEL).all()
    for term in (1, 2):
        rows = blocks[term].reshape(L.npad, T.WIDE)
        assert (rows[37:] == SENTINEL).all()
        assert (rows[:37] != SENTINEL).all() if aux & term else (rows[:37] == SENTINEL).all()
    for name in ("LT_F_COUNTERS", "LT_F_OBS_POLICY", "LT_F_OBS_CRITIC"):
        assert (L.arr(after, name) == L.arr(planted, name)).all()
    assert (L.quad(after, "LT_F_PLATE_SAMPLES").view(np.uint32) == L.quad(planted, "LT_F_PLATE_SAMPLES").view(np.uint32)).all()


def group_rows(cfg, arena, rows):
    return [ch[rows] for term in T.terms_of(cfg) for ch in T.emitted(cfg, arena, term).values()]


def test_env_index_offset_enters_the_key():
    """Env e of a 37-env shard at env_index_offset 368 produces the bits of env e + 368 of a 405-env run at offset 0."""
    shard, whole = (37, "heavy", P, 3, 368, 1, "random@368"), (405, "heavy", P, 3, 0, 1, "random")
    cfg_s, out_s = judged_run(make_env(T.reference_run(*shard)[0]), shard, "kernel n37 offset 368")
    cfg_w, out_w = judged_run(make_env(T.reference_run(*whole)[0]), whole, "kernel n405 offset 0")
    for a, b in zip(group_rows(cfg_s, out_s, slice(0, 37)), group_rows(cfg_w, out_w, slice(368, 405))):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_step_counter_enters_the_key_with_all_64_bits():
    """Steps 1, 2 and 2^33 + 7: three different noise draws, each the oracle's; the thresholds, keyed by the startup step, stay (the raw
    `original_tactile` contact map has no other draw in it)."""
    outs = []
    for step in (1, 2, 2 ** 33 + 7):
        run = (37, "heavy", P, 3, 0, step, "mixed")
        cfg, out = judged_run(make_env(T.reference_run(*run)[0]), run, f"kernel n37 step {step}")
        outs.append(out)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for term in (0, 2):
            a, b = T.emitted(cfg, outs[i], term), T.emitted(cfg, outs[j], term)
            assert (a["contact"] != b["contact"]).sum() > 100 and (a["disc"] != b["disc"]).sum() > 100
        a, b = T.emitted(cfg, outs[i], 1), T.emitted(cfg, outs[j], 1)
        assert (a["contact"] == b["contact"]).all() and (a["norm"] == b["norm"]).all() and (a["minmax"] == b["minmax"]).all()
        assert (a["disc"] != b["disc"]).any()  # the level noise is a per-step draw


def test_rows_do_not_depend_on_their_neighbours():
    """The same line and key: last row of 37, alone at n = 1 with the matching offset, and row 36 of 405."""
    runs = [(37, "heavy", P, 3, 0, 1, "random"), (1, "heavy", P, 3, 36, 1, "random@36"), (405, "heavy", P, 3, 0, 1, "random")]
    rows = []
    for run, row in zip(runs, (36, 0, 36)):
        cfg, out = judged_run(make_env(T.reference_run(*run)[0]), run, f"kernel n{run[0]} row {row}")
        rows.append(group_rows(cfg, out, row))
    for other in rows[1:]:
        assert len(other) == len(rows[0]) == 12
        for a, b in zip(rows[0], other):
            assert (a.view(np.uint32) == b.view(np.uint32)).all()


def kernels_of(fn):
    """Names of the device kernels `fn` launches (as tests/test_hip_collect.py counts them)."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return [k for k in dev if "memcpy" not in k.lower() and "memset" not in k.lower()]


def test_tactile_update_entry_point():
    """lt_env_tactile_update: idempotent on an arena, rewrites exactly what an env step left, one kernel per call, and a no-op
    without cfg.tactile_enabled."""
    import torch
    from locotouch_amd.env import LocoTouchVecEnv

    run = (37, "heavy", P, 3, 0, 1, "mixed")
    cfg, planted = T.reference_run(*run)[:2]
    env = make_env(cfg)
    first = device_run(env, cfg, planted)
    env.tactile_update()
    torch.cuda.synchronize()
    assert (device_arena_to_host(env) == first).all()
    kernels = kernels_of(env.tactile_update)
    print("kernels of one tactile_update:", kernels)
    assert len(kernels) == 1 and "lt_tactile_kernel" in kernels[0], kernels
    # after env steps (the cylinder lands within ~12): the rows the step left are what the pass writes again
    env = make_env(T.make_cfg(37, "registered", P, 3))
    for _ in range(24):
        env.step(torch.zeros(37, 12, device="cuda:0"))
    torch.cuda.synchronize()
    left = env._arena_aligned.clone()
    assert float(env.obs_tactile[:, : T.NT].sum()) > 37, "the carried cylinders must light taxels"
    env.tactile_update()
    torch.cuda.synchronize()
    assert torch.equal(env._arena_aligned, left)
    # no tactile sensor: LT_OK, nothing launched, nothing written
    plain = LocoTouchVecEnv("Isaac-RandCylinderTransportTeacher-LocoTouch-v1", num_envs=16, device="cuda:0", seed=3)
    assert plain.cfg.tactile_enabled == 0
    torch.cuda.synchronize()
    left = plain._arena_aligned.clone()
    assert kernels_of(plain.tactile_update) == []
    assert torch.equal(plain._arena_aligned, left)
