"""Pin the RNG-consuming terms of the oracle to the reference: tests/golden/mdp_replay.npz holds (per-env uniforms -> outputs)
recorded while REPLAYING those uniforms through the reference's own functions (tools/gen_golden_replay.py); the oracle's
explicit-uniform entry points - which its step path calls with Philox uniforms - must reproduce the outputs from the same
uniforms with lt_cfg_default's parameters.  CPU only.

  C4 commands.py:517-559   E3 events.py:160-196   E6 events.py:85-109   O1 (noise) observations.py:71-83
  K10 observations.py:121-126,154-184,281-308 (BinaryTactileSignals of the student task)
"""
import ctypes
import os

import numpy as np
import pytest

from locotouch_amd import _abi
from tests import oracle_lib as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mdp_replay.npz")
C = _abi.CONSTS
f32 = ctypes.c_float


def _cfg():
    return _abi.default_cfg(C["LT_TASK_TRANSPORT_TEACHER"], num_envs=16)


def _arr(vals):
    return (f32 * len(vals))(*[float(v) for v in vals])


def test_command_resample_matches_reference_replay(precision="f32"):
    """Bin selection by inverse CDF over (p, 1 - 2p, p), per-bin ranges [new_lo, old_lo], [old_lo, old_hi], [old_hi, new_hi],
    the equal-range shortcut, the standing draw (<=) and the buffer copy."""
    g = np.load(GOLD)
    lib, cfg = O.load(precision), _cfg()
    assert abs(cfg.cmd_new_probs - float(g["cmd_new_probs"])) < 1e-7
    S, n = g["cmd_ub"].shape[:2]
    seen_bins = set()
    for s in range(S):
        P = np.zeros(C["LT_CMD_PARAMS_LEN"], np.float32)
        P[0:6] = g["cmd_ranges"][s].reshape(-1)
        P[6:12] = g["cmd_prev_ranges"][s].reshape(-1)
        P[12:15] = g["cmd_equal"][s].astype(np.float32)
        P[15] = float(g["cmd_zero_steps"][s])
        P[16] = float(g["cmd_rel_standing"][s])
        for e in range(n):
            cmd, buf = (f32 * 3)(), (f32 * 3)()
            standing, tleft = f32(), f32()
            ub, uv = g["cmd_ub"][s, e], g["cmd_uv"][s, e]
            lib.lt_oracle_command_resample_u(ctypes.byref(cfg), O.fptr(P), _arr(ub), _arr(uv), float(g["cmd_ustand"][s, e]), 0.5,
                                             cmd, buf, ctypes.byref(standing), ctypes.byref(tleft))
            np.testing.assert_allclose(np.array(buf[:]), g["cmd_out_buffer"][s, e], rtol=0, atol=2e-7, err_msg=f"scenario {s} env {e}")
            assert bool(standing.value) == bool(g["cmd_out_standing"][s, e]), (s, e)
            # _resample_command ends with the zero-command window (commands.py:559): cmd = buffer, or 0 inside the window
            exp = np.array(buf[:]) * (0.0 if g["cmd_ep_len"][s, e] < g["cmd_zero_steps"][s] else 1.0)
            np.testing.assert_allclose(exp, g["cmd_out_cmd"][s, e], rtol=0, atol=2e-7)
            if not g["cmd_equal"][s].all():
                for d in range(3):
                    if not g["cmd_equal"][s, d]:
                        seen_bins.add(int(ub[d] >= cfg.cmd_new_probs) + int(ub[d] >= 1.0 - cfg.cmd_new_probs))
    assert seen_bins == {0, 1, 2}


def test_trunk_material_matches_reference_replay(precision="f32"):
    g = np.load(GOLD)
    lib, cfg = O.load(precision), _cfg()
    # lt_cfg_default carries the reference's resolved ranges (rand_cylinder cfg :56 overrides the static range)
    np.testing.assert_allclose(np.array(cfg.trunk_friction[:]), g["mat_ranges"][0], atol=1e-7)
    np.testing.assert_allclose(np.array(cfg.trunk_restitution[:]), g["mat_ranges"][2], atol=1e-7)
    for e in range(g["mat_u"].shape[0]):
        out = (f32 * 3)()
        lib.lt_oracle_material_u(_arr(cfg.trunk_friction[:]), _arr(g["mat_ranges"][1]), _arr(cfg.trunk_restitution[:]), _arr(g["mat_u"][e]), out)
        np.testing.assert_allclose(np.array(out[:]), g["mat_out"][e], rtol=0, atol=1e-7)
    assert (g["mat_out"][:, 1] <= g["mat_out"][:, 0]).all()  # make_consistent


def test_reset_object_state_matches_reference_replay(precision="f32"):
    """World-axis offset, + cylinder height / 2, orientation = robot quat (x) euler, velocity = robot root velocity."""
    g = np.load(GOLD)
    lib, cfg = O.load(precision), _cfg()
    pr = g["obj_pose_range"]
    for i in range(3):
        np.testing.assert_allclose(np.array(cfg.obj_reset_pos[i][:]), pr[i], atol=1e-7)
        np.testing.assert_allclose(np.array(cfg.obj_reset_rpy[i][:]), pr[3 + i], atol=1e-6)
    for e in range(g["obj_u_pose"].shape[0]):
        rs = g["obj_root_state"][e].astype(np.float32)
        pos, quat, lin, ang = (f32 * 3)(), (f32 * 4)(), (f32 * 3)(), (f32 * 3)()
        lib.lt_oracle_reset_object_u(ctypes.byref(cfg), _arr(rs[0:3]), _arr(rs[3:7]), _arr(rs[7:10]), _arr(rs[10:13]),
                                     float(g["obj_height"][e]), _arr(g["obj_u_pose"][e]), pos, quat, lin, ang)
        np.testing.assert_allclose(np.array(pos[:]), g["obj_out_pose"][e, 0:3], rtol=0, atol=2e-6)
        np.testing.assert_allclose(np.array(quat[:]), g["obj_out_pose"][e, 3:7], rtol=0, atol=2e-6)
        np.testing.assert_allclose(np.array(lin[:] + ang[:]), g["obj_out_vel"][e], rtol=0, atol=1e-7)


def test_noisy_object_state_observation_matches_reference_replay(precision="f32"):
    """Additive noise on position / velocities, euler noise right-multiplied onto the quaternion, the second draw for envs
    that have not touched the plate yet, then the per-component scale."""
    g = np.load(GOLD)
    lib, cfg = O.load(precision), _cfg()
    nmin, nmax = g["osn_n_min"], g["osn_n_max"]
    np.testing.assert_allclose(-nmin, nmax)
    np.testing.assert_allclose(np.array(cfg.obj_noise[:12]), nmax, atol=1e-7)
    np.testing.assert_allclose(np.array(cfg.obj_scale[:]), g["osn_scale"], atol=1e-7)
    T, n = g["osn_out"].shape[:2]
    n_noncontact = 0
    for t in range(T):
        for e in range(n):
            ti = O.TermIn()
            r, o = g["osn_robot_root_state"][t, e], g["osn_obj_root_state"][t, e]
            ti.root_pos[:], ti.root_quat[:], ti.root_lin[:], ti.root_ang[:] = r[0:3], r[3:7], r[7:10], r[10:13]
            ti.obj_pos[:], ti.obj_quat[:], ti.obj_lin[:], ti.obj_ang[:] = o[0:3], o[3:7], o[7:10], o[10:13]
            ti.obj_timers[1] = g["osn_obj_cur_contact"][t, e]
            ti.obj_timers[3] = g["osn_obj_last_contact"][t, e]
            n_noncontact += int(ti.obj_timers[1] < 1e-8 and ti.obj_timers[3] < 1e-8)
            out = (f32 * 13)()
            lib.lt_oracle_object_state_obs(ctypes.byref(cfg), ctypes.byref(ti), _arr(g["osn_u16"][t, e]), out)
            np.testing.assert_allclose(np.array(out[:]), g["osn_out"][t, e], rtol=2e-5, atol=3e-6, err_msg=f"t {t} env {e}")
    assert 0 < n_noncontact < T * n


def test_binary_tactile_matches_reference_replay(precision="f32"):
    """Thresholds (+ per-taxel offset drawn once), contact map, dropout THEN addition (a dropped taxel can be re-added), two
    identical channels - with the student preset's parameters, which the golden's resolved term params pin."""
    g = np.load(GOLD)
    lib = O.load(precision)
    cfg = _abi.preset_cfg("Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1", num_envs=16)
    thr, nmin, nmax, pdrop, padd = g["tac_params"]
    assert abs(cfg.tactile_threshold - thr) < 1e-7 and abs(cfg.tactile_threshold_noise - nmax) < 1e-7 and abs(nmin + nmax) < 1e-12
    assert abs(cfg.tactile_dropout_prob - pdrop) < 1e-9 and abs(cfg.tactile_addition_prob - padd) < 1e-9
    T, n, nt = g["tac_forces_local"].shape
    assert nt == C["LT_TACTILE_ROWS"] * C["LT_TACTILE_COLS"] and 2 * nt == C["LT_TACTILE_DIM"]
    dropped = added = readded = 0
    for t in range(T):
        for e in range(n):
            f = np.ascontiguousarray(g["tac_forces_local"][t, e], np.float32)
            ut = np.ascontiguousarray(g["tac_u_thr"][e], np.float32)
            ud = np.ascontiguousarray(g["tac_u_drop"][t, e], np.float32)
            ua = np.ascontiguousarray(g["tac_u_add"][t, e], np.float32)
            out = np.zeros(2 * nt, np.float32)
            lib.lt_oracle_tactile_signals_u(ctypes.byref(cfg), O.fptr(f), O.fptr(ut), O.fptr(ud), O.fptr(ua), O.fptr(out))
            assert np.array_equal(out, g["tac_out"][t, e]), (t, e, np.nonzero(out != g["tac_out"][t, e]))
            raw = f > np.float32(thr) + (ut * np.float32(nmax - nmin) + np.float32(nmin))
            dropped += int((raw & (ud < pdrop)).sum())
            added += int((~raw & (ua < padd)).sum())
            readded += int((raw & (ud < pdrop) & (ua < padd)).sum())
    assert dropped >= 5 and added >= 20  # the vectors exercise both corruption branches


FORMATS = {"binary": "LT_TACTILE_BINARY", "normalized": "LT_TACTILE_NORMALIZED", "discrete": "LT_TACTILE_DISCRETE",
           "continuous": "LT_TACTILE_CONTINUOUS", "processed": "LT_TACTILE_PROCESSED", "original": "LT_TACTILE_ORIGINAL"}


def tactile_cfg_for(g, pi, num_envs=16, play=False):
    """Student preset with parameter set `pi` of the golden (0: the registered cfg, 1: dropout / addition raised to 8 %, 2: the
    Denoised variants - no threshold / force / level noise).  Set 0 must BE the preset."""
    task = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-" + ("Play-v1" if play else "v1")
    cfg = _abi.preset_cfg(task, num_envs=num_envs)
    thr, tn, pdrop, padd, fn, fmax, levels, ln = g["tf_params"][pi]
    if pi == 0:
        got = [cfg.tactile_threshold, cfg.tactile_threshold_noise, cfg.tactile_dropout_prob, cfg.tactile_addition_prob, cfg.tactile_force_noise,
               cfg.tactile_maximal_force, cfg.tactile_total_levels, cfg.tactile_level_noise]
        np.testing.assert_allclose(got, g["tf_params"][0], rtol=1e-6)
    cfg.tactile_threshold, cfg.tactile_threshold_noise, cfg.tactile_dropout_prob, cfg.tactile_addition_prob = thr, tn, pdrop, padd
    cfg.tactile_force_noise, cfg.tactile_maximal_force, cfg.tactile_total_levels, cfg.tactile_level_noise = fn, fmax, int(levels), ln
    return cfg


@pytest.mark.parametrize("pi", [0, 1, 2])
@pytest.mark.parametrize("cname", list(FORMATS))
def test_every_tactile_signals_class_matches_reference_replay(pi, cname, precision="f32"):
    """O6: TactileSignals / Binary / Normalized / Discrete / Cotinuous / Processed (observations.py:248-429) on replayed uniforms:
    contact maps exact, force channels to f32 rounding (a discretisation level is 0.2: a flipped level would fail)."""
    g = np.load(GOLD)
    lib = O.load(precision)
    cfg = tactile_cfg_for(g, pi)
    fmt = C[FORMATS[cname]]
    pre = f"tf_{pi}_{cname}_"
    T, n, nt = g[pre + "forces"].shape
    width = g[pre + "out"].shape[-1]
    assert width == (4 * nt if cname in ("processed", "original") else 2 * nt)
    PF = ctypes.POINTER(ctypes.c_float)
    stats = dict(contact=0, dropped=0, added=0, levels=set())
    for t in range(T):
        for e in range(n):
            f = np.ascontiguousarray(g[pre + "forces"][t, e], np.float32)
            us = [np.ascontiguousarray(g[pre + "u_thr"][e], np.float32)] + [np.ascontiguousarray(g[pre + "u"][t, k, e], np.float32) for k in range(7)]
            u8 = (PF * 8)(*[O.fptr(u) for u in us])
            out = np.zeros(width, np.float32)
            lib.lt_oracle_tactile_format_u(ctypes.byref(cfg), fmt, O.fptr(f), u8, O.fptr(out))
            ref = g[pre + "out"][t, e]
            assert np.array_equal(out[:nt], ref[:nt]), (t, e, np.nonzero(out[:nt] != ref[:nt]))
            np.testing.assert_allclose(out[nt:], ref[nt:], rtol=2e-6, atol=2e-7, err_msg=f"{cname} set {pi} t {t} env {e}")
            stats["contact"] += int(ref[:nt].sum())
            if cname in ("discrete", "processed", "original"):
                stats["levels"] |= set(np.round(ref[-nt:][ref[:nt] > 0] * 5).astype(int).tolist())
    assert stats["contact"] > 50
    if cname in ("discrete", "processed", "original"):
        assert len(stats["levels"]) >= 4  # several discretisation levels occur


# the same reference pins on the double-precision oracle build (tests/oracle_lib.f64_twin)
test_command_resample_matches_reference_replay_f64 = O.f64_twin(test_command_resample_matches_reference_replay)
test_trunk_material_matches_reference_replay_f64 = O.f64_twin(test_trunk_material_matches_reference_replay)
test_reset_object_state_matches_reference_replay_f64 = O.f64_twin(test_reset_object_state_matches_reference_replay)
test_noisy_object_state_observation_matches_reference_replay_f64 = O.f64_twin(test_noisy_object_state_observation_matches_reference_replay)
test_binary_tactile_matches_reference_replay_f64 = O.f64_twin(test_binary_tactile_matches_reference_replay)
test_every_tactile_signals_class_matches_reference_replay_f64 = O.f64_twin(test_every_tactile_signals_class_matches_reference_replay)
