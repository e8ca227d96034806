"""Independent numpy (float64) twin of the HIP renderer (locotouch_amd/csrc/lt_render.hip) for the GPU tests.

Body poses come from compat/scene_views.link_kinematics (torch forward kinematics), not from the kernel's own FK; the primitives are
built from the URDF-derived constants and intersected per pixel without culling.  Returns ids, depth, rgb and the shadow flag per pixel.
"""
from __future__ import annotations

import numpy as np
import torch

from locotouch_amd import render as R
from locotouch_amd.compat.scene_views import link_kinematics

# include/lt_go1_model.h
TRUNK_HALF = (0.128, 0.05, 0.057)
HIP_R, HIP_LEN, HIP_Y = 0.046, 0.04, (-0.08, 0.08, -0.08, 0.08)
THIGH_BOX, CALF_BOX = (0.213, 0.0245, 0.034), (0.213, 0.016, 0.016)
FOOT_R = 0.02
BACK_TOP_Z, BACK_HALF_X, BACK_HALF_Y = 0.093, 0.125, 0.087
RAIL_Y, RAIL_Z, RAIL_R = 0.087, 0.083, 0.01
TAXEL_ROWS, TAXEL_COLS, TAXEL_X0, TAXEL_Y0, TAXEL_DX, TAXEL_DY = 17, 13, 0.1144, 0.0768, 0.0143, 0.0128
FAR, AMBIENT = 1000.0, 0.3
BOX, CYL, SPHERE = 0, 1, 2
TRUNK, BACK_MID, PLATE, RAIL_L, RAIL_R_, HIP, THIGH, CALF, FOOT, OBJECT, GROUND = 0, 1, 2, 3, 4, 5, 9, 13, 17, 21, 22


def quat_mat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def body_poses(root_pos, root_quat, joint_pos):
    """(17, 7) world pos + quat wxyz from link_kinematics (float64)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64)[None])  # noqa: E731
    z3 = torch.zeros(1, 3, dtype=torch.float64)
    pos, quat, _, _ = link_kinematics(t(root_pos), t(root_quat), z3, z3, t(joint_pos), torch.zeros(1, 12, dtype=torch.float64))
    return np.concatenate([pos[0].numpy(), quat[0].numpy()], axis=1)


def primitives(poses, obj=None):
    """[(id, type, R, c, e)] in the kernel's order; `obj` = (pos, quat, radius, length) or None."""
    out = []

    def add(pid, typ, body, off, e, rot=False):
        p, q = poses[body, :3], poses[body, 3:]
        B = quat_mat(q)
        Rm = B @ np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) if rot else B
        out.append((pid, typ, Rm, p + B @ np.asarray(off, np.float64), np.asarray(e, np.float64)))

    add(TRUNK, BOX, 0, (0, 0, 0), TRUNK_HALF)
    add(BACK_MID, BOX, 0, (0, 0, 0.5 * RAIL_Z), (BACK_HALF_X, RAIL_Y + RAIL_R, 0.5 * RAIL_Z))
    add(PLATE, BOX, 0, (0, 0, 0.5 * (BACK_TOP_Z + RAIL_Z)), (BACK_HALF_X, BACK_HALF_Y, 0.5 * (BACK_TOP_Z - RAIL_Z)))
    add(RAIL_L, CYL, 0, (0, RAIL_Y, RAIL_Z), (RAIL_R, BACK_HALF_X, 0), rot=True)
    add(RAIL_R_, CYL, 0, (0, -RAIL_Y, RAIL_Z), (RAIL_R, BACK_HALF_X, 0), rot=True)
    for leg in range(4):
        add(HIP + leg, CYL, 1 + leg, (0, HIP_Y[leg], 0), (HIP_R, 0.5 * HIP_LEN, 0))
        add(THIGH + leg, BOX, 5 + leg, (0, 0, -0.5 * THIGH_BOX[0]), (0.5 * THIGH_BOX[2], 0.5 * THIGH_BOX[1], 0.5 * THIGH_BOX[0]))
        add(CALF + leg, BOX, 9 + leg, (0, 0, -0.5 * CALF_BOX[0]), (0.5 * CALF_BOX[2], 0.5 * CALF_BOX[1], 0.5 * CALF_BOX[0]))
        add(FOOT + leg, SPHERE, 13 + leg, (0, 0, 0), (FOOT_R, 0, 0))
    if obj is not None:
        p, q, r, length = obj
        out.append((OBJECT, CYL, quat_mat(np.asarray(q, np.float64)), np.asarray(p, np.float64), np.array([r, 0.5 * length, 0.0])))
    return out


def intersect(prim, o, d, tmax):
    """Nearest t per ray (rays (N, 3), origins (N, 3) or (3,)) in (0, tmax); returns (t, world normal); t == tmax: no hit."""
    _, typ, Rm, c, e = prim
    n = d.shape[0]
    lo = np.broadcast_to((o - c) @ Rm, (n, 3))  # R^T (o - c)
    ld = d @ Rm
    t = np.full(n, np.inf)
    ln = np.zeros((n, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        if typ == BOX:
            tn = np.full(n, -np.inf)
            tf = np.full(n, np.inf)
            ax = np.zeros(n, int)
            sg = np.zeros(n)
            ok = np.ones(n, bool)
            for k in range(3):
                par = np.abs(ld[:, k]) < 1e-12
                ok &= ~(par & (np.abs(lo[:, k]) > e[k]))
                ta = (-e[k] - lo[:, k]) / ld[:, k]
                tb = (e[k] - lo[:, k]) / ld[:, k]
                lo_t, hi_t = np.minimum(ta, tb), np.maximum(ta, tb)
                lo_t[par], hi_t[par] = -np.inf, np.inf
                upd = lo_t > tn
                tn = np.where(upd, lo_t, tn)
                ax = np.where(upd, k, ax)
                sg = np.where(upd, np.where(ld[:, k] > 0, -1.0, 1.0), sg)
                tf = np.minimum(tf, hi_t)
            hit = ok & (tn <= tf) & (tn > 0)
            t = np.where(hit, tn, np.inf)
            ln[np.arange(n), ax] = sg
        elif typ == CYL:
            r, h = e[0], e[1]
            a = ld[:, 0] ** 2 + ld[:, 2] ** 2
            b = lo[:, 0] * ld[:, 0] + lo[:, 2] * ld[:, 2]
            cc = lo[:, 0] ** 2 + lo[:, 2] ** 2 - r * r
            disc = b * b - a * cc
            ts = (-b - np.sqrt(np.maximum(disc, 0))) / a
            y = lo[:, 1] + ts * ld[:, 1]
            side = (a > 1e-12) & (disc >= 0) & (ts > 0) & (np.abs(y) <= h)
            t = np.where(side, ts, np.inf)
            ln = np.where(side[:, None], np.stack([lo[:, 0] + ts * ld[:, 0], np.zeros(n), lo[:, 2] + ts * ld[:, 2]], 1) / r, ln)
            for s in (-1.0, 1.0):
                tc = (s * h - lo[:, 1]) / ld[:, 1]
                x, z = lo[:, 0] + tc * ld[:, 0], lo[:, 2] + tc * ld[:, 2]
                cap = (np.abs(ld[:, 1]) > 1e-12) & (tc > 0) & (tc < t) & (x * x + z * z <= r * r) & (s * ld[:, 1] < 0)
                t = np.where(cap, tc, t)
                ln = np.where(cap[:, None], np.array([0.0, s, 0.0]), ln)
        else:
            r = e[0]
            b = np.sum(lo * ld, 1)
            cc = np.sum(lo * lo, 1) - r * r
            disc = b * b - cc
            ts = -b - np.sqrt(np.maximum(disc, 0))
            hit = (disc >= 0) & (ts > 0)
            t = np.where(hit, ts, np.inf)
            ln = (lo + ts[:, None] * ld) / r
    t = np.where(t < tmax, t, tmax)
    return t, ln @ Rm.T


def render(state: dict, cam: R.Camera, width: int, height: int, flags: int = R.DEFAULT_FLAGS, light=R.DEFAULT_LIGHT):
    """state: root_pos (3), root_quat (4), joint_pos (12, type * 4 + leg), obj = (pos, quat, radius, length) or None, foot_force (4),
    taxels (221,) contact flags or None.  Returns dict(ids, depth, rgb float 0..255, shadow, poses)."""
    poses = body_poses(state["root_pos"], state["root_quat"], state["joint_pos"])
    prims = primitives(poses, state.get("obj"))
    eye, at = np.asarray(cam.eye, np.float64), np.asarray(cam.lookat, np.float64)
    if cam.origin == R.ORIGIN_ASSET_ROOT:
        eye, at = eye + state["root_pos"], at + state["root_pos"]
    d = R.ray_directions(eye, at, cam.fov_y_deg, width, height).reshape(-1, 3)
    n = d.shape[0]
    tbest = np.full(n, FAR)
    ids = np.full(n, -1)
    nrm = np.zeros((n, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = np.where((d[:, 2] < -1e-12) & (eye[2] > 0), -eye[2] / d[:, 2], np.inf)
    g = tg < tbest
    tbest, ids = np.where(g, tg, tbest), np.where(g, GROUND, ids)
    nrm[g] = (0.0, 0.0, 1.0)
    for p in prims:
        t, nn = intersect(p, eye, d, tbest)
        h = t < tbest
        tbest, ids = np.where(h, t, tbest), np.where(h, p[0], ids)
        nrm[h] = nn[h]
    ph = eye + tbest[:, None] * d
    base = np.zeros((n, 3))
    pal = {TRUNK: (0.25, 0.27, 0.30), BACK_MID: (0.25, 0.27, 0.30), PLATE: (0.80, 0.80, 0.78), RAIL_L: (0.55, 0.55, 0.58),
           RAIL_R_: (0.55, 0.55, 0.58), OBJECT: (0.15, 0.45, 0.85)}
    for leg in range(4):
        pal[HIP + leg], pal[THIGH + leg], pal[CALF + leg] = (0.35, 0.35, 0.38), (0.85, 0.55, 0.15), (0.20, 0.20, 0.22)
        tint = (flags & R._abi.CONSTS["LT_RENDER_CONTACT_TINT"]) and state["foot_force"][leg] > 1.0
        pal[FOOT + leg] = (0.95, 0.15, 0.10) if tint else (0.10, 0.10, 0.10)
    for pid, col in pal.items():
        base[ids == pid] = col
    gm = ids == GROUND
    par = (np.floor(ph[:, 0] * 2.0).astype(np.int64) + np.floor(ph[:, 1] * 2.0).astype(np.int64)) & 1
    base[gm] = np.where(par[gm, None] == 1, np.array([0.62, 0.62, 0.60]), np.array([0.42, 0.42, 0.40]))
    taxel_hit = np.full(n, -1)
    if flags & R._abi.CONSTS["LT_RENDER_TAXELS"]:
        pl = [p for p in prims if p[0] == PLATE][0]
        loc = (ph - pl[3]) @ pl[2]
        lnz = nrm @ pl[2][:, 2]
        row = np.rint((TAXEL_X0 - loc[:, 0]) / TAXEL_DX).astype(np.int64)
        col = np.rint((TAXEL_Y0 - loc[:, 1]) / TAXEL_DY).astype(np.int64)
        inside = ((ids == PLATE) & (lnz > 0.5) & (row >= 0) & (row < TAXEL_ROWS) & (col >= 0) & (col < TAXEL_COLS)
                  & (np.abs(loc[:, 0] - (TAXEL_X0 - TAXEL_DX * row)) <= 0.4 * TAXEL_DX)
                  & (np.abs(loc[:, 1] - (TAXEL_Y0 - TAXEL_DY * col)) <= 0.4 * TAXEL_DY))
        taxel_hit = np.where(inside, row * TAXEL_COLS + col, -1)
        tax = state.get("taxels")
        on = inside & (tax is not None) & (np.asarray(tax if tax is not None else np.zeros(221))[np.clip(taxel_hit, 0, 220)] > 0.5)
        base[inside] = (0.62, 0.64, 0.66)
        base[on] = (0.95, 0.20, 0.55)
    L = np.asarray(light, np.float64)
    L = L / np.linalg.norm(L)
    ndl = np.maximum(nrm @ L, 0.0)
    shadow = np.zeros(n, bool)
    if flags & R._abi.CONSTS["LT_RENDER_SHADOWS"]:
        cand = (ids >= 0) & (ndl > 0)
        so = ph + 1e-4 * nrm
        Ld = np.broadcast_to(L, (n, 3)).copy()
        for p in prims:
            t, _ = intersect(p, so, Ld, FAR)
            shadow |= cand & (t < FAR)
    ndl = np.where(shadow, 0.0, ndl)
    rgb = np.where((ids >= 0)[:, None], (AMBIENT + (1 - AMBIENT) * ndl)[:, None] * base, np.array([0.55, 0.70, 0.90]))
    rgb = np.clip(rgb, 0, 1) * 255.0
    shp = (height, width)
    depth = np.where(ids >= 0, tbest, R.DEPTH_MISS)
    return {"ids": ids.reshape(shp), "depth": depth.reshape(shp), "rgb": rgb.reshape(*shp, 3), "shadow": shadow.reshape(shp),
            "taxel": taxel_hit.reshape(shp), "poses": poses}


def env_state(env, e: int) -> dict:
    """The state render() needs, read from a LocoTouchVecEnv's views (float64 numpy)."""
    f = lambda name: env.field(name)[e].double().cpu().numpy()  # noqa: E731
    st = {"root_pos": f("LT_F_ROOT_POS")[0, :3], "root_quat": f("LT_F_ROOT_QUAT")[0, :4], "joint_pos": f("LT_F_JOINT_POS").reshape(12),
          "foot_force": f("LT_F_FORCE_HIST")[3], "obj": None, "taxels": None}
    if int(env.cfg.task) == R._abi.CONSTS["LT_TASK_TRANSPORT_TEACHER"]:
        prm = f("LT_F_OBJ_PARAMS")[0]
        st["obj"] = (f("LT_F_OBJ_POS")[0, :3], f("LT_F_OBJ_QUAT")[0, :4], prm[0], prm[1])
    if env.tactile:
        st["taxels"] = env.obs_tactile[e, :221].double().cpu().numpy()
    return st

