"""Contact-force vectors (lt_env_contact_force_bytes / lt_env_bind_contact_forces, include/lt_env.h), CPU side: the buffer size,
what binding refuses, and how the buffer maps to IsaacLab's net_forces_w_history through TermEnv - body order (trunk, then
1 + type * 4 + leg), slot order (newest first) and the object sensor.  No GPU: binding launches nothing, and the mapping runs on a
CPU vec that carries a synthetic buffer.  (GPU twin: tests/test_hip_contact_forces.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from locotouch_amd import _abi
from locotouch_amd.compat.scene_views import BODY_NAMES, ROBOT_SENSOR, ExtraTerms, TermEnv
from locotouch_amd.env import object_forces_from_buffer, robot_forces_from_buffer
from tests.oracle_vec_env import OracleVecEnv

C = _abi.CONSTS
TEACHER = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
FEET = [13, 14, 15, 16]


def _env(task=C["LT_TASK_TRANSPORT_TEACHER"], n=17, **cfg_fields):
    lib = _abi.load()
    cfg = _abi.default_cfg(task, num_envs=n)
    for k, v in cfg_fields.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    assert lib.lt_env_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    return lib, h


@pytest.mark.parametrize("n", [17, 4096, 8208])
def test_contact_force_bytes(n):
    lib, h = _env(n=n)
    try:
        nb = ctypes.c_size_t()
        assert lib.lt_env_contact_force_bytes(h, ctypes.byref(nb)) == 0
        npad = (n + 15) // 16 * 16
        assert nb.value == 3 * 14 * npad * 16
    finally:
        lib.lt_env_destroy(h)


def test_bind_refuses_bad_buffers_and_cfgs():
    lib, h = _env(n=100)
    fake = 1 << 20  # never dereferenced: binding only records the pointer
    try:
        nb = ctypes.c_size_t()
        assert lib.lt_env_contact_force_bytes(h, ctypes.byref(nb)) == 0
        assert lib.lt_env_bind_contact_forces(h, ctypes.c_void_p(fake), nb.value - 1) == C["LT_EINVAL"]
        assert b"too small" in lib.lt_last_error()
        assert lib.lt_env_bind_contact_forces(h, ctypes.c_void_p(fake + 16), nb.value) == C["LT_EINVAL"]
        assert b"256-byte aligned" in lib.lt_last_error()
        assert lib.lt_env_bind_contact_forces(h, ctypes.c_void_p(fake), nb.value) == 0
        assert lib.lt_env_bind_contact_forces(h, None, 0) == 0  # NULL unbinds
    finally:
        lib.lt_env_destroy(h)
    lib, h = _env(n=100, decimation=2)
    try:
        nb = ctypes.c_size_t()
        assert lib.lt_env_contact_force_bytes(h, ctypes.byref(nb)) == 0
        assert lib.lt_env_bind_contact_forces(h, ctypes.c_void_p(fake), nb.value) == C["LT_EINVAL"]
        assert b"decimation" in lib.lt_last_error()
        assert lib.lt_env_bind_contact_forces(h, None, 0) == 0
    finally:
        lib.lt_env_destroy(h)


class _VecWithForces(OracleVecEnv):
    """The CPU oracle env plus a contact-force buffer in the lt_env_bind_contact_forces layout, filled by the test."""

    def __init__(self, n, vectors=True):
        super().__init__(TEACHER, num_envs=n)
        self.contact_force_vectors = vectors
        self.buf = torch.zeros(3, 14, (n + 15) // 16 * 16, 4)

    @property
    def contact_forces_w_history(self):
        return robot_forces_from_buffer(self.buf, self.num_envs)

    @property
    def object_forces_w_history(self):
        return object_forces_from_buffer(self.buf, self.num_envs)


def _expected(buf, n):
    """(n, 3, 17, 3) and (n, 3, 1, 3) read element by element from the buffer layout of include/lt_env.h."""
    rob = np.zeros((n, 3, 17, 3), np.float32)
    obj = np.zeros((n, 3, 1, 3), np.float32)
    b = buf.numpy()
    for e in range(n):
        for s in range(3):
            for c in range(3):
                rob[e, s, 0, c] = b[s, 12, e, c]
                obj[e, s, 0, c] = b[s, 13, e, c]
                for ty in range(4):
                    for leg in range(4):
                        rob[e, s, 1 + ty * 4 + leg, c] = b[s, ty * 3 + c, e, leg]
    return rob, obj


def test_buffer_maps_to_sensor_views_in_body_and_slot_order():
    n = 20
    vec = _VecWithForces(n)
    vec.buf.copy_(torch.arange(vec.buf.numel(), dtype=torch.float32).reshape(vec.buf.shape))  # every element distinct
    te = TermEnv(vec)
    rob, obj = _expected(vec.buf, n)
    d = te.scene.sensors[ROBOT_SENSOR].data
    assert tuple(d.net_forces_w_history.shape) == (n, 3, 17, 3)
    np.testing.assert_array_equal(d.net_forces_w_history.numpy(), rob)
    np.testing.assert_array_equal(d.net_forces_w.numpy(), rob[:, 0])
    od = te.scene.sensors["object_contact_sensor"].data
    assert tuple(od.net_forces_w_history.shape) == (n, 3, 1, 3)
    np.testing.assert_array_equal(od.net_forces_w_history.numpy(), obj)
    np.testing.assert_array_equal(od.net_forces_w.numpy(), obj[:, 0])
    # spot checks against the names: env 5, newest slot, the rear-left calf (type 2, leg 3), y component
    assert BODY_NAMES[1 + 2 * 4 + 3] == "d_RL_calf"
    assert d.net_forces_w[5, 1 + 2 * 4 + 3, 1] == vec.buf[0, 2 * 3 + 1, 5, 3]
    # the oldest slot of the trunk's z component
    assert d.net_forces_w_history[5, 2, 0, 2] == vec.buf[2, 12, 5, 2]


def test_without_vectors_the_views_stay_norms():
    vec = _VecWithForces(20, vectors=False)
    te = TermEnv(vec)
    h = te.scene.sensors[ROBOT_SENSOR].data.net_forces_w_history
    assert torch.all(h[..., :2] == 0)
    assert not hasattr(te.scene.sensors["object_contact_sensor"].data, "net_forces_w")


def stumble_user(env, sensor_name, body_ids, ratio=4.0):
    """1 where a body's horizontal contact force exceeds `ratio` times its vertical one (a user term reading force components)."""
    f = env.scene.sensors[sensor_name].data.net_forces_w[:, body_ids]
    return torch.any(torch.norm(f[..., :2], dim=-1) > ratio * torch.abs(f[..., 2]), dim=1).float()


@pytest.mark.parametrize("vectors", [True, False])
def test_stumble_term_sees_horizontal_forces_only_with_vectors(vectors):
    n = 20
    vec = _VecWithForces(n, vectors=vectors)
    # every foot stands (F_z = 50 N); in envs 3 and 7 the front-left foot is pushed sideways (|F_xy| = 30 N > 4 * 5 N)
    vec.buf[:, 3 * 3 + 2] = 50.0
    for e in (3, 7):
        vec.buf[0, 3 * 3 + 0, e, 1] = 24.0
        vec.buf[0, 3 * 3 + 1, e, 1] = -18.0
        vec.buf[0, 3 * 3 + 2, e, 1] = 5.0
    extra = ExtraTerms(vec)
    extra.add_reward("stumble", stumble_user, -1.0, {"sensor_name": ROBOT_SENSOR, "body_ids": FEET})
    extra.apply(torch.zeros(n), torch.zeros(n, dtype=torch.long))
    val = extra.last_values["stumble"]
    want = torch.zeros(n)
    if vectors:
        want[[3, 7]] = 1.0
    else:  # |F| lands in z, x and y are 0: the term cannot fire (the gap the vectors close)
        assert float(val.sum()) == 0.0
    assert torch.equal(val, want)
