"""ctypes loader for the CPU oracle (oracle/_build/liblt_oracle.so) - test infrastructure only.

`load("f64")` / `OracleEnv(cfg, precision="f64")` use liblt_oracle_f64.so: the same source built with every continuous
quantity in double (-DLT_REAL=double) behind the same f32 ABI and arena, a high-precision reference for one step.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module.
"""
from __future__ import annotations

import ctypes
import functools
import inspect
import os
import subprocess

import numpy as np

from locotouch_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.path.join(REPO, "oracle", "_build", "liblt_oracle.so")
ORACLE_SOS = {"f32": ORACLE_SO, "f64": os.path.join(REPO, "oracle", "_build", "liblt_oracle_f64.so")}
PRECISIONS = tuple(ORACLE_SOS)

f32 = ctypes.c_float

# oracle/lt_oracle.h through the product's header parser, with typed data pointers (the callers pass POINTER(c_float) etc.)
_, _STRUCTS, _SIGNATURES = _abi.parse_header(open(os.path.join(REPO, "oracle", "lt_oracle.h")).read(), typed=True,
                                             structs={"lt_cfg": _abi.LtCfg})
TermIn, GaitIO = _STRUCTS["lt_term_in"], _STRUCTS["lt_gait_io"]

_libs: dict = {}


def load(precision: str = "f32") -> ctypes.CDLL:
    if precision in _libs:
        return _libs[precision]
    so = ORACLE_SOS[precision]
    src = os.path.join(REPO, "oracle", "lt_oracle.c")
    if not all(os.path.exists(p) and os.path.getmtime(p) >= os.path.getmtime(src) for p in ORACLE_SOS.values()):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle")], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(so)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _libs[precision] = lib
    return lib


def f64_twin(test):
    """The same test against the f64 oracle build, as a test of its own (`<name>_f64`): `test` takes `precision="f32"` as its
    last, defaulted argument, which pytest leaves alone, so the f32 test keeps its id and its fixtures / parametrization."""
    sig = inspect.signature(test)
    assert "precision" in sig.parameters, test.__name__

    @functools.wraps(test)
    def twin(*args, **kw):
        return test(*args, **kw, precision="f64")

    twin.__signature__ = sig.replace(parameters=[p for p in sig.parameters.values() if p.name != "precision"])
    twin.__name__ = twin.__qualname__ = test.__name__ + "_f64"
    return twin


def policy_normals(seed: int, n: int, step: int) -> np.ndarray:
    """The policy head's N(0,1) draws [n][12] in double (lt_oracle_policy_normals)."""
    z = np.zeros((n, 12), np.float64)
    load("f64").lt_oracle_policy_normals(seed, n, step, z.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return z


def fptr(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(f32))


class OracleEnv:
    """Whole-env oracle on a host arena with the device layout (include/lt_layout.h)."""

    def __init__(self, cfg: _abi.LtCfg, precision: str = "f32"):
        self.cfg = cfg.copy()
        self.precision = precision
        self.lib = load(precision)
        self.nbytes = self.lib.lt_oracle_state_bytes(ctypes.byref(self.cfg))
        self.arena = np.zeros(self.nbytes, dtype=np.uint8)

    @property
    def ptr(self):
        return self.arena.ctypes.data_as(ctypes.c_void_p)

    def reset_all(self):
        self.lib.lt_oracle_reset_all(ctypes.byref(self.cfg), self.ptr)

    def step(self, actions: np.ndarray, nthreads: int = 1):
        a = np.ascontiguousarray(actions, dtype=np.float32)
        self.lib.lt_oracle_step(ctypes.byref(self.cfg), self.ptr, fptr(a), nthreads)

    def curriculum_update(self, records: np.ndarray):
        r = np.ascontiguousarray(records, dtype=np.float32)
        self.lib.lt_oracle_curriculum_update(ctypes.byref(self.cfg), self.ptr, fptr(r))

    def curriculum_apply_global(self, ring_sums: np.ndarray, nsteps: int, n_total: int):
        r = np.ascontiguousarray(ring_sums, dtype=np.float32)
        self.lib.lt_oracle_curriculum_apply_global(ctypes.byref(self.cfg), self.ptr, fptr(r), int(nsteps), int(n_total))

    def eval_terms(self):
        self.lib.lt_oracle_eval_terms(ctypes.byref(self.cfg), self.ptr)

    def tactile_update(self):
        """The tactile pass alone on the arena as it stands (the twin of LocoTouchVecEnv.tactile_update)."""
        self.lib.lt_oracle_tactile_update(ctypes.byref(self.cfg), self.ptr)
