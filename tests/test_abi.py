"""CPU-only checks of the C-ABI boundary: the library loads, exports every symbol include/lt_env.h declares,
the ctypes mirror matches, and the Python layout mirror agrees with lt_env_get_view.  No compute calls."""
import ctypes
import os
import re

import numpy as np
import pytest

from locotouch_amd import _abi
from locotouch_amd.layout import Layout, QUAD_FIELDS, field_quads

C = _abi.CONSTS


def test_library_exports_every_declared_symbol():
    lib = _abi.load()
    src = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lt_\w+)\s*\(", src)) - {"lt_align256"}
    declared = {d for d in declared if not d.startswith("lt_field") and not d.startswith("lt_layout") and d != "lt_quad"}
    assert declared == set(_abi.EXPORTS), declared ^ set(_abi.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name


def test_cfg_struct_mirror_and_defaults():
    lib = _abi.load()
    assert lib.lt_cfg_sizeof() == ctypes.sizeof(_abi.LtCfg)
    loco = _abi.default_cfg(C["LT_TASK_LOCOMOTION"])
    teach = _abi.default_cfg(C["LT_TASK_TRANSPORT_TEACHER"])
    assert lib.lt_cfg_obs_dim(ctypes.byref(loco)) == 270 and lib.lt_cfg_obs_dim(ctypes.byref(teach)) == 348
    assert loco.num_envs == 4096 and loco.decimation == 4 and abs(loco.sim_dt - 0.005) < 1e-9 and loco.max_episode_length == 1000
    # 17 active rewards for locomotion, 23 for the teacher
    assert sum(1 for i in range(C["LT_NUM_REWARD_TERMS"]) if loco.reward_weight[i] != 0) == 17
    assert sum(1 for i in range(C["LT_NUM_REWARD_TERMS"]) if teach.reward_weight[i] != 0) == 23
    assert [teach.term_enabled[i] for i in range(7)] == [1, 1, 1, 0, 1, 1, 1]
    assert [loco.term_enabled[i] for i in range(7)] == [1, 1, 1, 1, 1, 0, 0]
    assert teach.cmd_multi_sampling == 1 and teach.cur_enabled == 1 and loco.cur_enabled == 0
    assert lib.lt_cfg_default(7, ctypes.byref(loco)) == C["LT_EINVAL"]


@pytest.mark.parametrize("task,n,tactile,fmt,aux", [(0, 4096, 0, 0, 0), (1, 4096, 0, 0, 0), (1, 100, 0, 0, 0), (1, 17, 0, 0, 0), (1, 405, 1, 0, 0),
                                                    (1, 20, 1, 0, 3), (1, 33, 1, 4, 2), (1, 16, 1, 2, 1)])
def test_layout_mirror_matches_c(task, n, tactile, fmt, aux):
    lib = _abi.load()
    cfg = _abi.default_cfg(task, num_envs=n)
    cfg.tactile_enabled = tactile
    cfg.tactile_format, cfg.tactile_aux_groups = fmt, aux
    tdim = lib.lt_cfg_tactile_dim(ctypes.byref(cfg))
    assert tdim == (0 if not tactile else 884 if fmt in (4, 5) else 442)
    h = ctypes.c_void_p()
    assert lib.lt_env_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    nbytes = ctypes.c_size_t()
    assert lib.lt_env_state_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)) == 0
    L = Layout(n, lib.lt_cfg_obs_dim(ctypes.byref(cfg)), tactile, tdim or None)
    assert L.total_bytes == nbytes.value
    v = _abi.LtView()
    for name in QUAD_FIELDS:
        if name == "LT_F_PLATE_SAMPLES" and not tactile:  # the tactile fields exist only with cfg.tactile_enabled
            assert lib.lt_env_get_view(h, C[name], ctypes.byref(v)) == C["LT_EINVAL"]
            continue
        assert lib.lt_env_get_view(h, C[name], ctypes.byref(v)) == 0
        assert (v.ptr or 0) == L.quad_off[name], name
        assert list(v.shape) == [n, field_quads(name), 4] and list(v.stride) == [4, L.npad * 4, 1]
    for name, (off, dtype, shape) in L.plain.items():
        if name.startswith("_"):
            continue  # internal regions (device args block) have no public view
        bit = {"LT_F_OBS_TACTILE": 4, "LT_F_OBS_TACTILE_ORIGINAL": 1, "LT_F_OBS_TACTILE_PROCESSED": 2}.get(name)
        if bit and (not tactile or not ((aux | 4) & bit)):  # the tactile groups exist only when enabled
            assert lib.lt_env_get_view(h, C[name], ctypes.byref(v)) == C["LT_EINVAL"]
            continue
        assert lib.lt_env_get_view(h, C[name], ctypes.byref(v)) == 0
        assert (v.ptr or 0) == off, name
        if bit:
            assert list(v.shape)[:2] == [n, shape[1]] and list(v.stride)[:2] == [shape[1], 1], name
    assert lib.lt_env_get_view(h, 63, ctypes.byref(v)) == C["LT_EINVAL"]
    rc = lib.lt_env_get_view(h, C["LT_F_OBS_OBJECT_STATE"], ctypes.byref(v))  # a strided window of the policy rows
    if task == 1:
        assert rc == 0 and (v.ptr or 0) == L.plain["LT_F_OBS_POLICY"][0] + 270 * 4 and list(v.shape)[:2] == [n, 78] and list(v.stride)[:2] == [348, 1]
    else:
        assert rc == C["LT_EINVAL"]
    # error behaviour: stepping / resetting without a bound arena fails loudly, never silently
    assert lib.lt_env_reset_all(h, None) == C["LT_EFAULT"]
    dummy = (ctypes.c_float * 12)()
    assert lib.lt_env_step(h, ctypes.cast(dummy, ctypes.c_void_p), None) == C["LT_EFAULT"]
    assert b"not bound" in lib.lt_last_error()
    assert lib.lt_env_bind(h, ctypes.c_void_p(256), 16) == C["LT_EFAULT"]
    assert lib.lt_env_destroy(h) == 0


def test_invalid_cfg_rejected():
    lib = _abi.load()
    cfg = _abi.default_cfg(1)
    cfg.num_envs = 0
    h = ctypes.c_void_p()
    assert lib.lt_env_create(ctypes.byref(cfg), ctypes.byref(h)) == C["LT_EINVAL"]
    cfg.num_envs = 8
    cfg.obs_history = 3
    assert lib.lt_env_create(ctypes.byref(cfg), ctypes.byref(h)) == C["LT_EINVAL"]


def test_product_path_has_no_oracle_dependency():
    """The shipped package must never import / link the oracle (it is the checker, not the product)."""
    import glob
    import os

    root = os.path.dirname(_abi.__file__)
    for path in glob.glob(os.path.join(root, "**", "*.py"), recursive=True) + glob.glob(os.path.join(root, "csrc", "*")):
        text = open(path, errors="ignore").read()
        # comments may cite the oracle as the executable spec; code may not include, import, link or dlopen it
        assert not re.search(r'#include\s+"[^"]*oracle', text), path
        assert not re.search(r"oracle_lib|liblt_oracle|from\s+oracle|import\s+oracle|lt_oracle_\w+\s*\(", text), path
    _ = np


def test_update_and_recurrence_entry_points_validate_their_arguments_before_touching_the_gpu():
    """Error behaviour of the PPO-update / GRU entry points (include/lt_env.h): a bad argument is LT_EINVAL with a message, decided
    on the host - no launch, so this runs without a GPU."""
    lib = _abi.load()
    vp = ctypes.c_void_p
    one = vp(16)  # any non-null address: argument checks come before the first dereference / launch
    null = vp(None)
    bad = C["LT_EINVAL"]
    # lt_ppo_loss: null operand, zero rows, more than 16 actions
    args = [one] * 10 + [null]
    assert lib.lt_ppo_loss(*([null] + args[1:]), 128, 12, 0.2, 1.0, 0.01, 1, one, one, one, one, null) == bad
    assert lib.lt_ppo_loss(*args, 0, 12, 0.2, 1.0, 0.01, 1, one, one, one, one, null) == bad
    assert lib.lt_ppo_loss(*args, 128, 17, 0.2, 1.0, 0.01, 1, one, one, one, one, null) == bad
    assert b"lt_ppo_loss" in lib.lt_last_error()
    # lt_elu_backward_bias: N not a multiple of 4 / beyond 1024
    assert lib.lt_elu_backward_bias(one, one, 64, 130, 1.0, one, one, one, null) == bad
    assert lib.lt_elu_backward_bias(one, one, 64, 2048, 1.0, one, one, one, null) == bad
    assert lib.lt_elu_backward_bias_ws_floats(96, 512) == 2 * 512 and lib.lt_elu_backward_bias_ws_floats(97, 512) == 3 * 512
    # lt_head_wgrad: more than 16 outputs, k not a multiple of 4, k beyond 1024
    assert lib.lt_head_wgrad(one, one, 0, 64, 17, 128, one, one, one, null) == bad
    assert lib.lt_head_wgrad(one, one, 0, 64, 12, 130, one, one, one, null) == bad
    assert lib.lt_head_wgrad(one, one, 0, 64, 16, 2048, one, one, one, null) == bad and b"lt_head_wgrad" in lib.lt_last_error()
    assert lib.lt_head_wgrad_ws_floats(96, 12, 128) == 12 * 128 + 16
    # lt_adam_clip_step: empty buffer, step 0
    assert lib.lt_adam_clip_step(one, one, one, one, 0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, one, null, null) == bad
    assert lib.lt_adam_clip_step(one, one, one, one, 10, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, one, null, null) == bad
    assert lib.lt_adam_clip_step_ws_floats(2048) == 1 and lib.lt_adam_clip_step_ws_floats(2049) == 2
    # GRU: hidden size must be a multiple of 64
    assert lib.lt_gru_forward(one, one, one, one, one, 4, 8, 96, one, one, null) == bad
    assert lib.lt_gru_backward(one, null, one, one, one, one, 4, 8, 96, one, one, one, one, null) == bad
    assert b"multiple of 64" in lib.lt_last_error()


def test_population_pass_placement_api():
    """lt_env_defer_gate / lt_env_gate_update (include/lt_env.h): modes 0..2, nothing to do while no pass is outstanding, no launch
    without a bound arena."""
    lib = _abi.load()
    cfg = _abi.default_cfg(1, num_envs=64)
    h = ctypes.c_void_p()
    assert lib.lt_env_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    for mode in (0, 1, 2, 0):
        assert lib.lt_env_defer_gate(h, mode) == 0
    assert lib.lt_env_defer_gate(h, 4) == C["LT_EINVAL"] and lib.lt_env_defer_gate(h, -1) == C["LT_EINVAL"]  # (3 = mode 2 + the lost-announcement test hook)
    assert lib.lt_env_defer_gate(None, 0) == C["LT_EINVAL"]
    assert lib.lt_env_gate_update(h, None) == C["LT_EFAULT"] and b"not bound" in lib.lt_last_error()
    assert lib.lt_env_destroy(h) == 0


def test_train_script_dumps_env_and_agent_params(tmp_path):
    """params/{env,agent}.{yaml,pkl} (reference locotouch/scripts/train.py:150-153): the resolved lt_cfg and the agent cfg as dicts."""
    import pickle

    import yaml

    from locotouch_amd import _abi as A
    from locotouch_amd.agents import train_cfg
    from locotouch_amd.scripts.train import dump_params

    task = "Isaac-RandCylinderTransportTeacher-LocoTouch-v1"
    cfg = A.preset_cfg(task, num_envs=128)
    dump_params(str(tmp_path), dict(cfg.to_dict(), gym_id=task), train_cfg(task))
    assert sorted(os.listdir(tmp_path / "params")) == ["agent.pkl", "agent.yaml", "env.pkl", "env.yaml"]
    env = yaml.safe_load(open(tmp_path / "params" / "env.yaml"))
    assert env["num_envs"] == 128 and env["gym_id"] == task and len(env["reward_weight"]) >= 25
    assert pickle.load(open(tmp_path / "params" / "env.pkl", "rb")) == env
    assert pickle.load(open(tmp_path / "params" / "agent.pkl", "rb")) == yaml.safe_load(open(tmp_path / "params" / "agent.yaml"))


# ---- the binding is derived from the header: pinned against literals, not against the parser itself ----
_vp, _int, _i64, _f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_P = ctypes.POINTER


def test_every_prototype_has_a_derived_signature():
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S))
    protos = set(re.findall(r"\b(lt_\w+)\s*\([^()]*\)\s*;", src))
    assert len(protos) == 67 and protos == set(_abi.EXPORTS) == set(_abi.SIGNATURES)
    assert len(_abi.EXPORTS) == len(set(_abi.EXPORTS))
    lib = _abi.load()
    for name, (restype, argtypes) in _abi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes and fn.restype is restype, name
    assert _abi.VALUE_QUERIES <= protos
    assert all(_abi.SIGNATURES[n][0] is _int for n in protos - _abi.VALUE_QUERIES)


def test_derived_signatures_match_literals():
    """One literal signature per branch of the type rule (scalars, data pointers, const char*, structure pointers, size_t*,
    pointer to pointer, an array parameter, the opaque handle, every restype)."""
    S = _abi.SIGNATURES
    assert S["lt_wgrad"] == (_int, [_vp, _int, _vp, _vp, _int, _i64, _int, _int, _vp, _int, _vp, _vp, _vp])
    assert S["lt_ppo_loss"] == (_int, [_vp] * 11 + [_i64, _int, _f32, _f32, _f32, _int] + [_vp] * 5)
    assert S["lt_partial_sums"] == (_int, [_int, _P(_vp), _vp, _vp, _vp, _vp, _P(_vp), _P(_vp), _vp])
    assert S["lt_env_create"] == (_int, [_P(_abi.LtCfg), _P(_vp)])
    assert S["lt_env_state_bytes"] == (_int, [_P(_abi.LtCfg), _P(ctypes.c_size_t)])
    assert S["lt_mlp_backward_blocks"] == (_i64, [_P(_abi.LtMlpDesc), _P(_abi.LtMlpDesc), _i64])
    assert S["lt_cfg_preset_id"] == (ctypes.c_char_p, [_int])
    assert S["lt_cfg_preset"] == (_int, [ctypes.c_char_p, _P(_abi.LtCfg)])
    assert S["lt_env_set_command_ranges"] == (_int, [_vp, _vp, _int, _f32, _vp])
    assert S["lt_rollout_act"] == (_int, [_i64, _int, ctypes.c_uint64] + [_vp] * 15)
    assert S["lt_env_render"] == (_int, [_vp, _P(_abi.LtRenderDesc), _P(_abi.LtRenderView), _int, _vp, _vp, _vp, _vp, _vp])
    assert S["lt_env_get_view"] == (_int, [_vp, _int, _P(_abi.LtView)])
    assert S["lt_cfg_sizeof"] == (ctypes.c_size_t, []) and S["lt_last_error"] == (ctypes.c_char_p, [])
    assert S["lt_env_bind"] == (_int, [_vp, _vp, ctypes.c_size_t])


def test_derived_structures_match_literals():
    i32 = ctypes.c_int32
    want = {
        "LtView": [("ptr", _vp), ("dtype", i32), ("ndim", i32), ("shape", _i64 * 3), ("stride", _i64 * 3)],
        "LtMlpDesc": [("num_layers", i32), ("dims", i32 * 7), ("activation", i32), ("input_format", i32)],
        "LtRenderView": [("env_id", i32), ("origin", i32), ("eye", _f32 * 3), ("lookat", _f32 * 3), ("fov_y_deg", _f32)],
        "LtRenderDesc": [("width", i32), ("height", i32), ("flags", i32), ("light_dir", _f32 * 3)],
    }
    for name, fields in want.items():
        cls = getattr(_abi, name)
        assert cls.__name__ == name and issubclass(cls, ctypes.Structure)
        assert list(cls._fields_) == fields, name
    assert ctypes.sizeof(_abi.LtView) == 64 and ctypes.sizeof(_abi.LtMlpDesc) == 40
    assert ctypes.sizeof(_abi.LtRenderView) == 36 and ctypes.sizeof(_abi.LtRenderDesc) == 24
    assert ctypes.sizeof(_abi.LtCfg) == _abi.load().lt_cfg_sizeof()
    cfg = _abi.default_cfg(1)
    assert isinstance(cfg.copy(), _abi.LtCfg) and cfg.copy().to_dict() == cfg.to_dict()
    assert [n for n, _ in _abi.LtCfg._fields_][:3] == ["seed", "num_envs", "task"] and dict(_abi.LtCfg._fields_)["cmd_range_init"] is _f32 * 2 * 3


@pytest.mark.parametrize("fragment,named", [
    ("int lt_bad(struct foo* x);", "lt_bad"),                    # a type the rule does not know
    ("int lt_bad(float m[3][3]);", "lt_bad"),                    # an array of arrays as a parameter
    ("long double lt_bad(void);", "lt_bad"),                     # an unknown return type
    ("int lt_bad(float*** p);", "lt_bad"),                       # deeper than pointer to pointer
    ("typedef struct lt_s { short v; } lt_s;", "lt_s"),          # an untypeable member
    ("typedef struct lt_s { float v[LT_NOPE]; } lt_s;", "lt_s"),  # an unknown array bound
    ("int lt_ok(int a); static inline int lt_f(int a) { return a; }", "lt_f"),  # not a plain prototype
], ids=["unknown-type", "array-of-arrays", "unknown-return", "triple-pointer", "member-type", "array-bound", "not-a-prototype"])
def test_parser_refuses_what_it_cannot_type(fragment, named):
    with pytest.raises(ImportError, match=named):
        _abi.parse_header(fragment)


def test_parser_on_a_fragment():
    consts, structs, protos = _abi.parse_header("""
        #define LT_N 3
        enum lt_e { LT_A = 4, LT_B };
        typedef struct lt_h lt_h;
        typedef struct lt_s { float a[LT_N + 1], b; void* p; } lt_s;
        void lt_f(lt_h* h, lt_h** out, const lt_s* s, const double* d, const float* const* pp, const float v[2], void* q);
        float lt_g(void);
    """)
    assert consts == {"LT_N": 3, "LT_A": 4, "LT_B": 5}
    s = structs["lt_s"]
    assert s.__name__ == "LtS" and list(s._fields_) == [("a", _f32 * 4), ("b", _f32), ("p", _vp)]
    assert protos == {"lt_f": (None, [_vp, _P(_vp), _P(s), _vp, _P(_vp), _vp, _vp]), "lt_g": (_f32, [])}
    typed = _abi.parse_header("void lt_f(const double* d, const float* u8[8], float v[2], void* q, const int* n);", typed=True)[2]
    assert typed["lt_f"] == (None, [_P(ctypes.c_double), _P(_P(_f32)), _P(_f32), _vp, _P(_int)])


def test_call_helper():
    import torch

    t = torch.arange(8, dtype=torch.float32)
    assert _abi.ptr(t).value == t.data_ptr() and _abi.ptr(t[2:]).value == t.data_ptr() + 8
    assert _abi.ptr(None).value is None and _abi.ptr(0).value is None and _abi.ptr(4096).value == 4096
    held = ctypes.c_void_p(32)
    assert _abi.ptr(held) is held
    arr = _abi.ptr_array([t, None, t[4:]])
    assert isinstance(arr, ctypes.c_void_p * 3) and list(arr) == [t.data_ptr(), None, t.data_ptr() + 16]
    assert len(_abi.ptr_array([])) == 1  # never a zero-length array
    # a bad argument is LT_EINVAL decided on the host (no launch): RuntimeError carrying lt_last_error()
    with pytest.raises(RuntimeError, match=r"lt_elu_backward_bias failed with code -22: lt_elu_backward_bias.*multiple of 4"):
        _abi.call("lt_elu_backward_bias", t, t, 64, 130, 1.0, t, t, t, None)
    with pytest.raises(RuntimeError, match="lt_head_wgrad"):
        _abi.call("lt_head_wgrad", 16, 16, 0, 64, 17, 128, 16, 16, 16, 0)
    # None / 0 reach the library as NULL, a tensor as its address: lt_ppo_loss names the first NULL operand it finds
    with pytest.raises(RuntimeError, match="lt_ppo_loss"):
        _abi.call("lt_ppo_loss", None, *[t] * 9, None, 128, 12, 0.2, 1.0, 0.01, 1, t, t, t, t, None)
    # structures go by reference, statuses of 0 return None
    cfg, nbytes, h = _abi.default_cfg(1, num_envs=64), ctypes.c_size_t(), ctypes.c_void_p()
    assert _abi.call("lt_env_state_bytes", cfg, ctypes.byref(nbytes)) is None and nbytes.value > 0
    assert _abi.call("lt_env_create", cfg, ctypes.byref(h)) is None and h.value
    v = _abi.LtView()
    _abi.call("lt_env_get_view", h, C["LT_F_REWARD"], v)
    assert list(v.shape)[:1] == [64] and v.ndim == 1
    with pytest.raises(RuntimeError, match="not bound"):
        _abi.call("lt_env_reset_all", h, None)
    _abi.call("lt_env_destroy", h)
    # value-returning queries are not statuses
    for name in ("lt_wgrad_splits", "lt_abi_version", "lt_mlp_kernel_name"):
        with pytest.raises(TypeError, match=name):
            _abi.call(name, 1, 2, 3)
    with pytest.raises(ValueError):  # a wrong argument count is an error, not a shifted call
        _abi.call("lt_env_destroy", h, None)


# ---- the table of headers (_abi.HEADERS) is held to the tree ----
def _declared(path):
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))
    return set(re.findall(r"^[ \t]*(?:const[ \t]+)?\w+[ \t*]+(lt_\w+)\s*\([^()]*\)\s*;", src, flags=re.M))  # a result type, a name, no body


def test_header_table_matches_the_tree(tmp_path):
    import glob

    include = os.path.join(_abi.REPO, "include")
    with_protos = sorted(os.path.basename(p) for p in glob.glob(os.path.join(include, "*.h")) if _declared(p))
    assert sorted(row[1] for row in _abi.HEADERS) == with_protos  # every header that declares an entry point, each once
    total, queries = 0, set()
    for prefix, fname, _, row_queries, published in _abi.HEADERS:
        p = prefix + "_" if prefix else ""
        assert getattr(_abi, p + "HEADER") == os.path.join(include, fname)
        sigs = getattr(_abi, p + "SIGNATURES")
        assert set(sigs) == _declared(os.path.join(include, fname)) and sigs, fname
        assert getattr(_abi, p + "VALUE_QUERIES") == frozenset(row_queries) <= set(sigs), fname
        for c in published:
            cls = getattr(_abi, "".join(w.capitalize() for w in c.split("_")))
            assert issubclass(cls, ctypes.Structure) and ctypes.sizeof(cls) > 0, c
        total += len(sigs)
        queries |= set(row_queries)
    assert len(_abi.ALL_SIGNATURES) == total and _abi.ALL_VALUE_QUERIES == queries  # no name of one header hides another's
    _abi.load()
    assert set(_abi._calls) == set(_abi.ALL_SIGNATURES) - queries  # `call` serves every status, and nothing that returns a value
    # the loop refuses, by name: a repeated entry point, a value query its header does not declare, a result that is no int
    (tmp_path / "a.h").write_text("int lt_one(int a);\nint lt_two(void);\n")
    (tmp_path / "b.h").write_text("int lt_three(void);\nint lt_two(float x);\n")
    (tmp_path / "c.h").write_text("float lt_four(void);\n")
    rows = {n: (n.upper(), n + ".h", False, (), ()) for n in "abc"}
    assert [set(b[3]) for b in _abi._bind((rows["a"],), str(tmp_path))] == [{"lt_one", "lt_two"}]
    with pytest.raises(ImportError, match=r"b\.h.*lt_two"):
        _abi._bind((rows["a"], rows["b"]), str(tmp_path))
    with pytest.raises(ImportError, match=r"a\.h.*lt_gone"):
        _abi._bind((("A", "a.h", False, ("lt_gone",), ()),), str(tmp_path))
    with pytest.raises(ImportError, match=r"c\.h.*lt_four"):
        _abi._bind((("C", "c.h", False, ("lt_four",), ()),), str(tmp_path))
    assert _abi._bind((("", "c.h", False, ("lt_four",), ()),), str(tmp_path))[0][4] == {"lt_four"}  # lt_env.h's queries alone may
