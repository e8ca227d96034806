"""ctypes mirror of include/lt_env.h and the headers beside it (one table, `HEADERS`), and loader of the HIP library (the product path).

Everything is parsed mechanically from the header - the `LT_*` constants, every structure and the signature of every entry
point - so the Python mirror cannot drift from the C ABI (a size check against `lt_cfg_sizeof()` guards it at load time) and
nobody counts pointers by hand.  `call` is the one way the package launches: it converts tensors / addresses / None to
pointers and raises on a non-zero status.  There is deliberately NO fallback: if `liblocotouch_env.so` is missing the import
fails loudly - nothing on the product path ever routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("LOCOTOUCH_AMD_LIB", os.path.join(_HERE, "_lib", "liblocotouch_env.so"))

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double}
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(\w*)\s*((?:\[[^\]]*\]\s*)*)")


def _ctype(decl, structs, opaque, consts, typed, param):
    """(name, ctypes type) of one C declarator, by the one rule of this binding: scalars by their C type; `const char*` ->
    c_char_p; pointer to a header structure -> POINTER(it); `size_t*` -> POINTER(c_size_t); pointer to pointer ->
    POINTER(c_void_p); every other pointer (and an array parameter, which decays to one) -> c_void_p, or with `typed` the
    typed POINTER.  None if the rule does not cover it."""
    m = _DECL.fullmatch(decl.strip())
    if not m:
        return None
    base, stars, name, dims = m.groups()
    depth = stars.count("*")
    try:
        dims = [sum(int(t) if t.strip().isdigit() else consts[t.strip()] for t in d.split("+")) for d in re.findall(r"\[([^\]]*)\]", dims)]
    except KeyError:
        return None
    if param and dims:  # an array parameter decays to a pointer to its elements
        depth, dims = depth + 1, dims[1:]
    t = structs.get(base) or _SCALARS.get(base)  # None: void, char or an opaque structure - pointers only
    if (t is None and base not in opaque and base not in ("void", "char")) or depth > 2 or (param and dims):
        return None
    if depth == 0 and t is None:
        return None
    if depth == 1 and base == "char":
        t = ctypes.c_char_p
    elif depth == 1:
        t = ctypes.POINTER(t) if t is not None and (typed or base in structs or base == "size_t") else ctypes.c_void_p
    elif depth == 2:
        t = ctypes.POINTER(ctypes.POINTER(t) if typed and t is not None else ctypes.c_void_p)
    for d in reversed(dims):
        t = t * d
    return name, t


def parse_header(text: str, typed: bool = False, structs: dict | None = None, bases: dict | None = None):
    """(constants, structures by C name, {entry point: (restype, [argtypes])}) of a C header in the style of lt_env.h.
    `structs`: structures other headers define; `bases`: Python base class per C structure name (for methods); `typed`: data
    pointers become typed POINTERs instead of c_void_p.  Whatever it cannot type raises ImportError naming it."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(LT_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    for m in re.finditer(r"enum\s+\w+\s*\{(.*?)\};", text, flags=re.S):
        val = -1
        for item in filter(None, (x.strip() for x in m.group(1).split(","))):
            name, _, v = (x.strip() for x in item.partition("="))
            val = int(v, 0) if v else val + 1
            consts[name] = val
    structs, opaque = dict(structs or {}), set(re.findall(r"typedef\s+struct\s+\w+\s+(\w+)\s*;", text))
    for m in re.finditer(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for line in filter(None, (x.strip() for x in m.group(1).split(";"))):
            first, *more = line.split(",")
            base = _DECL.match(first.strip())
            for decl in [first] + [f"{base.group(1) if base else ''} {x}" for x in more]:  # `float a[3], b[4];`
                field = _ctype(decl, structs, opaque, consts, typed, param=False)
                if field is None:
                    raise ImportError(f"cannot type member {decl.strip()!r} of {m.group(2)}")
                fields.append(field)
        pyname = "".join(w.capitalize() for w in m.group(2).split("_"))
        structs[m.group(2)] = type(pyname, ((bases or {}).get(m.group(2), ctypes.Structure),), {"_fields_": fields})
    rest = re.sub(r"^[ \t]*#[^\n]*$|typedef\s+struct\b[^;{]*(\{.*?\})?[^;{]*;|enum\s+\w+\s*\{.*?\};|extern\s+\"C\"\s*\{", "", text, flags=re.S | re.M)
    protos = {}
    for stmt in filter(None, (x.strip() for x in rest.split(";"))):
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\(([^()]*)\)", stmt, flags=re.S)
        if not m:
            if stmt == "}":  # closes extern "C"
                continue
            raise ImportError(f"cannot parse declaration {stmt!r}")
        ret, name, args = m.groups()
        res = (None, None) if ret.strip() == "void" else _ctype(ret, structs, opaque, consts, typed, param=False)
        args = [] if args.strip() == "void" else [_ctype(a, structs, opaque, consts, typed, param=True) for a in args.split(",")]
        if res is None or None in args:
            raise ImportError(f"cannot type prototype {name}: {' '.join(stmt.split())!r}")
        protos[name] = (res[1], [t for _, t in args])
    return consts, structs, protos


class _CfgMethods(ctypes.Structure):
    def copy(self) -> "LtCfg":
        new = LtCfg()
        ctypes.memmove(ctypes.byref(new), ctypes.byref(self), ctypes.sizeof(self))
        # (compat/cfg_translate.py: user terms for the slow torch path - Python attributes beside the C struct)
        for attr in ("extra_reward_terms", "extra_termination_terms", "extra_observation_terms", "reward_term_params"):
            if hasattr(self, attr):
                v = getattr(self, attr)
                setattr(new, attr, dict(v) if isinstance(v, dict) else list(v))
        return new

    def to_dict(self) -> dict:
        """Plain-Python form (scalars and nested lists) for params/env.{yaml,pkl}."""
        def py(v):
            return [py(x) for x in v] if hasattr(v, "__len__") else v

        return {name: py(getattr(self, name)) for name, *_ in self._fields_ if not name.startswith("_")}


# Entry points of lt_env.h that return a VALUE, not an LT_* status (the header's types cannot tell the two apart): never through `call`.
_ENV_VALUE_QUERIES = (
    "lt_abi_version", "lt_cfg_sizeof", "lt_cfg_num_presets", "lt_cfg_preset_id", "lt_cfg_obs_dim", "lt_cfg_tactile_dim", "lt_last_error",
    "lt_wgrad_splits", "lt_wgrad_ws_floats", "lt_elu_backward_bias_ws_floats", "lt_head_wgrad_ws_floats", "lt_adam_clip_step_ws_floats",
    "lt_elu_backward_bias_nblk", "lt_head_wgrad_nblk", "lt_mlp_backward_blocks", "lt_env_kernel_name", "lt_mlp_kernel_name")

# THE TABLE: one row per header of the C ABI, bound in this order.  A row is (public prefix, file under include/, whether the header may
# use lt_env.h's structures - or the file name of an EARLIER row whose structures it uses -, its value queries, the structures published
# as Lt* classes).  A header with prefix P is published as
# P_HEADER (its path), P_CONSTS, P_SIGNATURES and P_VALUE_QUERIES; lt_env.h has no prefix (HEADER, CONSTS, SIGNATURES, VALUE_QUERIES,
# and STRUCTS, EXPORTS).  Every header's LT_* constants are module globals as well.  Adding a header is adding a row.
HEADERS = (
    ("", "lt_env.h", False, _ENV_VALUE_QUERIES, ("lt_cfg", "lt_view", "lt_mlp_desc", "lt_render_view", "lt_render_desc")),
    ("OBS_NORM", "lt_obs_norm.h", False, (), ()),  # the observation normaliser
    ("STUDENT", "lt_student.h", True, ("lt_student_step_launches",), ("lt_student_desc", "lt_student_params")),  # the fused student inference step
    ("COLLECT", "lt_collect.h", False, (), ()),  # the tactile delay line and the step recording
    ("LEDGER", "lt_ledger.h", False, (), ()),  # the episode ledger of collection and evaluation; LEDGER_CONSTS: the head's field indices
    ("CNN_TRAIN", "lt_cnn_train.h", False, ("lt_cnn_launches",), ("lt_cnn_desc", "lt_cnn_params", "lt_cnn_grads")),  # the tactile CNN head, training form
    ("BC", "lt_bc.h", False, (), ()),  # batch assembly, masked loss and AdamW of the student's BC step; BC_CONSTS: the stats record's field indices
    ("LSTM", "lt_lstm.h", False, (), ()),  # the LSTM recurrence over whole trajectories
    ("MEMORY", "lt_memory.h", False, (), ("lt_memory_net",)),  # one rollout step of a recurrent policy's two LSTM memories
    ("MEMORY_SEQ", "lt_memory_seq.h", False, ("lt_memory_seq_backward_units",), ("lt_memory_seq_net", "lt_memory_seq_grad")),  # the two memories over a whole rollout
    ("MEMORY_GRU", "lt_memory_gru.h", False, ("lt_memory_gru_seq_backward_units",),
     ("lt_memory_gru_net", "lt_memory_gru_seq_net", "lt_memory_gru_seq_grad")),  # GRU memories, one rollout step and whole rollouts
    ("MEMORY_DX", "lt_memory_dx.h", False, ("lt_memory_input_grad_launches",), ("lt_memory_dx_net",)),  # the input gradient of a recurrent policy's two memories
    ("POLICY", "lt_policy.h", True, ("lt_policy_step_launches",), ("lt_policy_desc", "lt_policy_memory")),  # one inference step of a recurrent policy
    ("PPO_OPTS", "lt_ppo_opts.h", False, (), ()),  # the log-std policy and per-minibatch advantage statistics
    ("MLP_DX", "lt_mlp_dx.h", True, (), ()),  # the input gradient of the actor and critic stacks (recurrent policies: the memories' dout)
    ("PPO_SYM", "lt_ppo_sym.h", False, (), ()),  # the mirror-symmetric PPO update: table pack, row gather, the augmented batch's loss
    ("PPO_MIRROR", "lt_ppo_mirror.h", False, (), ()),  # the loss of the mirror-loss-only (and logging-only) symmetric update
    ("MLP_ROWS", "lt_mlp_rows.h", True, (), ()),  # the pair forward and backward chain with a row count per network
    ("ENCODER", "lt_encoder.h", False, ("lt_encoder_forward_launches",), ("lt_encoder_desc", "lt_encoder_net")),  # the encoder in front of an ActorCriticEncoder's stacks
    ("RNN_ENCODER", "lt_rnn_encoder.h", False, ("lt_rnn_encoder_forward_launches",),
     ("lt_rnn_encoder_memory", "lt_rnn_encoder_net")),  # an ActorCriticRNNEncoder's rollout: the memory step on strided rows, the encoder on the memory's output
    ("RNN_ENCODER_TRAIN", "lt_rnn_encoder_train.h", "lt_rnn_encoder.h", ("lt_rnn_encoder_backward_launches",),
     ("lt_rnn_encoder_grad",)),  # an ActorCriticRNNEncoder's update: the encoder's training form and its backward pass
    ("POLICY_ENCODER", "lt_policy_encoder.h", False, ("lt_policy_encoder_step_launches",),
     ("lt_policy_encoder_desc", "lt_policy_encoder_params")),  # one inference step of an ActorCriticEncoder / ActorCriticRNNEncoder
    ("TACTILE_PANEL", "lt_tactile_panel.h", False, ("lt_tactile_panel_launches",),
     ("lt_panel_signal", "lt_panel_desc")),  # the taxel panel drawn over rendered frames (--video_tactile)
    ("TELEMETRY", "lt_telemetry.h", False, ("lt_telemetry_record_launches", "lt_telemetry_chart_launches"),
     ("lt_telemetry_channel", "lt_chart_plot", "lt_chart_desc")),  # the per-step telemetry ring and its strip charts (--telemetry, --video_telemetry)
    ("EPISODE_STATS", "lt_episode_stats.h", "lt_telemetry.h", ("lt_episode_stats_step_launches", "lt_episode_stats_reduce_launches"),
     ("lt_episode_stats_pair", "lt_episode_stats_metric")),  # statistics over the finished episodes of all envs (--episode_stats)
)


def _bind(table, include_dir):
    """Parse every header of `table` (rows as in HEADERS), in order: one (path, constants, structures, signatures, value queries) per row.
    ImportError, naming the header and the entry point, if a value query of the row is not declared in its header, if an entry point
    returns no int (in lt_env.h: one that is no value query - there a query may return a size or a string), or if a name repeats one of an
    earlier header."""
    bound, seen, env_structs, structs_of = [], set(), None, {}
    for prefix, fname, uses_env_structs, queries, _ in table:
        path, queries = os.path.join(include_dir, fname), frozenset(queries)
        given = structs_of[uses_env_structs] if isinstance(uses_env_structs, str) else env_structs if uses_env_structs else None
        consts, structs, sigs = parse_header(open(path).read(), structs=given, bases={"lt_cfg": _CfgMethods})
        structs_of[fname] = structs
        if not prefix:
            env_structs = structs
        for name in sorted(queries - set(sigs)):
            raise ImportError(f"include/{fname}: the value query {name} named in _abi.HEADERS is not declared there")
        for name, (restype, _) in sigs.items():
            if name in seen:
                raise ImportError(f"include/{fname}: {name} repeats an entry point of an earlier header")
            if restype is not ctypes.c_int and (prefix or name not in queries):
                raise ImportError(f"include/{fname}: {name} returns no int (a new value query of lt_env.h belongs in _abi.HEADERS)")
        seen.update(sigs)
        bound.append((path, consts, structs, sigs, queries))
    return bound


ALL_SIGNATURES: dict = {}  # every header's entry points in one map (no name repeats: _bind), and the value queries among them
ALL_VALUE_QUERIES: set = set()
for (_prefix, _, _, _, _published), (_path, _consts, _structs, _sigs, _queries) in zip(HEADERS, _bind(HEADERS, os.path.join(REPO, "include"))):
    _p = _prefix + "_" if _prefix else ""
    globals().update(_consts)
    globals().update({_p + "HEADER": _path, _p + "CONSTS": _consts, _p + "SIGNATURES": _sigs, _p + "VALUE_QUERIES": _queries})
    globals().update({_structs[_c].__name__: _structs[_c] for _c in _published})  # lt_cfg -> LtCfg
    if not _prefix:
        STRUCTS, EXPORTS = _structs, list(_sigs)
    ALL_SIGNATURES.update(_sigs)
    ALL_VALUE_QUERIES |= _queries

_lib = None
_calls: dict = {}  # status-returning entry point -> (function, per-argument converter or None), filled by load()


def load() -> ctypes.CDLL:
    """Load liblocotouch_env.so (built in-tree by locotouch_amd.build).  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP extension is mandatory, there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ALL_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
        if name not in ALL_VALUE_QUERIES:
            _calls[name] = (fn, [ptr if t is ctypes.c_void_p else _ref if issubclass(t, ctypes._Pointer) and issubclass(t._type_, ctypes.Structure)
                                 else None for t in argtypes])
    if lib.lt_cfg_sizeof() != ctypes.sizeof(LtCfg):
        raise ImportError(f"lt_cfg ABI mismatch: C {lib.lt_cfg_sizeof()} vs ctypes {ctypes.sizeof(LtCfg)}")
    if lib.lt_abi_version() != CONSTS["LT_ABI_VERSION"]:
        raise ImportError("lt_env.h / liblocotouch_env.so ABI version mismatch")
    _lib = lib
    return lib


def ptr(x):
    """c_void_p of a tensor's data_ptr(), of an integer address (0 -> NULL) or of None (NULL); a ctypes object passes through."""
    if x is None or isinstance(x, int):
        return ctypes.c_void_p(x or None)
    data_ptr = getattr(x, "data_ptr", None)
    return ctypes.c_void_p(data_ptr()) if data_ptr else x


def _ref(x):
    return ctypes.byref(x) if isinstance(x, ctypes.Structure) else x


def stream(device=None) -> ctypes.c_void_p:
    """torch's current stream on `device` as the `void* stream` argument of a launch."""
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr_array(tensors):
    """HOST array of device pointers (None entries -> NULL): the `const float* const*` operands."""
    return (ctypes.c_void_p * max(1, len(tensors)))(*[None if t is None else t.data_ptr() for t in tensors])


def call(name: str, *args) -> None:
    """Call a status-returning entry point: tensors / addresses / None become pointers, structures are passed by reference
    (which positions: decided once per function in load(), from the header), and a non-zero status raises with lt_last_error()."""
    try:
        fn, conv = _calls[name]
    except KeyError:
        if name in ALL_VALUE_QUERIES:
            raise TypeError(f"{name} returns a value, not a status: call load().{name}(...)") from None
        if _lib is not None:
            raise
        load()
        fn, conv = _calls[name]
    rc = fn(*[a if c is None else c(a) for c, a in zip(conv, args, strict=True)])
    if rc:
        check(rc, name)


def preset_ids() -> list[str]:
    lib = load()
    return [lib.lt_cfg_preset_id(i).decode() for i in range(lib.lt_cfg_num_presets())]


def preset_cfg(gym_id: str, num_envs: int | None = None, seed: int | None = None) -> LtCfg:
    """Resolved lt_cfg of a registered gym id (lt_cfg_preset)."""
    cfg = LtCfg()
    rc = load().lt_cfg_preset(gym_id.encode(), ctypes.byref(cfg))
    if rc != 0:
        raise KeyError(f"unknown task {gym_id!r}; registered: {preset_ids()}")
    if num_envs is not None:
        cfg.num_envs = int(num_envs)
    if seed is not None:
        cfg.seed = int(seed)
    return cfg


def default_cfg(task: int, num_envs: int | None = None, seed: int | None = None) -> LtCfg:
    cfg = LtCfg()
    rc = load().lt_cfg_default(task, ctypes.byref(cfg))
    if rc != 0:
        raise ValueError(f"lt_cfg_default({task}) failed: {rc}")
    if num_envs is not None:
        cfg.num_envs = num_envs
    if seed is not None:
        cfg.seed = seed
    return cfg


def check(rc: int, what: str) -> None:
    if rc != 0:
        err = load().lt_last_error()
        raise RuntimeError(f"{what} failed with code {rc}: {err.decode() if err else ''}")
