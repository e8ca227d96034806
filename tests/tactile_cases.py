"""Planted contact lines for the tactile pass, and the judge that holds a candidate (lt_tactile_kernel, or a mutated oracle) to the
f32 and f64 oracle builds run from the same planted arena.  No GPU import: tests/test_tactile_cases.py checks the table and the
judge on the CPU, tests/test_hip_tactile.py runs the kernel through them.

A line is 12 floats, x[4], y[4], f[4]: four collinear samples in the trunk frame and their normal forces, the row layout of
`Layout.set_vec(arena, "LT_F_PLATE_SAMPLES", ...)`.  The geometry only reads samples 0 and 3."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from locotouch_amd import _abi
from locotouch_amd.layout import Layout
from tests import oracle_lib as O
from tests.parity_util import F64_RATIO, F64_ULPS

C = _abi.CONSTS
STUDENT = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"
ROWS, COLS = C["LT_TACTILE_ROWS"], C["LT_TACTILE_COLS"]
NT = ROWS * COLS
WIDE = C["LT_TACTILE_WIDE_DIM"]
X0, Y0, DX, DY, HX, HY = 0.1144, 0.0768, 0.0143, 0.0128, 0.00915, 0.00875  # include/lt_go1_model.h LT_TAXEL_*
GROUP_FIELDS = ("LT_F_OBS_TACTILE", "LT_F_OBS_TACTILE_ORIGINAL", "LT_F_OBS_TACTILE_PROCESSED")  # term 0, 1, 2
CHANNELS = ("contact", "norm", "minmax", "disc")
SECOND = {"LT_TACTILE_BINARY": "contact", "LT_TACTILE_NORMALIZED": "minmax", "LT_TACTILE_DISCRETE": "disc", "LT_TACTILE_CONTINUOUS": "norm"}
FMT_NAME = {C[k]: k for k in ("LT_TACTILE_BINARY", "LT_TACTILE_NORMALIZED", "LT_TACTILE_DISCRETE", "LT_TACTILE_CONTINUOUS",
                              "LT_TACTILE_PROCESSED", "LT_TACTILE_ORIGINAL")}
# cap on what the references may exclude, per case group: a condition on the table, not a measurement
MAX_EXCLUDED_FRAC, MAX_EXCLUDED_ENVS = 0.005, 1

PARAM_SETS = {
    "registered": {},
    "off": dict(tactile_threshold_noise=0.0, tactile_dropout_prob=0.0, tactile_addition_prob=0.0, tactile_force_noise=0.0,
                tactile_level_noise=0.0),
    "heavy": dict(tactile_dropout_prob=0.3, tactile_addition_prob=0.3),
    "alllit": dict(tactile_addition_prob=1.0),
}


def centre(row: int, col: int):
    return X0 - DX * row, Y0 - DY * col


def line(p0, p3, f) -> np.ndarray:
    """Four evenly spaced samples from p0 to p3 with forces f[4]."""
    p = np.linspace(np.asarray(p0, np.float64), np.asarray(p3, np.float64), 4)
    return np.concatenate([p[:, 0], p[:, 1], np.asarray(f, np.float64)]).astype(np.float32)


def _directed():
    even = [0.5, 1.0, 1.0, 0.5]  # a constant line pressure (the end cells are half cells), 3 N in all
    c86, c43 = centre(8, 6), centre(4, 3)
    ob0, ob3 = (0.0712, -0.0533), (-0.0551, 0.0467)  # oblique, inside the grid, crosses ~20 boxes and both kinds of overlap
    cases = [
        ("unloaded", line((0.05, -0.03), (-0.02, 0.04), [0, 0, 0, 0])),
        ("all_negative", line((0.05, -0.03), (-0.02, 0.04), [-1, -2, -0.5, -1])),
        ("mixed_sign", line((0.05, -0.03), (-0.02, 0.04), [-1.5, 0.8, -0.3, 1.1])),
        # collapsed to a point (length 0): 1, 2 and 4 boxes hold it, or none
        ("point_centre", line(c86, c86, even)),
        ("point_y_overlap", line((c86[0], c86[1] - DY / 2), (c86[0], c86[1] - DY / 2), even)),
        ("point_corner4", line((c86[0] - DX / 2, c86[1] - DY / 2), (c86[0] - DX / 2, c86[1] - DY / 2), even)),
        ("point_off_sensor", line((0.2, 0.0), (0.2, 0.0), even)),
        # (0.2 mm inside the x edge of row 4's box, past HALF_Y from its centre; also inside row 3's box)
        ("len_5e-7", line((c43[0] + 0.00895, c43[1] + 0.001), (c43[0] + 0.00895 + 5e-7, c43[1] + 0.001), even)),
        ("len_3e-6", line((c43[0] + 0.001, c43[1] + 0.001), (c43[0] + 0.001 + 2.1e-6, c43[1] + 0.001 + 2.1e-6), even)),
        # axis-parallel: the |dd| < 1e-9 branches
        ("along_y_row_centres", line((centre(5, 0)[0], -0.0631), (centre(5, 0)[0], 0.0417), even)),
        ("along_y_between_rows", line((centre(5, 0)[0] - DX / 2, -0.0631), (centre(5, 0)[0] - DX / 2, 0.0417), even)),
        ("along_x", line((-0.0907, centre(0, 9)[1] + 0.0011), (0.0623, centre(0, 9)[1] + 0.0011), [0.2, 1.4, 0.9, 0.6])),
        ("dx_1e-8", line((centre(11, 0)[0] + 0.0013, -0.0631), (centre(11, 0)[0] + 0.0013 + 1e-8, 0.0417), even)),
        ("oblique", line(ob0, ob3, [0.3, 1.2, 0.7, 0.9])),
        ("oblique_reversed", line(ob3, ob0, [0.9, 0.7, 1.2, 0.3])),
        ("one_end_off", line((0.02, 0.03), (0.1612, -0.0214), [0.6, 1.1, 0.8, 0.4])),
        ("both_ends_off", line((-0.1523, -0.0312), (0.1489, 0.0287), [0.4, 1.3, 1.0, 0.7])),
        ("wholly_off", line((0.14, -0.05), (0.19, 0.06), even)),
        ("clamp_4x20N", line((0.0712, -0.0533), (0.0208, -0.0134), [20, 20, 20, 20])),
        # taxel forces of 0.03 .. 0.07 N around the 0.05 N threshold (and its +-0.01 N noise)
        ("straddle_threshold", line((0.0834, -0.0611), (-0.0797, 0.0589), [0.05, 0.25, 0.3, 0.12])),
        ("load_on_one_end", line(ob0, ob3, [0, 0, 0, 2.5])),
        ("corner_taxel_0", line((centre(0, 0)[0] - 0.003, centre(0, 0)[1] - 0.002), (centre(0, 0)[0] + 0.004, centre(0, 0)[1] + 0.003), even)),
        ("corner_taxel_220", line((centre(16, 12)[0] + 0.003, centre(16, 12)[1] + 0.002), (centre(16, 12)[0] - 0.004, centre(16, 12)[1] - 0.003), even)),
    ]
    names = [nm for nm, _ in cases]
    assert len(set(names)) == len(names)
    return names, np.stack([v for _, v in cases])


DIRECTED_NAMES, DIRECTED = _directed()


def _random(count: int) -> np.ndarray:
    """Endpoints past the sensor on every side (it spans |x| <= 0.1236, |y| <= 0.0856); sample forces u^2 * U(0, 6) N."""
    rng = np.random.default_rng(1)
    out = np.zeros((count, 12), np.float32)
    for i in range(count):
        p0 = (rng.uniform(-0.12, 0.13), rng.uniform(-0.09, 0.09))
        p3 = (rng.uniform(-0.12, 0.13), rng.uniform(-0.09, 0.09))
        f = rng.uniform(0.0, 1.0, 4) ** 2 * rng.uniform(0.0, 6.0, 4)
        out[i] = line(p0, p3, f)
    return out


RANDOM = _random(512)


def mixed_lines(n: int):
    """The directed lines, then random ones up to n rows; with the env ranges of both case groups."""
    k = len(DIRECTED)
    assert n > k
    return np.concatenate([DIRECTED, RANDOM[: n - k]]), {"directed": np.arange(k), "random": np.arange(k, n)}


def make_cfg(n: int, params: str = "registered", fmt: str = "LT_TACTILE_BINARY", aux: int = 0, offset: int = 0, seed: int = 11):
    cfg = _abi.preset_cfg(STUDENT, num_envs=n, seed=seed)
    for k, v in PARAM_SETS[params].items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    cfg.tactile_format, cfg.tactile_aux_groups, cfg.env_index_offset = C[fmt], aux, offset
    return cfg


def layout(cfg) -> Layout:
    wide = int(cfg.tactile_format) in (C["LT_TACTILE_PROCESSED"], C["LT_TACTILE_ORIGINAL"])
    obs_dim = (45 if cfg.task == C["LT_TASK_LOCOMOTION"] else 58) * int(cfg.obs_history)
    return Layout(int(cfg.num_envs), obs_dim, int(cfg.tactile_enabled), WIDE if wide else C["LT_TACTILE_DIM"])


def terms_of(cfg):
    return [0] + [t for t in (1, 2) if int(cfg.tactile_aux_groups) & t]


def plant(cfg, lines: np.ndarray, step: int = 1) -> np.ndarray:
    """A host arena after the oracle's reset_all, with `lines` as the plate samples and `step` as the step counter."""
    n = int(cfg.num_envs)
    assert lines.shape == (n, 12) and lines.dtype == np.float32
    ora = O.OracleEnv(cfg)
    ora.reset_all()
    L = layout(cfg)
    L.set_vec(ora.arena, "LT_F_PLATE_SAMPLES", lines)
    L.arr(ora.arena, "LT_F_COUNTERS")[0] = step
    return ora.arena


def run_lib(lib, cfg, arena: np.ndarray) -> np.ndarray:
    """lt_oracle_tactile_update of `lib` (an oracle build, or a mutant of it) on a copy of `arena`."""
    out = arena.copy()
    c = cfg.copy()
    lib.lt_oracle_tactile_update(ctypes.byref(c), out.ctypes.data_as(ctypes.c_void_p))
    return out


def run_oracles(cfg, planted: np.ndarray):
    return run_lib(O.load("f32"), cfg, planted), run_lib(O.load("f64"), cfg, planted)


def thresholds(cfg) -> dict:
    """{term: [n][221]} from lt_oracle_tactile_thresholds (f32 in both builds, like the channel pipeline)."""
    n, lib, c = int(cfg.num_envs), O.load("f32"), cfg.copy()
    out = {}
    for term in terms_of(cfg):
        thr = np.zeros((n, NT), np.float32)
        for e in range(n):
            lib.lt_oracle_tactile_thresholds(ctypes.byref(c), term, e, O.fptr(thr[e]))
        out[term] = thr
    return out


def taxel_forces(lines: np.ndarray, precision: str) -> np.ndarray:
    """[n][221] pre-noise taxel forces in newtons (lt_oracle_taxel_forces; computed in `precision`, returned as f32)."""
    lib, out = O.load(precision), np.zeros((len(lines), NT), np.float32)
    for e, ln in enumerate(np.ascontiguousarray(lines, np.float32)):
        lib.lt_oracle_taxel_forces(O.fptr(ln[0:4]), O.fptr(ln[4:8]), O.fptr(ln[8:12]), O.fptr(out[e]))
    return out


def emitted(cfg, arena: np.ndarray, term: int) -> dict:
    """{channel: [n][221]} that term instance `term` writes under cfg (BINARY's second channel is 'contact2')."""
    n, L = int(cfg.num_envs), layout(cfg)
    rows = L.arr(arena, GROUP_FIELDS[term])[:n]
    if rows.shape[1] == WIDE:
        return {ch: rows[:, k * NT:(k + 1) * NT] for k, ch in enumerate(CHANNELS)}
    second = SECOND[FMT_NAME[int(cfg.tactile_format)]]
    return {"contact": rows[:, :NT], ("contact2" if second == "contact" else second): rows[:, NT:]}


def wide_cfg(cfg):
    """The same cfg with the `tactile` group in the 4-channel format of its own pipeline: term 0 draws from the same streams, so
    this run of an oracle supplies the channels a two-channel format does not emit."""
    c = cfg.copy()
    c.tactile_format = C["LT_TACTILE_ORIGINAL"] if int(cfg.tactile_format) == C["LT_TACTILE_ORIGINAL"] else C["LT_TACTILE_PROCESSED"]
    return c


def wide_channels(cfg, arena: np.ndarray, precision: str) -> dict:
    """{term: {channel: [n][221]}}: all four channels of every enabled term, from the samples and counter of `arena`."""
    cw = wide_cfg(cfg)
    out = run_lib(O.load(precision), cw, arena)
    return {term: emitted(cw, out, term) for term in terms_of(cfg)}


def plate_lines(cfg, arena: np.ndarray) -> np.ndarray:
    return layout(cfg).vec(arena, "LT_F_PLATE_SAMPLES")


def written_mask(cfg) -> np.ndarray:
    """Over the 3 * npad * 884 floats of the tactile blocks: what the pass writes (rows [0, n) of the enabled groups, at the `tactile`
    group's own row width)."""
    n, L = int(cfg.num_envs), layout(cfg)
    m = np.zeros((3, L.npad * WIDE), bool)
    m[0, : n * L.tactile_dim] = True
    for term in (1, 2):
        if int(cfg.tactile_aux_groups) & term:
            m[term, : n * WIDE] = True
    return m.reshape(-1)


def tactile_blocks(cfg, arena: np.ndarray) -> np.ndarray:
    """Flat float view of the three tactile blocks inside `arena`."""
    L = layout(cfg)
    off = L.plain["LT_F_OBS_TACTILE"][0]
    return arena[off:off + 3 * L.npad * WIDE * 4].view(np.float32)


class Judged:
    """Per case group: lit taxels, exclusions against the cap, and the errors against the f64 oracle."""

    def __init__(self, what):
        self.what, self.groups, self.failures = what, {}, []

    def lines(self):
        out = []
        for g, s in self.groups.items():
            ratio = f"{s['e_cand'] / s['e_o32']:.2f}" if s["e_o32"] > 0 else ("-" if s["e_cand"] == 0 else "inf")
            out.append(f"[tactile] {self.what} / {g}: envs {s['envs']} lit {s['lit']} excluded taxel-terms {s['excluded']}/{s['taxel_terms']} "
                       f"(cap {s['cap']}) excluded envs {s['excluded_envs']} (cap {MAX_EXCLUDED_ENVS}) | vs f64: cand {s['e_cand']:.3e} "
                       f"o32 {s['e_o32']:.3e} ratio {ratio} worst cand/bound {s['frac']:.3f} | compared {s['compared']}")
        return out


def judge(cfg, cand: np.ndarray, o32: np.ndarray, o64: np.ndarray, thr: dict, groups: dict | None = None, what: str = "",
          check: bool = True) -> Judged:
    """Hold the tactile rows of `cand` to the oracles' (all three arenas run from the same planted arena).

    Continuous channels, per env and channel: |cand - o64| <= F64_RATIO * max|o32 - o64| + F64_ULPS * 2^-24 * max(1, sum f+ / maximal_force).
    Contact bits and noise-free levels: equal to the f32 oracle's, with zero allowance outside the exclusion set, which is computed
    from the references alone; noisy levels within the continuous bound / total_levels of the f32 oracle's.  The exclusion set is
    capped per case group.  Raises AssertionError (after collecting every failure) unless `check` is False."""
    n = int(cfg.num_envs)
    groups = groups or {"all": np.arange(n)}
    res = Judged(what)
    lines = plate_lines(cfg, o64)
    assert (lines == plate_lines(cfg, o32)).all() and (lines == plate_lines(cfg, cand)).all(), "the three arenas must hold the same planted lines"
    maxf, levels = float(cfg.tactile_maximal_force), int(cfg.tactile_total_levels)
    noisy_levels = float(cfg.tactile_level_noise) > 0
    f64 = taxel_forces(lines, "f64").astype(np.float64)
    mag = np.maximum(1.0, np.maximum(lines[:, 8:12].astype(np.float64), 0).sum(axis=1) / maxf)  # pre-subtraction size of pressure_integral
    floor = F64_ULPS * 2.0 ** -24 * mag
    w32, w64 = wide_channels(cfg, o32, "f32"), wide_channels(cfg, o64, "f64")
    terms = terms_of(cfg)
    acc = {g: dict(envs=len(ix), lit=0, excluded=0, taxel_terms=len(ix) * len(terms) * NT, cap=int(MAX_EXCLUDED_FRAC * len(ix) * len(terms) * NT),
                   ex_envs=set(), e_cand=0.0, e_o32=0.0, frac=0.0, compared=0) for g, ix in groups.items()}
    fail = res.failures
    for term in terms:
        a32, a64 = {k: v.astype(np.float64) for k, v in w32[term].items()}, {k: v.astype(np.float64) for k, v in w64[term].items()}
        e_norm = np.abs(a32["norm"] - a64["norm"]).max(axis=1)
        e_mm = np.abs(a32["minmax"] - a64["minmax"]).max(axis=1)
        bound = {"norm": F64_RATIO * e_norm + floor, "minmax": F64_RATIO * e_mm + floor}
        # -- the exclusion set, from the references alone
        ex_contact = (np.abs(f64 - thr[term].astype(np.float64)) <= (bound["norm"] * maxf)[:, None]) | (a32["contact"] != a64["contact"])
        ex_env = ex_contact.any(axis=1)
        x = a64["minmax"] * levels
        ex_level = np.abs(x - np.floor(x) - 0.5) <= (bound["minmax"] * levels)[:, None]
        if noisy_levels:
            ex_level |= np.abs(a32["disc"] - a64["disc"]) > (bound["minmax"] / levels)[:, None]
        else:
            ex_level |= a32["disc"] != a64["disc"]
        ex_level &= (a64["contact"] != 0) | (a32["contact"] != 0)  # levels of taxels out of contact are 0 whatever the min-max
        keep = {"contact": ~ex_contact, "contact2": ~ex_contact, "norm": ~ex_contact,
                "minmax": np.broadcast_to(~ex_env[:, None], (n, NT)), "disc": ~ex_env[:, None] & ~ex_level}
        ec, e32, e64 = emitted(cfg, cand, term), emitted(cfg, o32, term), emitted(cfg, o64, term)
        for ch in e32:  # the wide rerun must restate what the judged oracle arenas hold
            assert (e32[ch] == w32[term][ch.rstrip("2")]).all() and (e64[ch] == w64[term][ch.rstrip("2")]).all(), (term, ch)
        for ch, c in ec.items():
            if not np.isfinite(c).all():
                fail.append(f"term {term} {ch}: non-finite values in envs {np.nonzero(~np.isfinite(c).all(axis=1))[0][:5].tolist()}")
                c = np.nan_to_num(c, nan=-1.0, posinf=-1.0, neginf=-1.0)
            k = keep[ch]
            c64, r32, r64 = c.astype(np.float64), e32[ch].astype(np.float64), e64[ch].astype(np.float64)
            if ch in ("contact", "contact2"):
                if not np.isin(c, (0.0, 1.0)).all():
                    fail.append(f"term {term} {ch}: values outside {{0, 1}}")
                bad = k & (c64 != r32)
                err = None
            elif ch == "disc" and not noisy_levels:
                bad = k & (c64 != r32)
                err = None
            elif ch == "disc":
                bad = k & ~(np.abs(c64 - r32) <= (bound["minmax"] / levels)[:, None])
                err = None
            else:
                err, err32 = np.where(k, np.abs(c64 - r64), 0.0), np.where(k, np.abs(r32 - r64), 0.0)
                bad = k & ~(err <= bound[ch][:, None])
            for g, ix in groups.items():
                s = acc[g]
                s["compared"] += int(k[ix].sum())
                if err is not None and len(ix):
                    s["e_cand"], s["e_o32"] = max(s["e_cand"], float(err[ix].max())), max(s["e_o32"], float(err32[ix].max()))
                    s["frac"] = max(s["frac"], float((err[ix] / bound[ch][ix, None]).max()))
                if bad[ix].any():
                    e, t = [v[0] for v in np.nonzero(bad[ix])]
                    fail.append(f"group {g} term {term} {ch}: {int(bad[ix].sum())} mismatches in {int(bad[ix].any(axis=1).sum())} envs; first env {int(ix[e])} "
                                f"taxel {int(t)}: cand {c[ix[e], t]!r} o32 {e32[ch][ix[e], t]!r} o64 {e64[ch][ix[e], t]!r}"
                                + (f" bound {bound[ch][ix[e]]:.3e}" if ch in bound else ""))
        for g, ix in groups.items():
            s = acc[g]
            s["excluded"] += int((ex_contact[ix] | (ex_level[ix] & ~ex_env[ix, None])).sum())
            s["ex_envs"] |= set(ix[ex_env[ix]].tolist())
            if term == 0:
                s["lit"] = int(a32["contact"][ix].sum())
    for g, s in acc.items():
        s["excluded_envs"] = len(s.pop("ex_envs"))
        if s["excluded"] > s["cap"] or s["excluded_envs"] > MAX_EXCLUDED_ENVS:
            fail.append(f"group {g}: the references exclude {s['excluded']} taxel-terms (cap {s['cap']}) and {s['excluded_envs']} envs (cap {MAX_EXCLUDED_ENVS})")
        res.groups[g] = s
    if check and fail:
        raise AssertionError("\n".join([f"tactile judge {what}: {len(fail)} failures"] + fail + res.lines()))
    return res


@functools.lru_cache(maxsize=None)
def reference_run(n: int, params: str, fmt: str, aux: int, offset: int = 0, step: int = 1, lines: str = "mixed"):
    """(cfg, planted arena, o32, o64, thresholds, groups) of one run of the table; computed once per process and not to be written to.
    `lines`: 'mixed' (the directed lines, then random ones), 'random', 'random@K' (random lines K ...), 'unloaded'."""
    cfg = make_cfg(n, params, fmt, aux, offset)
    if lines == "mixed":
        rows, groups = mixed_lines(n)
    elif lines == "unloaded":
        rows, groups = np.repeat(DIRECTED[DIRECTED_NAMES.index("unloaded")][None], n, axis=0), {"unloaded": np.arange(n)}
    else:
        k = int(lines.partition("@")[2] or 0)
        rows, groups = RANDOM[k:k + n], {"random": np.arange(n)}
    planted = plant(cfg, np.ascontiguousarray(rows), step)
    o32, o64 = run_oracles(cfg, planted)
    for a in (planted, o32, o64):
        a.setflags(write=False)
    return cfg, planted, o32, o64, thresholds(cfg), groups
