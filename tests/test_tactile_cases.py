"""The planted-line table and the judge of tests/tactile_cases.py on the CPU: the references alone meet the exclusion cap, the f32
oracle passes as a candidate, the table reaches the branches it claims (counted), and the judge rejects every listed mutant of the
oracle, each built at test time from a textual replacement in a copy of oracle/lt_oracle.c."""
import ctypes
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import tactile_cases as T

P, G = "LT_TACTILE_PROCESSED", "LT_TACTILE_ORIGINAL"
# (n, params, format, aux, env_index_offset, step, lines): n = 37 has npad = 48, so the aux blocks do not start at n * 884
RUNS = [(37, ps, P, 3, 0, 1, "mixed") for ps in T.PARAM_SETS] + [
    (37, "registered", G, 3, 0, 1, "mixed"),
    (37, "heavy", "LT_TACTILE_BINARY", 0, 0, 1, "mixed"),
    (37, "heavy", "LT_TACTILE_DISCRETE", 2, 0, 1, "mixed"),
    (37, "registered", "LT_TACTILE_NORMALIZED", 1, 0, 1, "mixed"),
    (37, "off", "LT_TACTILE_CONTINUOUS", 0, 0, 1, "mixed"),
    (37, "registered", P, 3, 368, 1, "random@368"),
    (37, "heavy", P, 3, 0, 2 ** 33 + 7, "mixed"),
    (1, "alllit", P, 3, 0, 1, "random"),
    (128, "registered", P, 3, 0, 1, "random"), (128, "off", P, 3, 0, 1, "random"), (128, "heavy", P, 3, 0, 1, "random"),
]


def run_id(r):
    return f"n{r[0]}-{r[1]}-{r[2][11:].lower()}-aux{r[3]}" + (f"-off{r[4]}" if r[4] else "") + (f"-step{r[5]}" if r[5] != 1 else "") + f"-{r[6]}"


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_references_meet_the_cap_and_the_f32_oracle_passes(run):
    cfg, _, o32, o64, thr, groups = T.reference_run(*run)
    res = T.judge(cfg, o32, o32, o64, thr, groups, what=run_id(run))  # asserts the cap per group, too
    print("\n".join(res.lines()))
    for s in res.groups.values():
        assert s["compared"] > 0 and s["e_cand"] == s["e_o32"]
    # the f64 oracle is no candidate for the exact comparisons only where the references exclude: it passes as well
    T.judge(cfg, o64, o32, o64, thr, groups, what=run_id(run) + " (f64 as candidate)")


def test_directed_lines_reach_their_branches():
    """Lit counts under the all-off set (threshold exactly 0.05 N, no noise), case by case."""
    cfg, planted, o32, o64, thr, groups = T.reference_run(37, "off", P, 3, 0, 1, "mixed")
    contact = T.emitted(cfg, o32, 0)["contact"]
    norm = T.emitted(cfg, o32, 0)["norm"]
    lit = {nm: int(contact[i].sum()) for i, nm in enumerate(T.DIRECTED_NAMES)}
    print(lit)
    lines = T.plate_lines(cfg, planted)
    length = {nm: float(np.hypot(lines[i, 3] - lines[i, 0], lines[i, 7] - lines[i, 4])) for i, nm in enumerate(T.DIRECTED_NAMES)}
    for nm in ("unloaded", "all_negative", "point_off_sensor", "wholly_off"):
        assert lit[nm] == 0, nm
    # collapsed lines (len < 1e-6): the whole force on 1, 2 and 4 boxes
    for nm, k in (("point_centre", 1), ("point_y_overlap", 2), ("point_corner4", 4), ("len_5e-7", 2)):
        assert length[nm] < 1e-6 and lit[nm] == k, (nm, length[nm], lit[nm])
        i = T.DIRECTED_NAMES.index(nm)
        assert (norm[i][contact[i] != 0] == 1.0).all()  # 3 N on each box that holds the point = maximal_force
    assert 0 < length["len_5e-7"] and 1e-6 < length["len_3e-6"] < 4e-6 and lit["len_3e-6"] == 1
    dxs = {nm: float(lines[T.DIRECTED_NAMES.index(nm), 3] - lines[T.DIRECTED_NAMES.index(nm), 0]) for nm in T.DIRECTED_NAMES}
    dys = {nm: float(lines[T.DIRECTED_NAMES.index(nm), 7] - lines[T.DIRECTED_NAMES.index(nm), 4]) for nm in T.DIRECTED_NAMES}
    assert dxs["along_y_row_centres"] == 0 and dxs["along_y_between_rows"] == 0 and dys["along_x"] == 0
    assert 1e-9 < abs(dxs["dx_1e-8"]) < 3e-8  # takes the division
    grid = {nm: contact[i].reshape(T.ROWS, T.COLS) for i, nm in enumerate(T.DIRECTED_NAMES)}
    assert (grid["along_y_row_centres"].sum(axis=1) > 0).sum() == 1 and (grid["along_y_between_rows"].sum(axis=1) > 0).sum() == 2
    assert (grid["along_x"].sum(axis=0) > 0).sum() == 1 and (grid["dx_1e-8"].sum(axis=1) > 0).sum() == 1
    assert lit["oblique"] == lit["oblique_reversed"] >= 15 and (grid["oblique"] == grid["oblique_reversed"]).all()
    assert lit["mixed_sign"] > 0 and lit["one_end_off"] > 0 and lit["both_ends_off"] > 10 and lit["load_on_one_end"] > 0
    assert lit["load_on_one_end"] < lit["oblique"]
    i = T.DIRECTED_NAMES.index("clamp_4x20N")
    assert lit["clamp_4x20N"] > 3 and (norm[i] == 1.0).sum() >= 3
    f = T.taxel_forces(lines, "f64")[T.DIRECTED_NAMES.index("straddle_threshold")]
    assert ((f > 0.03) & (f < 0.05)).sum() >= 2 and ((f > 0.05) & (f < 0.07)).sum() >= 2, np.sort(f[f > 0])
    assert grid["corner_taxel_0"][0, 0] == 1 and grid["corner_taxel_220"][16, 12] == 1 and lit["corner_taxel_0"] <= 4 and lit["corner_taxel_220"] <= 4
    # no directed line within 0.2 mm of a box edge it runs parallel to; no collapsed point within 0.2 mm of any edge
    cx, cy = T.X0 - T.DX * np.arange(T.ROWS), T.Y0 - T.DY * np.arange(T.COLS)
    for i, nm in enumerate(T.DIRECTED_NAMES):
        x0, y0 = float(lines[i, 0]), float(lines[i, 4])
        if abs(dxs[nm]) < 1e-7 or length[nm] < 1e-6:
            assert np.abs(np.abs(x0 - cx) - T.HX).min() >= 0.0002 - 1e-7, nm
        if abs(dys[nm]) < 1e-7 or length[nm] < 1e-6:
            assert np.abs(np.abs(y0 - cy) - T.HY).min() >= 0.0002 - 1e-7, nm


def test_noise_branches_are_reached_and_counted():
    """All-lit: 221 contacts and a positive per-env minimum.  Heavy: dropped and added taxels, and the too-small repair, counted from
    the thresholds and the oracle's channels."""
    cfg, planted, o32, _, thr, _ = T.reference_run(1, "alllit", P, 3, 0, 1, "random")
    for term in (0, 2):
        ch = T.emitted(cfg, o32, term)
        assert ch["contact"].sum() == T.NT and ch["norm"].min() > 0  # mn > 0: the inactive lanes' identity decides the minimum
        assert ch["minmax"].min() == 0.0 and ch["minmax"].max() == 1.0
    cfg, planted, o32, _, thr, _ = T.reference_run(37, "heavy", P, 3, 0, 1, "mixed")
    forces = T.taxel_forces(T.plate_lines(cfg, planted), "f32")
    # the same draws without force noise: the pre-noise force g of every taxel.  With noise p the unrepaired output is g (1 + U(-p, p)),
    # so a contact taxel outside that band was repaired (a lower bound: a repaired value may also land inside the band)
    quiet = cfg.copy()
    quiet.tactile_force_noise = 0.0
    q32 = T.run_lib(O.load("f32"), quiet, planted)
    p, maxf = float(cfg.tactile_force_noise), float(cfg.tactile_maximal_force)
    assert p > 0
    dropped = added = repaired = 0
    for term in (0, 2):
        pre = forces > thr[term]
        ch, g = T.emitted(cfg, o32, term), T.emitted(quiet, q32, term)["norm"].astype(np.float64)
        contact = ch["contact"] != 0
        assert (contact == (T.emitted(quiet, q32, term)["contact"] != 0)).all()
        dropped += int((pre & ~contact).sum())
        added += int((~pre & contact).sum())
        out = ch["norm"].astype(np.float64)
        unclamped = contact & (g < 1.0) & (out < 1.0)
        repaired += int((unclamped & ((out > g * (1 + p) * (1 + 1e-5)) | (out < g * (1 - p) * (1 - 1e-5)))).sum())
        assert (out[contact] * maxf >= thr[term][contact] * (1 - 1e-6)).all()  # what the repair guarantees
    print(f"heavy set, 37 envs x 2 processed terms: dropped {dropped} added {added} repaired (lower bound) {repaired}")
    assert dropped >= 50 and added >= 50 and repaired >= 10


# ---- the judge can fail ------------------------------------------------------------------------------------------------------
MUTANTS = {
    "end_cells_as_full_cells": ("{f[0] / ((real)0.5 * dl), f[1] / dl, f[2] / dl, f[3] / ((real)0.5 * dl)}", "{f[0] / dl, f[1] / dl, f[2] / dl, f[3] / dl}"),
    "no_ta_tb_swap": ("if (ta > tb) { real tt = ta; ta = tb; tb = tt; }", ""),
    "half_y_on_both_axes": ("(real)fabs(x[0] - cx) <= LT_TAXEL_HALF_X", "(real)fabs(x[0] - cx) <= LT_TAXEL_HALF_Y"),
    "aux_block_from_n": ("const int64_t blk = L->npad * (int64_t)LT_TACTILE_WIDE_DIM;", "const int64_t blk = L->n * (int64_t)LT_TACTILE_WIDE_DIM;"),
    "key_without_env_index_offset": ("const uint32_t ekey = EKEY(cfg, e);", "const uint32_t ekey = (uint32_t)e;"),
    "minimum_seeded_with_0": ("float mn = 2.0f, mx = -1.0f;", "float mn = 0.0f, mx = -1.0f;"),
    "dropout_force_from_u_drop": ("{ f = u_dropf[t] * thr; contact = 0; }", "{ f = u_drop[t] * thr; contact = 0; }"),
    "repair_against_cfg_threshold": ("if (contact && f < thr) f = thr", "if (contact && f < cfg->tactile_threshold) f = thr"),
    "step_key_32_bits": ("const uint64_t step = (uint64_t)((int64_t*)((char*)arena + L->off_counters))[0];",
                         "const uint64_t step = (uint32_t)((int64_t*)((char*)arena + L->off_counters))[0];"),
    "level_noise_after_bin": (re.compile(r"(    if \(cfg->tactile_level_noise > 0\) d \+= [^\n]*\n)(    d \*= bin;\n)"), r"\2\1"),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """{name: CDLL}: f32 builds of the mutated source with the Makefile's compiler flags, compiled side by side."""
    odir = os.path.join(O.REPO, "oracle")
    src = open(os.path.join(odir, "lt_oracle.c")).read()
    cflags = re.search(r"^CFLAGS \?= (.*)$", open(os.path.join(odir, "Makefile")).read(), re.M).group(1).split()
    tmp = tmp_path_factory.mktemp("mutants")
    O.load("f32")

    def build(item):
        name, (pat, repl) = item
        if isinstance(pat, str):
            assert src.count(pat) == 1, f"{name}: pattern occurs {src.count(pat)} times"
            text = src.replace(pat, repl)
        else:
            assert len(pat.findall(src)) == 1, f"{name}: pattern occurs {len(pat.findall(src))} times"
            text = pat.sub(repl, src)
        assert text != src
        c, so = tmp / f"{name}.c", tmp / f"lib{name}.so"
        c.write_text(text)
        cc = subprocess.run([os.environ.get("CC", "gcc"), *cflags, "-I", odir, "-shared", "-o", str(so), str(c), "-lm"], capture_output=True, text=True)
        assert cc.returncode == 0, cc.stderr  # (a mutant may leave a parameter unused: its warnings are not shown)
        lib = ctypes.CDLL(str(so))
        for fn, (restype, argtypes) in O._SIGNATURES.items():
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = restype, argtypes
        return name, lib

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(pool.map(build, MUTANTS.items()))


@pytest.mark.parametrize("name", list(MUTANTS))
def test_judge_rejects_mutant(mutant_libs, name):
    rejected = []
    for run in RUNS:
        cfg, planted, o32, o64, thr, groups = T.reference_run(*run)
        cand = T.run_lib(mutant_libs[name], cfg, planted)
        try:
            T.judge(cfg, cand, o32, o64, thr, groups, what=f"mutant {name} on {run_id(run)}")
        except AssertionError as err:
            first = str(err).splitlines()[1]
            m = re.match(r"group directed .*first env (\d+) ", first)
            rejected.append((run_id(run), (f"line '{T.DIRECTED_NAMES[int(m.group(1))]}': " if m else "") + first))
    print(f"mutant {name}: rejected by {len(rejected)}/{len(RUNS)} runs; first: {rejected[:1]}")
    assert rejected, f"no run of the table rejects the mutant {name}"
