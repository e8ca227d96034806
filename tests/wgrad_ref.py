"""A plain-torch restatement of `lt_wgrad` and `lt_split_rows` (csrc/lt_wgrad.hip), a seeded case generator and the PER-ELEMENT comparator
that tests/test_hip_wgrad_f64.py holds the kernel to.  Nothing here needs a GPU; tests/test_wgrad_ref.py pins it.

`reference` is one text for every role: float64 on the CPU is the oracle, float32 on the CPU and on the GPU are the baselines (library
GEMM), and the bias gradient gets the float32 sum in row order as a third.  `designed` is the value the kernel is BUILT to produce - the
three kept products of the (hi, lo) split, summed in float64 - so that the kernel differs from it by its float32 accumulation only.

The bound, per output element, with S = |dz|^T |x| in float64:

    B[n][k] = 3 * 2^-22 * S[n][k]  +  floor * sum_m |x[m][k]|  +  2^-31 * sum_m |dz[m][n]|

- 3 * 2^-22 S: the dropped lo lo product and the two lo roundings, 2^-22 |a| |b| each (hi = f16(c) leaves |c - hi| <= 2^-11 |c|, which
  times 64 is an exact f32; lo = f16 of it errs by 2^-11 of that, and |lo / 64| <= 2^-11 |c| on both operands).
- floor = 2^-37 max |dz|, the header's: the scaled dz has its maximum in [2^7, 2^8), the lo half of a scaled element whose 64 (c - hi) is
  below 2^-14 is an f16 subnormal (spacing 2^-24), so every dz element carries an ABSOLUTE 2^-24 / 64 = 2^-30 in scaled units, 2^-37
  of the maximum.  With `amax == NULL` the scale is 1 and the same spacing is 2^-30 whatever the maximum: floor = max(2^-37 max, 2^-30 / s).
- 2^-31 sum |dz|: the same on x, which is not scaled: the rounding to f16's subnormal spacing, 2^-25, on the lo half of an |x| below 2^-9,
  divided by 64.

Check (1), f32 equivalence:   e(X) = max |X - X64| / B,          e_hip <= 1 + FACTOR max(e_baselines)
Check (2), the designed value: d(X) = max |X - D64| / S,         d_hip <= FACTOR max_baselines(max |X32 - X64| / S) + FACTOR * 2^-24
  Where a half is an f16 SUBNORMAL, |X - D64| may exceed that by 2^-24 of the products' NOMINAL size (each subnormal counted as 2^-14),
  less their true size: `aligned_standin` is the CPU model this comes from, tests/test_wgrad_ref.py shows it on the `range` case.
db: scaled by the float64 sum of |dz| per column (tests/ppo_ref.py's rule for reduced outputs), FACTOR max(e_baselines) + FACTOR * 2^-24;
the split-dz form adds 2^-22 (its summands are hi + lo / 64) and M times the floor above (every summand's subnormal lo half).
B, S and the floors come from the inputs and the oracle, never from a kernel's output.  A NaN or an infinity gives inf."""
import functools

import numpy as np
import torch

from tests.seq_ref import EPS, FACTOR

CLAMP = 1000.0  # LT_MLP_INPUT_CLAMP: what lt_split_rows (and the training forward) saturates rows at
FORMS = {"f32/f32": (False, False), "f32/split": (False, True), "split/split": (True, True), "split/f32": (True, False)}  # (dz_split, x_split)
MUTATIONS = {  # name -> the case it is shown on (`named_case`) and what it stands for
    "drop_alo_bhi": "the correction term a_lo b_hi dropped",
    "drop_ahi_blo": "the correction term a_hi b_lo dropped",
    "mantissa10": "both operands rounded to a 10-bit mantissa (the hi halves alone)",
    "ragged_repeats_last_row": "rows beyond a ragged M repeat row M - 1 unmasked",
    "drop_last_partial_step": "the last, partial 32-row step left out",
    "drop_one_slab": "one slice's slab left out of the sum",
    "amax_first_64_blocks": "the amax reduction reads its first 64 blocks only",
    "overhang_from_clamped_lane": "the last four columns of an overhanging k tile stored from the neighbouring (clamped) lane's columns",
    "db_wave0_only": "db without the partial sums of waves 1..3",
    "split_rows_without_clamp": "lt_split_rows without its clamp (held by the exact dword compare)",
}
# (480 / 481: 15 and 16 steps of 32 rows, where one slice becomes two; 511 and 513 are 16 and 17 steps, two slices both)
SHAPES = [(1, 4, 4), (31, 68, 60), (32, 64, 64), (33, 64, 64), (255, 12, 132), (257, 132, 68), (480, 64, 64), (481, 64, 64), (511, 64, 64),
          (513, 64, 64), (4100, 64, 64), (2049, 132, 348)]
VARIANT_SHAPES = [(257, 132, 68), (2049, 132, 348)]
VARIANTS = [("amax", dict(nblk=1)), ("amax", dict(nblk=64)), ("amax", dict(nblk=65)), ("amax", dict(nblk=512)), ("no_amax", {}), ("pow2_max", {}),
            ("ones_max", {}), ("big_x", {}), ("range", {}), ("zeros", {})]
SPLIT_EDGES = [0.0, -0.0, 1000.0, -1000.0, 1000.0001, -1000.0001, 1e9, -1e9, float("inf"), float("-inf"),
               2.0 ** -14, float(np.nextafter(np.float32(2.0 ** -14), np.float32(0))), float(np.nextafter(np.float32(2.0 ** -14), np.float32(1))),
               2.0 ** -24, float(np.nextafter(np.float32(2.0 ** -24), np.float32(0))), float(np.nextafter(np.float32(2.0 ** -24), np.float32(1))),
               2.0 ** -25, float(np.nextafter(np.float32(2.0 ** -25), np.float32(0))), float(np.nextafter(np.float32(2.0 ** -25), np.float32(1))),
               1.0 + 2.0 ** -11, -(1.0 + 2.0 ** -11), 1.0 + 3 * 2.0 ** -11, 65504.0, -65504.0, 2.0 ** -149, -(2.0 ** -149), 999.9999, 0.1, -3.3]


# ---- the host side of lt_wgrad ----------------------------------------------------------------------------------------------------------
def splits_of(M, N, K):
    """lt_wgrad_splits: at most 512 workgroups of one 64 x 64 tile each, at least 8 steps of 32 rows per slice"""
    tiles = -(-N // 64) * -(-K // 64)
    return max(1, min(512 // tiles, -(-M // 32) // 8))


def slice_rows(M, splits, split, wave=None):
    """the rows [r0, r1) of slice `split` (the 32-row steps dealt as evenly as possible); `wave`: of that wave's quarter of the slice"""
    steps = -(-M // 32)
    b0, b1 = steps * split // splits, steps * (split + 1) // splits
    if wave is not None:
        b0, b1 = b0 + (b1 - b0) * wave // 4, b0 + (b1 - b0) * (wave + 1) // 4
    return min(32 * b0, M), min(32 * b1, M)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def make_case(M, N, K, seed, variant=None, nblk=1):
    """CPU float32 inputs of one call: dict(dz [M][N], x [M][K], amax [nblk] or None, M, N, K, variant).

    x ~ N(0, 1) times a column scale in [0.25, 3]; dz ~ N(0, 1) times a heavy-tailed row scale (rand^4: most of the mass in few rows, as the
    PPO loss leaves it), a column scale in [1/8, 1] and 3 / M.  Rows M - 1, M - 2 and the first row of the last 32-row step have row scale 1:
    a slip at the ragged end of M (a clamped load that is not masked, a last step dropped) must meet rows that carry mass.
    Variants: `amax` - the maxima in `nblk` blocks of consecutive rows, with ONE element of row M - 1 planted at 16 times the largest other
    and that row counted in the LAST block, so a reduction that misses the last block scales the gradient out of f16; `no_amax` - amax NULL,
    dz of order 1; `pow2_max` / `ones_max` - max |dz| exactly 2^-13 / nextafter(2^-12, 0) (the scaled maximum is 2^7 / rounds up to 2^8 in
    f16); `big_x` - a few x at +-65504 and +-60000; `range` - one dz column times 2^-24, one times 2^-30, one x column times 1e-5, one times
    1e-7; `zeros` - rows 0..31 of dz and one column of it all zero."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rand, randn = (lambda *s: torch.rand(*s, generator=gen)), (lambda *s: torch.randn(*s, generator=gen))
    x = randn(M, K) * (0.25 + 2.75 * rand(1, K))
    rows = rand(M, 1) ** 4
    for r in {M - 1, max(M - 2, 0), (M - 1) // 32 * 32}:
        rows[r] = 1.0
    dz = randn(M, N) * rows * (0.125 + 0.875 * rand(1, N)) * (3.0 / M)
    if variant == "no_amax":
        dz = dz * (M / 3.0)
    elif variant in ("pow2_max", "ones_max"):
        t = 2.0 ** -13 if variant == "pow2_max" else float(np.nextafter(np.float32(2.0 ** -12), np.float32(0)))
        at = int(dz.abs().argmax())
        dz = (dz * (t / float(dz.abs().max()))).clamp(-t, t)
        dz.view(-1)[at] = t
        assert float(dz.abs().max()) == t
    elif variant == "big_x":
        flat, spots = x.view(-1), torch.arange(3, M * K, max(1, M * K // 13))
        flat[spots] = torch.tensor([65504.0, -65504.0, 60000.0, -60000.0])[torch.arange(spots.numel()) % 4]
    elif variant == "range":
        dz[:, 1] *= 2.0 ** -24
        dz[:, N - 2] *= 2.0 ** -30
        x[:, 2] *= 1e-5
        x[:, K - 3] *= 1e-7
    elif variant == "zeros":
        dz[:32] = 0.0
        dz[:, N // 2] = 0.0
    amax = None
    if variant == "amax":
        dz[M - 1, N // 2] = 16.0 * float(dz.abs().max())
        block = (torch.arange(M) * nblk // M).clamp(max=nblk - 1)
        block[M - 1] = nblk - 1
        amax = torch.zeros(nblk).scatter_reduce_(0, block, dz.abs().amax(1), "amax", include_self=True)
        assert int(amax.argmax()) == nblk - 1 and (nblk == 1 or float(amax[:-1].max()) * 16.0 <= float(amax[-1]))
    elif variant != "no_amax":
        amax = dz.abs().max().reshape(1).clone()
    return dict(dz=dz.contiguous(), x=x.contiguous(), amax=amax, M=M, N=N, K=K, variant=variant)


@functools.lru_cache(maxsize=None)
def case_of(M, N, K, variant=None, nblk=1):
    """THE case of a shape and variant, built once and shared (nobody writes into it); the seed is a function of the shape (with these seeds
    `designed` uses at most 0.35 of check (1)'s allowance on every case: tests/test_wgrad_ref.py asserts 0.5)"""
    return make_case(M, N, K, 1000 * M + 10 * N + K, variant, nblk)


# ---- the kernels' arithmetic, bit for bit -----------------------------------------------------------------------------------------------
def split_ref(v, clamp=None):
    """lt_split_rows (clamp = CLAMP) / split8 (clamp None) on float32 values: hi = f16(c), lo = f16(64 (c - f32(hi))), round to nearest even
    -> (hi, lo, the packed int32 dwords hi | lo << 16)"""
    c = v.to(torch.float32)
    if clamp is not None:
        c = c.clamp(-clamp, clamp)
    hi = c.half()
    lo = ((c - hi.float()) * 64.0).half()
    return hi, lo, (hi.view(torch.int16).to(torch.int32) & 0xFFFF) | (lo.view(torch.int16).to(torch.int32) << 16)


def scale_ref(amax):
    """the power of two lt_wgrad multiplies dz by: 2^(7 - e), e the exponent FIELD of the float32 maximum of `amax` less 127 (zero and
    subnormals: -127), the exponent clamped to +-100.  amax None: 1."""
    if amax is None:
        return 1.0
    bits = int(amax.to(torch.float32).max().view(torch.int32))
    e = ((bits >> 23) & 0xFF) - 127
    return 2.0 ** max(-100, min(100, 7 - e))


def _round_mantissa10(x):
    return ((x.view(torch.int32) + 0x1000) & ~0x1FFF).view(torch.float32)


def operands(case, x_clamped=False):
    x = case["x"].clamp(-CLAMP, CLAMP) if x_clamped else case["x"]
    return case["dz"], x


def reference(case, dtype=torch.float64, device="cpu", x_clamped=False):
    """dW = dz^T x [N][K] and db = column sums of dz [N] in `dtype` on `device`; in float32 on the CPU also db_seq, the sum in row order
    (numpy's cumsum: torch's accumulates float32 in double on the CPU).  `x_clamped`: the rows as the split format holds them."""
    dz, x = (t.to(device=device, dtype=dtype) for t in operands(case, x_clamped))
    res = dict(dw=dz.t() @ x, db=dz.sum(0))
    if dtype == torch.float32 and device == "cpu":
        res["db_seq"] = torch.from_numpy(np.cumsum(case["dz"].numpy(), axis=0, dtype=np.float32)[-1].copy())
    return res


def designed(case, mutate=None, x_clamped=False, dz_split=False):
    """What the kernel is designed to produce, in float64: dW = (64 a_hi b_hi + a_hi b_lo + a_lo b_hi) / (64 s) with a = s dz, b = x split by
    `split_ref` and s = `scale_ref`, the sums in float64 (products of two f16 numbers have 22 bits: each is exact, and so is their sum to
    2^-53); db = the float64 column sums of dz, or of (a_hi + a_lo / 64) / s in the split-dz form.  `mutate`: one of MUTATIONS, a slip."""
    dz, x = operands(case, x_clamped)
    M, N, K = case["M"], case["N"], case["K"]
    amax = case["amax"]
    if mutate == "amax_first_64_blocks" and amax is not None:
        amax = amax[:64]
    s = scale_ref(amax)
    a = dz * s
    if mutate == "mantissa10":
        ah, bh = _round_mantissa10(a).double(), _round_mantissa10(x).double()
        al, bl = torch.zeros_like(ah), torch.zeros_like(bh)
        a64 = 64.0 * ah
    else:
        ah, al, _ = split_ref(a, CLAMP if dz_split else None)
        bh, bl, _ = split_ref(x, None)
        a64 = (ah * 64.0).double()  # formed in f16 by the kernel: exact while |s dz| < 2^10, inf beyond
        ah, al, bh, bl = ah.double(), al.double(), bh.double(), bl.double()
    keep = torch.ones(M, 1, dtype=torch.float64)
    sp = splits_of(M, N, K)
    if mutate == "drop_last_partial_step" and M % 32:
        keep[(M - 1) // 32 * 32:] = 0.0
    if mutate == "drop_one_slab" and sp > 1:
        r0, r1 = slice_rows(M, sp, sp // 2)
        keep[r0:r1] = 0.0
    main, c1, c2 = (a64 * keep).t() @ bh, (ah * keep).t() @ bl, (al * keep).t() @ bh
    if mutate == "drop_alo_bhi":
        c2 = torch.zeros_like(c2)
    if mutate == "drop_ahi_blo":
        c1 = torch.zeros_like(c1)
    dw = (main + c1 + c2) / (64.0 * s)
    if mutate == "ragged_repeats_last_row" and M % 32:
        pad = 32 - M % 32  # the clamped loads of BOTH operands land on row M - 1
        dw = dw + pad * (a64[M - 1:].t() @ bh[M - 1:] + ah[M - 1:].t() @ bl[M - 1:] + al[M - 1:].t() @ bh[M - 1:]) / (64.0 * s)
    if mutate == "overhang_from_clamped_lane" and K % 64 and K >= 8:
        dw[:, K - 4:] = dw[:, K - 8:K - 4]
    # what check (2) allows for SUBNORMAL halves (see `aligned_standin`): the sum of the three products at the operands' nominal magnitudes
    # less the same at their true ones - zero when no half is an f16 subnormal
    nom = lambda v: v.abs().clamp_min(2.0 ** -14)  # noqa: E731
    excess = (nom(a64).t() @ nom(bh) + nom(ah).t() @ nom(bl) + nom(al).t() @ nom(bh)
              - (a64.abs().t() @ bh.abs() + ah.abs().t() @ bl.abs() + al.abs().t() @ bh.abs())) / (64.0 * s)
    excess = torch.where(torch.isfinite(excess), excess, torch.zeros_like(excess))
    summand = (ah + al / 64.0) / s if dz_split else dz.double()
    if mutate == "db_wave0_only":
        keep = torch.zeros(M, 1, dtype=torch.float64)
        for split in range(sp):
            r0, r1 = slice_rows(M, sp, split, wave=0)
            keep[r0:r1] = 1.0
    db = (summand * keep).sum(0) if mutate in ("db_wave0_only", "drop_last_partial_step", "drop_one_slab") else summand.sum(0)
    return dict(dw=dw, db=db, excess=excess)


def aligned_standin(case, window=24):
    """A CPU stand-in for the one way the matrix core may differ from `designed` beyond the order of its float32 additions: an adder that
    ALIGNS the 32 products of one MFMA at the largest NOMINAL exponent among them and cuts each `window` bits below it.  A product of two
    normal f16 numbers has 22 bits below its nominal exponent, so among normal operands of similar size nothing is cut that a float32
    accumulator keeps; an f16 SUBNORMAL is held at exponent 2^-14 whatever its value, so its products are cut at 2^-24 of 2^-14 |other|,
    not of the product.  Everything else is float64.  window = 24: the narrowest an adder that feeds a float32 accumulator can be.
    -> dW [N][K] float64 (f32 / f32 form; small cases only: it forms every product)"""
    dz, x = operands(case)
    M, s = case["M"], scale_ref(case["amax"])
    ah, al, _ = split_ref(dz * s)
    bh, bl, _ = split_ref(x)
    pad = -M % 32
    total = 0.0
    for A, Bm in (((ah * 64.0).double(), bh.double()), (ah.double(), bl.double()), (al.double(), bh.double())):
        A, Bm = torch.nn.functional.pad(A, (0, 0, 0, pad)), torch.nn.functional.pad(Bm, (0, 0, 0, pad))
        ea = torch.frexp(A.abs().clamp_min(2.0 ** -14))[1] - 1
        eb = torch.frexp(Bm.abs().clamp_min(2.0 ** -14))[1] - 1
        P = (A[:, :, None] * Bm[:, None, :]).view(-1, 32, A.shape[1], Bm.shape[1])
        E = (ea[:, :, None] + eb[:, None, :]).view(-1, 32, A.shape[1], Bm.shape[1])
        unit = torch.exp2((E.amax(1, keepdim=True) - (window - 1)).double())
        total = total + (torch.trunc(P / unit) * unit).sum((0, 1))
    return total / (64.0 * s)


# ---- the comparator ---------------------------------------------------------------------------------------------------------------------
def oracle(case, x_clamped=False):
    """Everything the comparator needs that does not depend on a kernel: the float64 reference, S, B, the column sums of |dz|, the floor."""
    dz, x = (t.double() for t in operands(case, x_clamped))
    ref = reference(case, x_clamped=x_clamped)
    S = dz.abs().t() @ x.abs()
    amax_dz, s = float(dz.abs().max()), scale_ref(case["amax"])
    floor = max(2.0 ** -37 * amax_dz, 2.0 ** -30 / s) if case["amax"] is None else 2.0 ** -37 * amax_dz
    sum_dz, sum_x = dz.abs().sum(0), x.abs().sum(0)
    B = 3.0 * 2.0 ** -22 * S + floor * sum_x[None, :] + 2.0 ** -31 * sum_dz[:, None]
    return dict(dw=ref["dw"], db=ref["db"], S=S, B=B, sum_dz=sum_dz, floor=floor, M=case["M"])


def _ratio(got, want, scale):
    """max over elements of |got - want| / scale and where: 0 / 0 is 0, anything else over 0 and any NaN or infinity is inf"""
    g = got.detach().to(device="cpu", dtype=torch.float64)
    assert g.shape == want.shape == scale.shape, (g.shape, want.shape, scale.shape)
    diff = (g - want).abs()
    q = torch.where(scale > 0.0, diff / scale, torch.where(diff == 0.0, 0.0, float("inf")).to(diff.dtype))
    q = torch.where(torch.isfinite(g) & (q == q), q, torch.full_like(q, float("inf")))
    at = int(q.argmax())
    return float(q.view(-1)[at]), tuple(int(i) for i in np.unravel_index(at, tuple(q.shape)))


def judge(got, orc, des, baselines, dz_split=False):
    """`got`: dict(dw, db or None) of a kernel (or a stand-in); `orc` = oracle(case), `des` = designed(case), `baselines`: float32 results
    of `reference`.  -> name -> (value, allowance, where, value / allowance); a check passes when value <= allowance."""
    rep = {}
    e_b = max(_ratio(b["dw"], orc["dw"], orc["B"])[0] for b in baselines)
    e, at = _ratio(got["dw"], orc["dw"], orc["B"])
    rep["dw(1)"] = (e, 1.0 + FACTOR * e_b, at)
    d_b = max(_ratio(b["dw"], orc["dw"], orc["S"])[0] for b in baselines)
    d, at = _ratio(got["dw"], des["dw"], orc["S"])
    rep["dw(2)"] = (d, FACTOR * d_b + FACTOR * EPS, at)
    if "excess" in des and float(des["excess"].max()) > 0.0:  # subnormal halves: 2^-24 of the products' NOMINAL size on top (`aligned_standin`)
        allow = (FACTOR * d_b + FACTOR * EPS) * orc["S"] + EPS * des["excess"]
        d, at = _ratio(got["dw"], des["dw"], allow)
        rep["dw(2)"] = (d, 1.0, at)
    if got.get("db") is not None:
        sums = [b[n] for b in baselines for n in ("db", "db_seq") if n in b]
        e_b = max(_ratio(b, orc["db"], orc["sum_dz"])[0] for b in sums)
        extra = 2.0 ** -22 * orc["sum_dz"] + orc["M"] * orc["floor"] if dz_split else torch.zeros_like(orc["sum_dz"])
        allow = (FACTOR * e_b + FACTOR * EPS) * orc["sum_dz"] + extra
        e, at = _ratio(got["db"], orc["db"], allow)
        rep["db"] = (e, 1.0, at)
    return {n: (v, a, at, v / a if a > 0.0 and v == v else float("inf")) for n, (v, a, at) in rep.items()}


def failures(report):
    return {n: r for n, r in report.items() if not r[0] <= r[1]}


def worst(report):
    name = max(report, key=lambda n: report[n][3] if report[n][3] == report[n][3] else float("inf"))
    return name, report[name][3], report[name][2]


def format_report(report):
    return " ".join(f"{n}:{v:.2e}/{a:.2e}={r:.2f}@{at}" for n, (v, a, at, r) in report.items())


def named_case(mutation):
    """the case each slip is shown on"""
    if mutation == "amax_first_64_blocks":
        return case_of(257, 132, 68, "amax", 65)
    if mutation == "drop_one_slab":
        return case_of(2049, 132, 348)
    if mutation in ("ragged_repeats_last_row", "drop_last_partial_step"):
        return case_of(33, 64, 64)
    return case_of(257, 132, 68)
