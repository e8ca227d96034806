"""`lt_wgrad` and `lt_split_rows` (csrc/lt_wgrad.hip) straight through the C ABI, held to the float64 oracle of tests/wgrad_ref.py ELEMENT BY
ELEMENT, in all four operand forms (f32 / f32, f32 / split x, split dz / split x, split dz / f32 x).  Per output element, with
S = |dz|^T |x| and B = 3 * 2^-22 S + floor * sum |x| + 2^-31 sum |dz| (the module docstring of tests/wgrad_ref.py derives it):

    (1)  max |dW - dW64| / B   <=  1 + 4 max(the same of the float32 baselines, CPU and GPU)
    (2)  max |dW - D64| / S    <=  4 max(max |dW32 - dW64| / S of the baselines) + 4 * 2^-24     (D64: the designed value)
         (where a half is an f16 subnormal, 2^-24 of the products' nominal size on top: `wgrad_ref.aligned_standin`)
    db:  |db - db64| <= (4 max(e_baselines) + 4 * 2^-24) sum |dz|, the split-dz form 2^-22 sum |dz| + M floor more

The slabs are added in float64 (lt_partial_sums, which adds them in training, is held by tests/test_hip_ppo_f64.py).  Every input, output
and scale is a view into a larger allocation with 64 words of a NaN bit pattern on each side, outputs start as that NaN; afterwards every
guard and every input is bit-identical and slabs[:splits N K] / db_slabs[:splits N] hold no NaN.  A second run gives the same bits slab by
slab, and the four forms give the same dW slab bits ("same halves, same MFMAs").  `lt_split_rows` equals `split_ref` dword for dword.

One line per case is printed (`-s`): WGRADF64, the worst ratio to its allowance over the forms and where; DESIGN.md records them."""
import pytest
import torch

from tests import wgrad_ref as R
from tests.guarded import DEV, NAN_BITS, guard_problem, guarded

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32


def _call(name, *args):
    from locotouch_amd import _abi

    _abi.call(name, *args, _abi.stream(torch.device(DEV)))


class _Arrays:
    """the guarded device arrays of one case: inputs are compared bit for bit with what went in, outputs start as the NaN pattern"""

    def __init__(self):
        self.bufs, self.inputs = {}, {}

    def input(self, name, data):
        """`data`: a CPU float32 or int32 tensor (dwords of the split format travel as int32)"""
        bits = data.contiguous().view(I32)
        self.bufs[name] = guarded(tuple(bits.shape), bits.view(F32))
        self.inputs[name] = bits.clone()
        return self.bufs[name][1]

    def freeze(self, name):
        """an array a kernel of this test wrote (the split operands) and the next only reads"""
        torch.cuda.synchronize()
        self.inputs[name] = self.bufs[name][1].view(I32).cpu().clone()

    def output(self, name, shape):
        self.bufs[name] = guarded(shape)
        return self.bufs[name][1]

    def refill(self, name):
        self.bufs[name][1].view(I32).fill_(NAN_BITS)

    def problems(self):
        torch.cuda.synchronize()
        out = [p for p in (guard_problem(n, buf, view) for n, (buf, view) in self.bufs.items()) if p]
        out += [f"input {n} changed" for n, bits in self.inputs.items() if not torch.equal(self.bufs[n][1].view(I32).cpu(), bits)]
        return out


def _split_rows(G, name, data):
    """`data` (CPU float32) through lt_split_rows on guarded arrays -> the device dwords (a float32 view), checked against split_ref"""
    src = G.input(name + ".f32", data)
    out = G.output(name, tuple(data.shape))
    _call("lt_split_rows", src, out, data.numel())
    G.freeze(name)
    assert torch.equal(G.inputs[name], R.split_ref(data, R.CLAMP)[2]), f"lt_split_rows({name}) differs from split_ref"
    return out


def _run_forms(case, forms=tuple(R.FORMS), with_db=True):
    """-> {form: (slabs [splits][N][K] CPU float32, db slabs [splits][N] or None)}; asserts guards, inputs, NaN, run-to-run bits"""
    M, N, K = case["M"], case["N"], case["K"]
    sp, s = R.splits_of(M, N, K), R.scale_ref(case["amax"])
    G = _Arrays()
    dz, x = G.input("dz", case["dz"]), G.input("x", case["x"])
    amax = G.input("amax", case["amax"]) if case["amax"] is not None else None
    nblk = 0 if amax is None else amax.numel()
    scale = G.input("dz_scale", torch.tensor([s], dtype=F32))
    dzs = _split_rows(G, "dz.split", case["dz"] * s) if any(R.FORMS[f][0] for f in forms) else None
    xs = _split_rows(G, "x.split", case["x"]) if any(R.FORMS[f][1] for f in forms) else None
    slabs, dbs = G.output("slabs", (sp, N, K)), G.output("db_slabs", (sp, N))
    res = {}
    for form in forms:
        a_split, b_split = R.FORMS[form]
        runs = []
        for _ in range(2):
            G.refill("slabs"), G.refill("db_slabs")
            _call("lt_wgrad", dzs if a_split else dz, int(a_split), scale if a_split else None, xs if b_split else x, int(b_split), M, N, K, amax, nblk,
                  slabs, dbs if with_db else None)
            problems = G.problems()
            assert not problems, (form, problems)
            runs.append((slabs.cpu().clone(), dbs.cpu().clone()))
        assert torch.equal(runs[0][0].view(I32), runs[1][0].view(I32)), f"{form}: two runs differ in the slabs"
        assert torch.equal(runs[0][1].view(I32), runs[1][1].view(I32)), f"{form}: two runs differ in the db slabs"
        assert not bool(torch.isnan(runs[0][0]).any()), f"{form}: {int(torch.isnan(runs[0][0]).sum())} NaN left in the slabs"
        if with_db:
            assert not bool(torch.isnan(runs[0][1]).any()), f"{form}: NaN left in the db slabs"
        else:
            assert bool((runs[0][1].view(I32) == NAN_BITS).all()), f"{form}: db slabs written without being given"
        res[form] = (runs[0][0], runs[0][1] if with_db else None)
    return res


def _baselines(case, x_clamped):
    return [R.reference(case, F32, "cpu", x_clamped), R.reference(case, F32, DEV, x_clamped)]


def _judge(tag, case, res, clamped_forms=()):
    """print the case's line, then checks (1), (2) and db per form.  `clamped_forms`: the forms whose x the split format saturated."""
    reports, orc = {}, {}
    for form, (slabs, dbs) in res.items():
        xc = form in clamped_forms
        if xc not in orc:
            orc[xc] = (R.oracle(case, xc), _baselines(case, xc))
        got = dict(dw=slabs.double().sum(0), db=None if dbs is None else dbs.double().sum(0))
        des = R.designed(case, x_clamped=xc, dz_split=R.FORMS[form][0])
        reports[form] = R.judge(got, orc[xc][0], des, orc[xc][1], dz_split=R.FORMS[form][0])
    form = max(reports, key=lambda f: R.worst(reports[f])[1])
    name, ratio, at = R.worst(reports[form])
    print(f"\nWGRADF64 {tag}: worst {ratio:.2f} of its allowance at {form} {name}{list(at)} | "
          + " | ".join(f"{f} {R.format_report(r)}" for f, r in reports.items()))
    bad = {f: R.failures(r) for f, r in reports.items() if R.failures(r)}
    assert not bad, bad


def _same_slab_bits(res, groups):
    for group in groups:
        first = res[group[0]][0].view(I32)
        for form in group[1:]:
            assert torch.equal(first, res[form][0].view(I32)), f"dW slabs of {form} differ from {group[0]}'s in {int((first != res[form][0].view(I32)).sum())} words"


@pytest.mark.parametrize("m,n,k", R.SHAPES, ids=str)
def test_every_shape_in_all_four_forms(m, n, k):
    case = R.case_of(m, n, k)
    res = _run_forms(case)
    _same_slab_bits(res, [tuple(R.FORMS)])
    # db: the two f32-dz forms add the same floats in the same order, and so do the two split-dz forms
    for a, b in (("f32/f32", "f32/split"), ("split/split", "split/f32")):
        assert torch.equal(res[a][1].view(I32), res[b][1].view(I32)), (a, b)
    _judge(f"({m},{n},{k}) {R.splits_of(m, n, k)} slices", case, res)


@pytest.mark.parametrize("m,n,k", [(33, 64, 64), (2049, 132, 348)], ids=str)
def test_without_db_slabs_the_same_slabs_and_nothing_else_written(m, n, k):
    case = R.case_of(m, n, k)
    res, with_db = _run_forms(case, with_db=False), _run_forms(case, forms=("f32/f32",))
    _same_slab_bits({**res, "with db": with_db["f32/f32"]}, [tuple(R.FORMS) + ("with db",)])
    _judge(f"({m},{n},{k}) db_slabs NULL", case, res)


@pytest.mark.parametrize("variant,kw", R.VARIANTS, ids=str)
@pytest.mark.parametrize("m,n,k", R.VARIANT_SHAPES, ids=str)
def test_variants(m, n, k, variant, kw):
    case = R.case_of(m, n, k, variant, kw.get("nblk", 1))
    res = _run_forms(case)
    split_x = tuple(f for f in R.FORMS if R.FORMS[f][1])
    if variant == "big_x":  # the split format saturates x at 1000: two pairs of forms, two oracles
        assert float(case["x"].abs().max()) == 65504.0
        _same_slab_bits(res, [("f32/f32", "split/f32"), ("f32/split", "split/split")])
    else:
        _same_slab_bits(res, [tuple(R.FORMS)])
    if variant == "zeros":
        for form, (slabs, dbs) in res.items():
            assert float(slabs[:, n // 2].abs().max()) == 0.0 and float(dbs[:, n // 2].abs().max()) == 0.0, form  # dz's all-zero column, every slab
    _judge(f"({m},{n},{k}) {variant} {kw or ''}", case, res, clamped_forms=split_x if variant == "big_x" else ())


@pytest.mark.parametrize("count", [None, 4, 4 * 257 + 4])
def test_split_rows_is_split_ref_bit_for_bit(count):
    """the edge table padded to a multiple of 4; tiled to 4 values (one thread) and to 4 * 257 + 4 (a second block, partly filled)"""
    edges = torch.tensor(R.SPLIT_EDGES, dtype=F32)
    if count == 4:
        data = torch.tensor([1000.0001, -1e9, 2.0 ** -14, 1.0 + 2.0 ** -11], dtype=F32)
    else:
        count = count or -(-edges.numel() // 4) * 4
        data = edges.repeat(-(-count // edges.numel()))[:count].clone()
    G = _Arrays()
    _split_rows(G, "edges", data)  # (asserts the dwords)
    problems = G.problems()
    print(f"\nWGRADF64 lt_split_rows count {count}: equal to split_ref dword for dword")
    assert not problems, problems


def test_largest_accepted_operand_has_no_wrapped_offset():
    """M = 2^21 - 1, N = 4, K = 512: x is 4 GiB less 2 KiB, the largest lt_wgrad accepts; f32 / f32, checks (1) and (2) with the float64
    reference, S, B and the designed value formed on the device in row chunks (the float32 baseline is the GPU's GEMM in the same chunks,
    added in float32).  Rows M - 1, M - 2 and the first row of the last step carry row scale 1 as in every case."""
    M, N, K = (1 << 21) - 1, 4, 512
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 16 << 30:
        pytest.skip(f"needs 16 GiB of free device memory, {free >> 30} GiB are free")
    gen = torch.Generator(device=DEV).manual_seed(21)
    xbuf = torch.empty(M * K + 128, dtype=F32, device=DEV)
    xbuf.view(I32)[:64] = NAN_BITS
    xbuf.view(I32)[-64:] = NAN_BITS
    x = xbuf[64:64 + M * K].view(M, K)
    CH = 1 << 17
    for r in range(0, M, CH):
        x[r:r + CH] = torch.randn(min(CH, M - r), K, device=DEV, generator=gen) * (0.25 + 2.75 * torch.rand(1, K, device=DEV, generator=gen))
    rows = torch.rand(M, 1, device=DEV, generator=gen) ** 4
    rows[[M - 1, M - 2, (M - 1) // 32 * 32]] = 1.0
    dz_cpu = (torch.randn(M, N, device=DEV, generator=gen) * rows * (0.125 + 0.875 * torch.rand(1, N, device=DEV, generator=gen)) * (3.0 / M)).cpu()
    G = _Arrays()
    dz, amax = G.input("dz", dz_cpu), G.input("amax", dz_cpu.abs().max().reshape(1))
    sp, s = R.splits_of(M, N, K), R.scale_ref(dz_cpu.abs().max().reshape(1))
    slabs = G.output("slabs", (sp, N, K))
    x_sum_before = x.view(I32).sum(dtype=torch.int64)
    _call("lt_wgrad", dz, 0, None, x, 0, M, N, K, amax, 1, slabs, None)
    problems = G.problems()
    assert not problems, problems
    assert bool((xbuf.view(I32)[:64] == NAN_BITS).all()) and bool((xbuf.view(I32)[-64:] == NAN_BITS).all()) and int(x.view(I32).sum(dtype=torch.int64)) == int(x_sum_before)
    got = slabs.cpu()
    assert not bool(torch.isnan(got).any())
    F64 = torch.float64
    z = lambda dt: torch.zeros(N, K, dtype=dt, device=DEV)  # noqa: E731
    dw64, S, D, dw32, sum_x = z(F64), z(F64), z(F64), z(F32), torch.zeros(K, dtype=F64, device=DEV)
    for r in range(0, M, CH):
        a32, b32 = dz[r:r + CH], x[r:r + CH]
        a, b = a32.double(), b32.double()
        dw64 += a.t() @ b
        S += a.abs().t() @ b.abs()
        sum_x += b.abs().sum(0)
        dw32 += a32.t() @ b32
        (ah, al, _), (bh, bl, _) = R.split_ref(a32 * s), R.split_ref(b32)
        D += ((ah * 64.0).double().t() @ bh.double() + ah.double().t() @ bl.double() + al.double().t() @ bh.double()) / (64.0 * s)
    sum_dz = dz_cpu.double().abs().sum(0)
    B = 3.0 * 2.0 ** -22 * S.cpu() + 2.0 ** -37 * float(dz_cpu.abs().max()) * sum_x.cpu()[None, :] + 2.0 ** -31 * sum_dz[:, None]
    orc = dict(dw=dw64.cpu(), S=S.cpu(), B=B)
    rep = R.judge(dict(dw=got.double().sum(0), db=None), orc, dict(dw=D.cpu()), [dict(dw=dw32.cpu())])
    name, ratio, at = R.worst(rep)
    print(f"\nWGRADF64 ({M},{N},{K}) {sp} slices, x of 4 GiB - 2 KiB: worst {ratio:.2f} of its allowance at {name}{list(at)} | {R.format_report(rep)}")
    assert not R.failures(rep), R.failures(rep)
