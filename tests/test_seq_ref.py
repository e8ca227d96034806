"""tests/seq_ref.py itself, on the CPU: the oracle is pinned to a float64 `nn.LSTM` / `nn.GRU`, and the comparator with the generated
inputs is shown to tell a subtly wrong kernel from a right one (a float32 CPU form stands in for the kernel)."""
import functools

import pytest
import torch
import torch.nn as nn

from tests import seq_ref as R

MUT_SHAPE = (2, 17, 128)  # (L, B, H): a second row tile of one row, two k-blocks per wave, two steps


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("L,B,I,H", [(3, 5, 7, 64), (2, 17, 8, 128)])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_oracle_equals_float64_nn_module(cell, L, B, I, H):
    """With ig = x W_ih^T and dX, dW_*, db_* formed from the oracle's dig / dhg the way the contract tells the caller to, the oracle is
    nn.LSTM / nn.GRU in float64: outputs, final states and every gradient to 1e-12 relative."""
    torch.manual_seed(11)
    rnn = (nn.LSTM if cell == "lstm" else nn.GRU)(I, H).double()
    for p in rnn.parameters():  # PyTorch's init is U(-1/sqrt(H), 1/sqrt(H)) for everything; make the two biases visibly different
        p.data.mul_(3.0)
    x = torch.randn(L, B, I, dtype=torch.float64, requires_grad=True)
    h0 = torch.tanh(torch.randn(B, H, dtype=torch.float64)).requires_grad_(True)
    c0 = torch.randn(B, H, dtype=torch.float64, requires_grad=True)
    dout, dhn, dcn = torch.randn(L, B, H).double(), torch.randn(B, H).double(), torch.randn(B, H).double()
    if cell == "lstm":
        out, (hn, cn) = rnn(x, (h0[None], c0[None]))
        loss = (out * dout).sum() + (hn[0] * dhn).sum() + (cn[0] * dcn).sum()
    else:
        out, hn = rnn(x, h0[None])
        loss = (out * dout).sum() + (hn[0] * dhn).sum()
    loss.backward()

    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in rnn.parameters())
    case = dict(ig=x.detach() @ w_ih.t(), h0=h0.detach(), c0=c0.detach(), w_hh=w_hh, b_ih=b_ih, b_hh=b_hh, dout=dout, dhn=dhn, dcn=dcn)
    res = R.reference(cell, case)
    dig, dhg = (res["dgates"], res["dgates"]) if cell == "lstm" else (res["dig"], res["dhg"])
    h_prev = torch.cat([h0.detach()[None], res["out"][:-1]])
    flat = lambda t: t.reshape(L * B, -1)  # noqa: E731
    pairs = {"out": (res["out"], out.detach()), "h_n": (res["out"][-1], hn.detach()[0]), "dh0": (res["dh0"], h0.grad),
             "dx": (dig @ w_ih, x.grad), "dW_ih": (flat(dig).t() @ flat(x.detach()), rnn.weight_ih_l0.grad),
             "dW_hh": (flat(dhg).t() @ flat(h_prev), rnn.weight_hh_l0.grad), "db_ih": (flat(dig).sum(0), rnn.bias_ih_l0.grad),
             "db_hh": (flat(dhg).sum(0), rnn.bias_hh_l0.grad)}
    if cell == "lstm":
        pairs.update({"c_n": (res["cell"][-1], cn.detach()[0]), "dc0": (res["dc0"], c0.grad)})
    for name, (got, want) in pairs.items():
        assert _rel(got, want) <= 1e-12, (name, _rel(got, want))


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_oracle_with_null_carries_is_the_oracle_with_zero_carries(cell):
    case = R.make_case(cell, 2, 3, 64, seed=5)
    zero = dict(case, dhn=torch.zeros_like(case["dhn"]), dcn=torch.zeros_like(case["dcn"]))
    a, b = R.reference(cell, case, carries=False), R.reference(cell, zero)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["dh0"], R.reference(cell, case)["dh0"])


def test_case_generator_is_seeded_and_the_saturated_variant_saturates():
    a, b = R.make_case("gru", 2, 17, 128, seed=3), R.make_case("gru", 2, 17, 128, seed=3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["ig"], R.make_case("gru", 2, 17, 128, seed=4)["ig"])
    assert not torch.equal(a["b_ih"], a["b_hh"])
    s = R.make_case("gru", 2, 17, 128, seed=3, saturated=True)
    assert torch.equal(s["ig"][:, 1], a["ig"][:, 1]) and torch.equal(s["ig"][:, ::3, ::5], a["ig"][:, ::3, ::5] * 60.0)
    assert int((s["ig"].abs() > 88.0).sum()) >= 10 and int((s["ig"].abs() > 17.0).sum()) >= 100


@functools.lru_cache(maxsize=None)
def _mutation_setup(cell):
    case = R.make_case(cell, *MUT_SHAPE, seed=2017)
    return case, R.reference(cell, case), R.reference(cell, case, dtype=torch.float32)


@pytest.mark.parametrize("kernel_math", [False, True], ids=["library_order", "kernel_order"])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_unmutated_float32_form_passes(cell, kernel_math):
    """`kernel_order`: the float32 form arranged as the kernel is - the recurrent sum in four quarters of k added in wave order, sigmoid as
    1 / (1 + exp(-x)), tanh from exp(-2 |x|) - held against the library-order baseline: the bound has room for a correct kernel."""
    case, ref64, base = _mutation_setup(cell)
    report = R.compare(cell, R.reference(cell, case, dtype=torch.float32, kernel_math=kernel_math), ref64, [base])
    print(f"\nSEQREF {cell} {MUT_SHAPE} unmutated kernel_math={kernel_math}: worst {R.worst(report)} | {R.format_report(report)}")
    assert not R.failures(report), R.failures(report)
    if not kernel_math:  # the baseline against itself: e / (e + 2^-24)
        assert R.worst(report)[1] <= 1.0


MUTANTS = [(cell, m) for m, cells in R.MUTATIONS.items() for cell in cells]


@pytest.mark.parametrize("cell,mutation", MUTANTS, ids=[f"{c}-{m}" for c, m in MUTANTS])
def test_mutated_float32_form_is_rejected(cell, mutation):
    case, ref64, base = _mutation_setup(cell)
    report = R.compare(cell, R.reference(cell, case, dtype=torch.float32, kernel_math=True, mutate=mutation), ref64, [base])
    bad = R.failures(report)
    print(f"\nSEQREF {cell} {MUT_SHAPE} {mutation}: rejected on {len(bad)}/{len(report)} arrays, worst {R.worst(report)}")
    assert bad, R.format_report(report)
    # far outside, not marginally: the weakest of these (the mantissa rounding) lands about a thousand times outside the baseline's error
    assert R.worst(report)[1] >= 100.0, R.worst(report)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_mantissa_rounding_is_rejected_on_every_array(cell):
    """The reduced-precision MFMA that the 2e-4 bound of the older tests lets through: every array sees it, each on its own."""
    case, ref64, base = _mutation_setup(cell)
    report = R.compare(cell, R.reference(cell, case, dtype=torch.float32, kernel_math=True, mutate="mantissa10"), ref64, [base])
    assert R.failures(report).keys() == report.keys(), sorted(report.keys() - R.failures(report).keys())


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_saturated_case_is_finite_and_the_baseline_passes_itself(cell):
    case = R.make_case(cell, *MUT_SHAPE, seed=2018, saturated=True)
    ref64, base = R.reference(cell, case), R.reference(cell, case, dtype=torch.float32)
    for res in (ref64, base):
        for name, v in res.items():
            assert torch.isfinite(v).all(), name
    first = base["ws"][..., :MUT_SHAPE[2]]  # the first plane is a sigmoid in both cells: in f32 some of it has rounded to 1, some is tiny
    assert bool((first == 1.0).any()) and float(first.min()) < 1e-30
    report = R.compare(cell, base, ref64, [base])
    assert not R.failures(report) and R.worst(report)[1] <= 1.0
    kern = R.compare(cell, R.reference(cell, case, dtype=torch.float32, kernel_math=True), ref64, [base])
    print(f"\nSEQREF {cell} {MUT_SHAPE} saturated kernel_order: worst {R.worst(kern)} | {R.format_report(kern)}")
    assert not R.failures(kern), R.failures(kern)
