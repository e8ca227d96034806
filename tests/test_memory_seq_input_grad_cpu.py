"""`memory_rollout_sequence` on rows that require a gradient, PyTorch-op form (the CPU, float64): the rows get dX = d_ih W_ih - before
this they got nothing, so a layer in front of a memory trained as if frozen - and the eight parameter gradients are what a call on rows
without a gradient gives, bit for bit.  The reference is an `nn.LSTMCell` / `nn.GRUCell` loop over the same parameters that zeroes the
state behind a done (tests/memory_dx_ref.py).  The HIP form's counterpart is tests/test_hip_memory_dx.py."""
import pytest
import torch

from tests.memory_dx_ref import Case

T, E, I_A, I_C, H = 5, 7, 5, 9, 64


@pytest.fixture(scope="module", params=["lstm", "gru"])
def case(request):
    c = Case(request.param, T, E, I_A, I_C, H, seed=3)
    assert bool(c.dones[0].any()) and bool(c.dones[T - 1].any()) and bool(c.dones[1:T - 1].any()) and not bool(c.dones.all(0).any())
    return c, c.loop(torch.float64)


def test_row_gradients_equal_the_cell_loop(case):
    c, (ref_dx, ref_params) = case
    dx, params, rows, _ = c.run(torch.float64, "cpu", requires_grad=True)
    for name, got, ref, x in zip(("obs.grad", "critic_obs.grad"), dx, ref_dx, rows):
        assert got is not None, f"{name} is None: the memory hands its input rows no gradient"
        assert got.shape == x.shape and got.dtype == torch.float64
        top = float(ref.abs().max())
        err = float((got - ref).abs().max())
        print(f"\n[{c.kind}] {name}: max |err| {err:.3e}  max |ref| {top:.3e}")
        assert top > 0 and err <= 1e-12 * top, (name, err, top)
    for k, (got, ref) in enumerate(zip(params, ref_params)):  # (the parameters' own, for the record: the loop is a fair reference)
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), k


def test_parameter_gradients_do_not_depend_on_whether_the_rows_ask(case):
    c, _ = case
    _, with_dx, _, _ = c.run(torch.float64, "cpu", requires_grad=True)
    dx, without, _, _ = c.run(torch.float64, "cpu", requires_grad=False)
    assert dx == [None, None]
    assert len(with_dx) == len(without) == 8
    for k, (a, b) in enumerate(zip(with_dx, without)):
        assert a is not None and torch.equal(a, b), k


def test_one_network_asking_alone_gets_the_same_gradient(case):
    c, _ = case
    both, _, _, _ = c.run(torch.float64, "cpu", requires_grad=True)
    for k in (0, 1):
        rows = c.rows(torch.float64, "cpu", False)
        rows[k].requires_grad_(True)
        dx, _, _, _ = c.run(torch.float64, "cpu", rows=rows)
        assert dx[1 - k] is None and torch.equal(dx[k], both[k]), k


def test_float32_rows_get_float32_gradients(case):
    c, (ref_dx, _) = case
    dx, _, _, _ = c.run(torch.float32, "cpu", requires_grad=True)
    for got, ref in zip(dx, ref_dx):
        assert got.dtype == torch.float32
        assert float((got.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
