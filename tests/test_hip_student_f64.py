"""`lt_student_pack` and `lt_student_step` (csrc/lt_student.hip, the conv stack of csrc/lt_cnn_device.h) straight through the C ABI,
over the descriptor family include/lt_student.h advertises (tests/student_ref.py: CASES - the clamped k groups of the GRU launch, one
and two of its workgroups per row tile, one and seventeen unit tiles of an MLP layer, padded tails, the concatenation at P = 0, odd P
and cat_pad 528, encoder LDS above 64 KB, one to six layers), against the float64 restatement `student_ref.stages`.

Accuracy, per output array (the rule of tests/test_hip_encoder.py): the kernels sum the same exact f32 products as a plain f32
composition of torch ops on the same inputs (`student_ref.compose`: unfold + matmul, F.linear, the gate arithmetic) in another order,
so their largest error against float64 may be at most the larger of TWICE the composition's and one f32 ulp of the array's magnitude.
Both figures are printed (`STUDENTF64` lines).  tests/test_student_ref.py shows on the CPU that every fault of `student_ref.faults()`
moves an output by 500 times that allowance at these seeds.

Every array a launch sees lies between guard words (tests/guarded.py); outputs and scratch start as NaN patterns; both input matrices
are column slices of wider allocations whose other columns are NaN patterns.  Row independence, the done mask, a second run and the
row strides are held to equal bits.  Nothing here builds a `Student`, an env or a runner."""
import ctypes
import functools

import numpy as np
import pytest

from tests import student_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = R.NS[-1]
NAMES = list(R.CASES)


class Rig:
    """One case: its parameters on the device (the tensors the pack reads are the f32 composition's), the packed buffer between
    guards, and the inputs of N rows."""

    def __init__(self, name):
        import torch

        from locotouch_amd import _abi
        from tests import guarded as G

        self.name, self.case, self.seed = name, R.CASES[name], R.SEEDS[name]
        self.desc = R.desc_of(self.case)
        assert _abi.load().lt_student_validate(ctypes.byref(self.desc)) == 0
        self.P = R.random_params(self.case, self.seed)
        self.T = R.to_torch(self.P, DEV, torch.float32)
        self.img, self.Pd, self.H, self.A = int(np.prod(self.case["img"])), self.case["P"], self.case["H"], self.case["bb"][-1]
        size = ctypes.c_size_t()
        _abi.call("lt_student_packed_floats", self.desc, ctypes.byref(size))
        self.packed_buf, self.packed = G.guarded((size.value,))
        self.pack()
        self.in64 = R.random_inputs(self.case, N, self.seed)  # float64 arrays of f32 values: proprio, tactile, h
        self.prop, self.tac, self.h0 = (torch.as_tensor(a, dtype=torch.float32, device=DEV) for a in self.in64)

    def pack(self):
        import torch

        from locotouch_amd import _abi

        p, T = _abi.LtStudentParams(), self.T
        for i, (w, b, _) in enumerate(T["convs"]):
            p.conv_w[i], p.conv_b[i] = w.data_ptr(), b.data_ptr()
        p.head_w, p.head_b = (t.data_ptr() for t in T["head"][0])
        p.gru_w_ih, p.gru_w_hh, p.gru_b_ih, p.gru_b_hh = (t.data_ptr() for t in T["gru"])
        for tag in ("enc", "bb"):
            for i, (w, b) in enumerate(T[tag]):
                getattr(p, tag + "_w")[i], getattr(p, tag + "_b")[i] = w.data_ptr(), b.data_ptr()
        _abi.call("lt_student_pack", self.desc, p, self.packed, _abi.stream(torch.device(DEV)))
        torch.cuda.synchronize()

    def step(self, prop, tac, h, done=None, strided=True):
        """One lt_student_step on the rows given ([n][P], [n][img] plain tensors; `h`: a tensor [n][H], copied between guards, or the
        (allocation, view) pair of an earlier call, advanced IN PLACE; `done`: uint8 tensor or None).  Checks every guard, that inputs,
        mask and packed buffer keep their bits and that no output element stays NaN.  -> (actions, h view, (h allocation, h view))"""
        import torch

        from locotouch_amd import _abi
        from tests import guarded as G

        n, tag = tac.shape[0], f"{self.name} n={tac.shape[0]}"
        arrays = {"packed": (self.packed_buf, self.packed)}
        ps, ts = (self.Pd + (78 if self.Pd else 5), self.img + 3) if strided else (self.Pd, self.img)
        assert ts % 4 != 0 or not strided
        if self.Pd:
            arrays["proprio"] = G.guarded((n, ps))
            arrays["proprio"][1][:, :self.Pd].copy_(prop)
        arrays["tactile"] = G.guarded((n, ts))
        arrays["tactile"][1][:, :self.img].copy_(tac)
        if done is not None:
            arrays["done"] = G.guarded_like(done)
        arrays["h"] = h if isinstance(h, tuple) else G.guarded((n, self.H), data=h)
        arrays["actions"] = G.guarded((n, self.A))
        size = ctypes.c_size_t()
        _abi.call("lt_student_ws_floats", self.desc, n, ctypes.byref(size))
        assert size.value == n * (self.case["D"] + self.H)
        arrays["ws"] = G.guarded((size.value,))
        const = ("packed", "proprio", "tactile", "done")
        before = {k: arrays[k][0].clone() for k in const if k in arrays}
        _abi.call("lt_student_step", self.desc, self.packed, arrays["proprio"][1] if self.Pd else None, ps, arrays["tactile"][1], ts,
                  arrays["done"][1] if done is not None else None, arrays["h"][1], n, arrays["actions"][1], arrays["ws"][1],
                  _abi.stream(torch.device(DEV)))
        torch.cuda.synchronize()
        for k, (buf, view) in arrays.items():
            assert G.guard_problem(k, buf, view) is None, (tag, G.guard_problem(k, buf, view))
        for k, was in before.items():
            assert torch.equal(arrays[k][0], was), (tag, f"the step changed {k}")
        if strided:  # the columns between the rows were neither written (above) nor are anything but the NaN pattern they started as
            for k, width in (("proprio", self.Pd), ("tactile", self.img)):
                if k in arrays:
                    assert bool((arrays[k][1][:, width:].view(torch.int32) == G.NAN_BITS).all()), (tag, k)
        a, hv = arrays["actions"][1], arrays["h"][1]
        assert not torch.isnan(a).any() and not torch.isnan(hv).any(), (tag, "an output element was not written, or a NaN was read")
        return a, hv, arrays["h"]


@functools.lru_cache(maxsize=None)
def rig(name):
    return Rig(name)


@functools.lru_cache(maxsize=None)
def base(name):
    """(actions, h) clones of the single step of the case at N rows from its h0, no mask, strided inputs: shared, never changed."""
    g = rig(name)
    a, h, _ = g.step(g.prop, g.tac, g.h0)
    return a.clone(), h.clone()


@functools.lru_cache(maxsize=None)
def zero_state(name):
    """The same rows from an all-zero state, no mask."""
    import torch

    g = rig(name)
    a, h, _ = g.step(g.prop, g.tac, torch.zeros_like(g.h0))
    return a.clone(), h.clone()


def judge(tag, got, comp, want):
    """The house rule for one array: `got` (kernel) and `comp` (f32 composition) tensors against the float64 array `want`."""
    got, comp = got.double().cpu().numpy(), comp.double().cpu().numpy()
    err = np.abs(got - want)
    e_k, e_c = float(err.max()), float(np.abs(comp - want).max())
    bound = max(R.FACTOR * e_c, R.ulp32(float(np.abs(want).max())))
    print(f"\nSTUDENTF64 {tag}: max |err| vs f64  kernel {e_k:.3e}  f32 composition {e_c:.3e}  ratio {e_k / max(e_c, 1e-300):.2f}  bound {bound:.3e}")
    r, u = np.unravel_index(int(np.nanargmax(np.where(np.isnan(err), np.inf, err))), err.shape)
    assert e_k <= bound, f"{tag}: kernel {e_k:.3e} > bound {bound:.3e}; worst element row {r} unit {u} (row % 16 = {r % 16}, unit % 16 = {u % 16})"


def judge_step(g, tag, a, h, h_in, done):
    """Both output arrays of a step that started from the raw f32 state `h_in` (done rows may hold NaN) under `done`."""
    import torch

    d = None if done is None else done.cpu().numpy()
    want = R.stages(g.P, g.in64[0], g.in64[1], h_in.double().cpu().numpy(), d)
    with torch.no_grad():
        ca, ch = R.compose(g.T, g.prop, g.tac, h_in, done)
    judge(f"case={g.name} n={N} {tag} h", h, ch, want["h_new"])
    judge(f"case={g.name} n={N} {tag} actions", a, ca, want["actions"])


@pytest.mark.parametrize("name", NAMES)
def test_single_step_is_as_close_to_float64_as_the_f32_composition(name):
    g = rig(name)
    a, h = base(name)
    judge_step(g, "step", a, h, g.h0, None)


@pytest.mark.parametrize("name", NAMES)
def test_four_chained_steps_in_place_under_every_kind_of_mask(name):
    """Masks NULL, all zero, mixed, all one in front of the steps; the state advances in place.  Step t is judged alone: its
    references start from the raw f32 state the kernel left after step t - 1.  Before the mixed step the done rows' state is
    overwritten with NaN: the kernel must not read it."""
    import torch

    g = rig(name)
    mixed = torch.as_tensor(R.mixed_mask(N, g.seed), device=DEV)
    assert mixed[0] == 1 and mixed[-1] == 0 and 0 < int(mixed.sum()) < N
    masks = [None, torch.zeros(N, dtype=torch.uint8, device=DEV), mixed, torch.ones(N, dtype=torch.uint8, device=DEV)]
    a0, h0 = zero_state(name)
    state = g.h0
    for t, (kind, done) in enumerate(zip(("NULL", "zeros", "mixed", "ones"), masks)):
        if kind == "mixed":
            state[1][mixed != 0] = float("nan")
        h_in = (state[1] if isinstance(state, tuple) else state).clone()
        a, h, state = g.step(g.prop, g.tac, state, done)
        judge_step(g, f"chain step {t} mask={kind}", a, h, h_in, done)
        if kind == "zeros":  # a mask of zeros is no mask
            a2, h2, _ = g.step(g.prop, g.tac, h_in, None)
            assert torch.equal(a, a2) and torch.equal(h, h2), (name, kind)
        if kind == "mixed":  # a done row = the row from a zero state, bit for bit, whatever its state held
            rows = mixed != 0
            assert torch.equal(a[rows], a0[rows]) and torch.equal(h[rows], h0[rows]), (name, kind)
        if kind == "ones":
            assert torch.equal(a, a0) and torch.equal(h, h0), (name, kind)


@pytest.mark.parametrize("name", NAMES)
def test_a_rows_bits_depend_on_nothing_but_the_row(name):
    import torch

    g = rig(name)
    a, h = base(name)
    for n in R.NS[:-1]:  # the first rows alone
        an, hn, _ = g.step(g.prop[:n], g.tac[:n], g.h0[:n])
        assert torch.equal(an, a[:n]) and torch.equal(hn, h[:n]), (name, n)
    a2, h2, _ = g.step(g.prop, g.tac, g.h0)  # a second run
    assert torch.equal(a2, a) and torch.equal(h2, h), name
    idx = torch.roll(torch.arange(N, device=DEV), 37)  # every row in another place: another lane, another row tile, another conv tile
    am, hm, _ = g.step(g.prop[idx], g.tac[idx], g.h0[idx])
    assert torch.equal(am, a[idx]) and torch.equal(hm, h[idx]), name
    ac, hc, _ = g.step(g.prop, g.tac, g.h0, strided=False)  # contiguous rows: tactile_row_stride == img, proprio_row_stride == P
    assert torch.equal(ac, a) and torch.equal(hc, h), name


@pytest.mark.parametrize("name", NAMES)
def test_pack_writes_the_documented_layout_float_for_float_and_a_second_pack_refreshes(name):
    import torch

    from tests import guarded as G

    g = Rig(name)  # its own: the parameters are changed below
    a, h, _ = g.step(g.prop, g.tac, g.h0)
    a, h = a.clone(), h.clone()
    assert torch.equal(a, base(name)[0]) and torch.equal(h, base(name)[1])

    def check(P):
        want, known = R.pack(g.case, P)
        got = g.packed.cpu().numpy()
        assert got.shape == want.shape and G.guard_problem("packed", g.packed_buf, g.packed) is None
        bad = np.flatnonzero((got.view(np.int32) != want.view(np.int32)) & known)
        where = [(nm, int(bad[0]) - off) for nm, off, r, c in R.packed_blocks(g.case)[0] if bad.size and off <= bad[0] < off + r * c]
        assert bad.size == 0, (name, f"{bad.size} packed floats differ, the first in block {where}")
        zeros = known & (want == 0)  # every padding float of the layout, exact +0
        assert zeros.sum() >= sum(R.pad16(o) - o for o in g.case["enc"][1:] + g.case["bb"][1:]) and not got.view(np.int32)[zeros].any()

    check(g.P)
    with torch.no_grad():  # what an optimizer step does: the tensors change in place
        for group in (g.T["convs"], g.T["head"], g.T["enc"], g.T["bb"]):
            for w, b, *_ in group:
                w.mul_(0.75), b.add_(0.0625)
        for t in g.T["gru"]:
            t.mul_(1.25)
    a_old, h_old, _ = g.step(g.prop, g.tac, g.h0)  # not packed again: still the old parameters
    assert torch.equal(a_old, a) and torch.equal(h_old, h)
    g.pack()
    f = lambda t: t.double().cpu().numpy()  # noqa: E731
    P2 = dict(g.P, convs=[(f(w), f(b), s) for w, b, s in g.T["convs"]], gru=tuple(f(t) for t in g.T["gru"]),
              **{k: [(f(w), f(b)) for w, b in g.T[k]] for k in ("head", "enc", "bb")})
    check(P2)
    a_new, h_new, _ = g.step(g.prop, g.tac, g.h0)
    assert not torch.equal(a_new, a) and not torch.equal(h_new, h)
    want = R.stages(P2, g.in64[0], g.in64[1], g.in64[2])
    with torch.no_grad():
        ca, ch = R.compose(g.T, g.prop, g.tac, g.h0)
    judge(f"case={name} n={N} after the second pack h", h_new, ch, want["h_new"])
    judge(f"case={name} n={N} after the second pack actions", a_new, ca, want["actions"])
