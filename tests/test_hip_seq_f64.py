"""csrc/lt_seq_tile.h with the two cells of csrc/lt_lstm.hip and csrc/lt_gru.hip, straight through the C ABI (`lt_lstm_forward/backward`,
`lt_gru_forward/backward`), held to the float64 oracle of tests/seq_ref.py ARRAY BY ARRAY: `out`, `cell`, each of the four saved planes
of `ws`, each gate plane of `dgates` (LSTM) or `dig` / `dhg` (GRU), `dh0`, `dc0`.  Per array X, e(X) = max |X - X64| / max |X64| (no
clamp, no element left out) and the kernel passes when

    e_hip(X) <= 4 max(e_cpu32(X), e_gpu32(X)) + 4 * 2^-24

where the two baselines are the same plain-torch form in float32 on the CPU and on the GPU (`seq_ref.compare` has the reasons for the
factor and the floor).  The backward entry point is called with the kernel's OWN out / cell / ws, as its contract says.

Every input, output and the scratch array is a view into a larger allocation with 64 floats of a NaN bit pattern on each side (16-byte
alignment is kept); outputs and scratch start as that NaN.  After the calls every guard and every input is bit-identical (compared as
int32) and no output holds a NaN: a store outside [B] rows of a partial 16-row tile, or an element a kernel form leaves unwritten, shows.

One line per case is printed (`-s`): SEQF64, the worst ratio and its array, then e_hip/e_cpu32/e_gpu32=ratio per array; DESIGN.md
records them."""
import pytest
import torch

from tests import seq_ref as R
from tests.guarded import DEV, GUARD, NAN_BITS
from tests.guarded import guarded as _guarded

pytestmark = pytest.mark.gpu

# (L, B, H) -> what it reaches in lt_seq_tile.h
SHAPES = [(1, 1, 64),      # generic form, one k-block per wave, one row; the opening and the closing backward launch meet
          (2, 17, 128),    # KB = 2; a second row tile of one row; the GRU backward's single partial group (6 j-blocks)
          (3, 15, 192),    # generic form, 3 k-blocks per wave; a tile one row short
          (3, 16, 256),    # KB = 4; an exact tile; GRU backward with one whole and one partial group
          (2, 33, 320),    # generic form above the largest small compile-time size
          (5, 33, 512)]    # KB = 8, the student's H; three row tiles
CASES = ([(s, "plain") for s in SHAPES] + [((2, 17, 128), "saturated"), ((3, 15, 192), "saturated"), ((2, 17, 128), "null_carries")])


def _run_kernels(cell, case, carries):
    """-> (outputs by name, problems found in guards / inputs / unwritten outputs)"""
    from locotouch_amd import _abi

    L, B, H = case["ig"].shape[0], case["h0"].shape[0], case["h0"].shape[1]
    ng = R.NG[cell]
    names_in = ["ig", "h0", "w_hh", "b_ih", "b_hh", "dout"] + (["c0"] if cell == "lstm" else [])
    if carries:
        names_in += ["dhn"] + (["dcn"] if cell == "lstm" else [])
    shapes_out = dict(out=(L, B, H), ws=(L, B, 4 * H), dh0=(B, H), scratch=(B, H))
    if cell == "lstm":
        shapes_out.update(cell=(L, B, H), dgates=(L, B, ng * H), dc0=(B, H))
    else:
        shapes_out.update(dig=(L, B, ng * H), dhg=(L, B, ng * H))
    bufs = {n: _guarded(case[n].shape, case[n]) for n in names_in}
    bufs.update({n: _guarded(s) for n, s in shapes_out.items()})
    v = {n: view for n, (_, view) in bufs.items()}
    v.setdefault("dhn", None)
    v.setdefault("dcn", None)
    st = _abi.stream(torch.device(DEV))
    if cell == "lstm":
        _abi.call("lt_lstm_forward", v["ig"], v["h0"], v["c0"], v["w_hh"], v["b_ih"], v["b_hh"], L, B, H, v["out"], v["cell"], v["ws"], st)
        _abi.call("lt_lstm_backward", v["dout"], v["dhn"], v["dcn"], v["out"], v["cell"], v["ws"], v["h0"], v["c0"], v["w_hh"], L, B, H,
                  v["dgates"], v["scratch"], v["dh0"], v["dc0"], st)
    else:
        _abi.call("lt_gru_forward", v["ig"], v["h0"], v["w_hh"], v["b_ih"], v["b_hh"], L, B, H, v["out"], v["ws"], st)
        _abi.call("lt_gru_backward", v["dout"], v["dhn"], v["out"], v["ws"], v["h0"], v["w_hh"], L, B, H, v["dig"], v["dhg"], v["scratch"],
                  v["dh0"], st)
    torch.cuda.synchronize()

    problems = []
    for n, (buf, view) in bufs.items():
        lo, hi = buf[:GUARD], buf[GUARD + view.numel():]
        if not (bool((lo == NAN_BITS).all()) and bool((hi == NAN_BITS).all())):
            problems.append(f"guard of {n} touched ({int((lo != NAN_BITS).sum())} words below, {int((hi != NAN_BITS).sum())} above)")
        if n in names_in:
            if not torch.equal(view.view(torch.int32).cpu(), case[n].view(torch.int32)):
                problems.append(f"input {n} changed")
        elif n != "scratch" and bool(torch.isnan(view).any()):
            problems.append(f"output {n} holds {int(torch.isnan(view).sum())} NaN of {view.numel()}")
    return {n: v[n].cpu() for n in shapes_out if n != "scratch"}, problems


@pytest.mark.parametrize("shape,variant", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{v}" for s, v in CASES])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_sequence_kernels_against_float64_per_array(cell, shape, variant):
    L, B, H = shape
    carries = variant != "null_carries"
    case = R.make_case(cell, L, B, H, seed=1000 * L + 10 * B + H, saturated=variant == "saturated")
    ref64 = R.reference(cell, case, carries=carries)
    cpu32 = R.reference(cell, case, dtype=torch.float32, carries=carries)
    gpu32 = R.reference(cell, case, dtype=torch.float32, device=DEV, carries=carries)
    got, problems = _run_kernels(cell, case, carries)
    report = R.compare(cell, got, ref64, [cpu32, gpu32])
    name, ratio = R.worst(report)
    print(f"\nSEQF64 cell={cell} shape=({L},{B},{H}) {variant}: worst ratio {ratio:.2f} at {name} | {R.format_report(report)}")
    assert not problems, problems
    bad = R.failures(report)
    assert not bad, {n: f"e_hip {e:.3e} baselines {[f'{b:.3e}' for b in eb]} ratio {r:.2f} > {R.FACTOR}" for n, (e, eb, r) in bad.items()}
