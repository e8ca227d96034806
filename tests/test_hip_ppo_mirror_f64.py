"""The entry points behind the mirror-loss-only PPO update straight through the C ABI: `lt_ppo_loss_mirror` (include/lt_ppo_mirror.h;
csrc/lt_ppo_sym.hip) and the pair launches with a row count per network (include/lt_mlp_rows.h; csrc/lt_mlp.hip).

The loss is held to the float64 statement of tests/ppo_mirror_ref.py ARRAY BY ARRAY with the comparator, the guarded arrays and the
baselines of tests/test_hip_ppo_f64.py, unchanged:

    e_hip(X) <= 4 max(e_baseline(X)) + 4 * 2^-24        (FACTOR and EPS are tests/seq_ref.py's)

`dvalue` is a guarded [M] array, the mirrored half of `dmu` is zero WORDS at coefficient 0, the accumulator adds across calls, and refused
calls launch nothing.

The `_rows` entries run the networks 348-(128, 64)-12 and 348-(128, 64)-1 on (m0, m1) rows into guarded arrays, so that a row written
behind a network's own m_k shows, and are held to float64 by the rule of tests/test_hip_mlp_f64.py (`mlp_ref.err`,
`f64_ratio_failures`, `F64_RATIO`): the forward in both activation formats, the chain with and without `in_amax` / `dz_split`.  At equal
rows every output is bit-equal to the equal-row entries'.  The row counts: the smallest; a partial last 16-row tile in both networks;
the first network the smaller; 513 and 1025 tiles in all, one past `pick_row_tiles`' thresholds (two and four row tiles a workgroup).

Figures on the MI355X (`-s` prints them): `lt_ppo_loss_mirror` worst ratio 1.58 of the bound 4 ((255, 16), index, `acc_dstd`); the `_rows` forward
worst ratio 5.0 to torch's fp32 (rule: 8), the chain 3.9."""
import ctypes

import pytest
import torch

from tests import mlp_ref
from tests import ppo_mirror_ref as MR
from tests.guarded import NAN_BITS, guard_problem, guarded
from tests.test_hip_mlp_f64 import _chain32, _check, _dec_split, _net, _packed, _rows
from tests.test_hip_ppo_f64 import _Arrays, _judge, _stream
from tests.test_hip_ppo_opts_f64 import LOSS_INPUTS
from tests.test_hip_ppo_sym_f64 import _table

pytestmark = pytest.mark.gpu


# ---- lt_ppo_loss_mirror ----------------------------------------------------------------------------------------------------------------
def _loss_call(G, case, M, A, sym_sum, suffix=""):
    from locotouch_amd import _abi

    v = {n: G.input(n + suffix, case[n]) for n in LOSS_INPUTS}
    assert v["mu"].shape == (2 * M, A) and v["value"].shape == (M,)
    idx = G.input("idx" + suffix, case["idx"]) if case["idx"] is not None else None
    stats = G.input("adv_stats" + suffix, case["adv_stats"]) if case.get("adv_stats") is not None else None
    table = _table(G, "act_table" + suffix, case["act_src"], case["act_sign"])
    dmu, dvalue, acc = G.output("dmu" + suffix, (2 * M, A)), G.output("dvalue" + suffix, (M,)), G.output("acc" + suffix, (24,))
    out = G.output("out" + suffix, (24,), whole=False)
    _abi.call("lt_ppo_loss_mirror", *[v[n] for n in LOSS_INPUTS], idx, M, A, case["clip"], case["vcoef"], case["ecoef"], case["clipped"], case["std_is_log"],
              stats, table, case["mirror_coeff"], dmu, dvalue, acc, out, sym_sum, _stream())
    G.written("out[0:6]" + suffix, out[:6])
    G.written("out[8:8+A]" + suffix, out[8:8 + A])
    return dmu, dvalue, acc, out


def _arrays_of(dmu, dvalue, acc, out, A):
    return dict(dmu=dmu, dvalue=dvalue, acc_surrogate=acc[0], acc_value_loss=acc[1], acc_kl=acc[2], acc_sym=acc[3], acc_dstd=acc[4:4 + A], amax_mu=acc[20],
                amax_v=acc[21], loss=out[0], surrogate=out[1], value_loss=out[2], entropy=out[3], kl=out[4], symmetry=out[5], dstd=out[8:8 + A])


@pytest.mark.parametrize("M,A,clipped,variant,opts,coeff", MR.MIRROR_CASES, ids=[f"{m}x{a}-c{c}-{v}-{o}-k{k}" for m, a, c, v, o, k in MR.MIRROR_CASES])
def test_ppo_loss_mirror(M, A, clipped, variant, opts, coeff):
    case = MR.mirror_case(M, A, clipped, variant, opts, coeff)
    G = _Arrays()
    sym_sum = G.state("sym_sum", torch.tensor([0.25]))
    dmu, dvalue, acc, out = _loss_call(G, case, M, A, sym_sum)
    _judge(f"lt_ppo_loss_mirror ({M},{A}) clipped={clipped} {variant} {opts} coeff={coeff}", MR.ppo_loss_mirror, case, _arrays_of(dmu, dvalue, acc, out, A),
           G.problems())
    assert float(sym_sum) == float(torch.tensor(0.25) + out[5].cpu())  # one float32 addition to what the accumulator held
    assert int((out.view(torch.int32) == NAN_BITS).sum()) == 24 - 6 - A  # every other word of `out` is left alone
    if coeff == 0.0:
        assert bool((dmu[M:].view(torch.int32) == 0).all()), "the mirrored rows of dmu must be +0.0 in every word"
    else:
        assert bool((dmu[M:] != 0).any())


def test_gradient_maximum_sees_the_mirrored_rows():
    """At the seeded cases' coefficient 0.5 the largest |dmu| lies in the scored rows; at `AMAX_COEFF` it lies in the mirrored ones, and
    acc[20] (held to the kernel's own dmu with no tolerance) must be theirs."""
    M, A = 257, 12
    case = dict(MR.mirror_case(M, A, 1, "index", "both", 0.5), mirror_coeff=MR.AMAX_COEFF)
    G = _Arrays()
    dmu, dvalue, acc, out = _loss_call(G, case, M, A, None)
    _judge(f"lt_ppo_loss_mirror ({M},{A}) coeff={MR.AMAX_COEFF}", MR.ppo_loss_mirror, case, _arrays_of(dmu, dvalue, acc, out, A), G.problems())
    assert float(acc[20]) == float(dmu[M:].abs().max()) > 2.0 * float(dmu[:M].abs().max())


def test_symmetry_accumulator_adds_across_two_calls():
    M, A = 257, 12
    a, b = MR.mirror_case(M, A, 1, "index", "both", 0.5), MR.mirror_case(255, A, 0, "index", "plain", 0.0)
    G = _Arrays()
    sym_sum = G.state("sym_sum", torch.zeros(1))
    out_a = _loss_call(G, a, M, A, sym_sum, suffix="_a")[3]
    out_b = _loss_call(G, b, 255, A, sym_sum, suffix="_b")[3]
    none = _loss_call(G, b, 255, A, None, suffix="_c")[3]  # no accumulator: the scalars are the same, nothing is added
    problems = G.problems()
    assert not problems, problems
    assert float(sym_sum) == float(out_a[5].cpu() + out_b[5].cpu()) and float(out_a[5]) > 0.0 and float(out_b[5]) > 0.0
    assert torch.equal(none[:6].view(torch.int32), out_b[:6].view(torch.int32))


def test_refused_loss_calls_launch_nothing():
    """A = 17, M = 0, a misaligned input, a missing table, a non-finite coefficient: LT_EINVAL with the stated text, and every output still
    holds the NaN pattern it started with."""
    from locotouch_amd import _abi

    M, A = 64, 12
    case = MR.mirror_case(M, A, 1, "plain", "both", 0.5)
    G = _Arrays()
    v = {n: G.input(n, case[n]) for n in LOSS_INPUTS}
    stats_in = G.input("adv_stats", case["adv_stats"])
    good_table = _table(G, "good_table", case["act_src"], case["act_sign"])
    outs = [G.output(n, s, whole=False) for n, s in (("dmu", (2 * M, A)), ("dvalue", (M,)), ("acc", (24,)), ("out", (24,)), ("sym_sum", (1,)))]
    dmu, dvalue, acc, out, sym_sum = outs
    head = [v[n] for n in LOSS_INPUTS]
    tail = [case["clip"], case["vcoef"], case["ecoef"], 1, 1, stats_in, good_table, 0.5, dmu, dvalue, acc, out, sym_sum, _stream()]

    def refused(text, *args):
        with pytest.raises(RuntimeError) as e:
            _abi.call("lt_ppo_loss_mirror", *args)
        assert f"code {_abi.CONSTS['LT_EINVAL']}" in str(e.value) and text in str(e.value), str(e.value)

    refused("lt_ppo_loss_mirror: invalid argument: A must be in [1, 16]", *head, None, M, 17, *tail)
    refused("lt_ppo_loss_mirror: invalid argument: M must be in [1, 2^31)", *head, None, 0, A, *tail)
    refused("lt_ppo_loss_mirror: invalid argument: adv must be non-null and 4-byte aligned", *[v[n].data_ptr() + 2 if n == "adv" else v[n] for n in LOSS_INPUTS],
            None, M, A, *tail)
    refused("lt_ppo_loss_mirror: invalid argument: act_table must be non-null and 4-byte aligned", *head, None, M, A, *tail[:6], None, *tail[7:])
    refused("lt_ppo_loss_mirror: invalid argument: dvalue must be non-null and 4-byte aligned", *head, None, M, A, *tail[:9], dvalue.data_ptr() + 1, *tail[10:])
    refused("lt_ppo_loss_mirror: invalid argument: mirror_coeff must be finite", *head, None, M, A, *tail[:7], float("nan"), *tail[8:])
    problems = G.problems()
    assert not problems, problems
    for t in outs:
        assert bool((t.view(torch.int32) == NAN_BITS).all())


# ---- lt_mlp_forward_pair_rows / lt_mlp_backward_pair_rows ------------------------------------------------------------------------------
ACTOR = (348, (128, 64), 12, "elu", False)
CRITIC = (348, (128, 64), 1, "elu", False)
SPECS = (ACTOR, CRITIC)
ROWS = [(2, 1), (34, 17), (130, 65), (17, 64), (5462, 2731), (10924, 5462)]
ROW_TILES = {(5462, 2731): 2, (10924, 5462): 4}  # (every other case: one row tile a workgroup)
EQUAL_ROWS = [64, 4096]


class _Guarded:
    """output arrays between guard words that start as the NaN pattern: `problems()` names a touched guard and an unwritten element"""

    def __init__(self):
        self.bufs = {}

    def new(self, name, shape):
        self.bufs[name] = guarded(shape)
        return self.bufs[name][1]

    def problems(self):
        torch.cuda.synchronize()
        out = [p for p in (guard_problem(n, buf, view) for n, (buf, view) in self.bufs.items()) if p]
        for n, (_, view) in self.bufs.items():
            left = int((view.view(torch.int32) == NAN_BITS).sum())
            if left:
                out.append(f"{n}: {left} of {view.numel()} words not written")
        return out


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _networks():
    seqs = (_net(ACTOR, 11), _net(CRITIC, 12))
    nets = [_packed(s, sp) for s, sp in zip(seqs, SPECS)]
    for n in nets:
        n.pack_backward()
    return seqs, nets


def _forward(nets, xs, split, rows_entry):
    """the pair forward into guarded arrays through lt_mlp_forward_pair_rows, or (equal rows) through lt_mlp_forward_pair"""
    from locotouch_amd import _abi

    G = _Guarded()
    ms = [x.shape[0] for x in xs]
    ys = [G.new(f"y{k}", (ms[k], SPECS[k][2])) for k in range(2)]
    acts = [[G.new(f"act{k}.{l}", (ms[k], h)) for l, h in enumerate(SPECS[k][1])] for k in range(2)]
    head = (nets[0].desc, nets[0].packed, xs[0], nets[1].desc, nets[1].packed, xs[1])
    tail = (ys[0], ys[1], _ptrs(acts[0]), _ptrs(acts[1]), int(split), _stream())
    if rows_entry:
        _abi.call("lt_mlp_forward_pair_rows", *head, ms[0], ms[1], *tail)
    else:
        assert ms[0] == ms[1]
        _abi.call("lt_mlp_forward_pair", *head, ms[0], *tail)
    problems = G.problems()
    assert not problems, problems
    return ys, acts


def _blocks(nets, ms):
    from locotouch_amd import _abi

    b = (ctypes.c_int64(), ctypes.c_int64())
    _abi.call("lt_mlp_backward_blocks_rows", nets[0].desc, nets[1].desc, ms[0], ms[1], ctypes.byref(b[0]), ctypes.byref(b[1]))
    return b[0].value, b[1].value


def _backward(nets, dys, acts32, scaled, rows_entry):
    """the chain into guarded arrays; `scaled`: one scale per network from the global max |dy| (`in_amax`) and dz in the split format"""
    from locotouch_amd import _abi

    G = _Guarded()
    ms = [d.shape[0] for d in dys]
    nblk = _blocks(nets, ms)
    if not rows_entry:
        assert ms[0] == ms[1] and nblk == (_abi.load().lt_mlp_backward_blocks(ctypes.byref(nets[0].desc), ctypes.byref(nets[1].desc), ms[0]),) * 2
    dzs = [[G.new(f"dz{k}.{l}", tuple(a.shape)) for l, a in enumerate(acts32[k])] for k in range(2)]
    amax = [[G.new(f"amax{k}.{l}", (nblk[k],)) for l in range(len(acts32[k]))] for k in range(2)]
    scales = G.new("scales", (2,)) if scaled else None
    in_amax = [d.abs().max().view(1) for d in dys] if scaled else [None, None]
    sat = torch.zeros(1, device="cuda:0")
    args = [nets[0].desc, nets[0].bpacked, dys[0], _ptrs(acts32[0]), _ptrs(dzs[0]), _ptrs(amax[0]),
            nets[1].desc, nets[1].bpacked, dys[1], _ptrs(acts32[1]), _ptrs(dzs[1]), _ptrs(amax[1])]
    tail = [0, in_amax[0], in_amax[1], int(scaled), scales, sat, _stream()]
    if rows_entry:
        _abi.call("lt_mlp_backward_pair_rows", *args, ms[0], ms[1], *tail)
    else:
        _abi.call("lt_mlp_backward_pair", *args, ms[0], *tail)
    problems = G.problems()
    assert not problems, problems
    assert float(sat) == 0.0
    return dzs, amax, scales, nblk


def _inputs(ms):
    xs = [_rows(SPECS[k], ms[k], 7 + k) for k in range(2)]
    g = torch.Generator(device="cuda:0").manual_seed(ms[0] + ms[1])
    dys = [torch.randn(ms[k], SPECS[k][2], device="cuda:0", generator=g) * 1e-3 for k in range(2)]
    dys[0][::53] *= 200.0  # heavy-tailed rows, as PPO's are
    return xs, dys


@pytest.mark.parametrize("split", [False, True], ids=["f32", "split"])
@pytest.mark.parametrize("m0,m1", ROWS, ids=[f"{a}x{b}" for a, b in ROWS])
def test_forward_pair_rows_matches_float64(m0, m1, split):
    seqs, nets = _networks()
    xs, _ = _inputs((m0, m1))
    ys, acts = _forward(nets, xs, split, rows_entry=True)
    e_hip, e_f32 = {}, {}
    for k in range(2):
        y64, a64 = mlp_ref.forward64(seqs[k], xs[k])
        y32, a32 = mlp_ref.forward32(seqs[k], xs[k])
        e_hip[f"y{k}"], e_f32[f"y{k}"] = mlp_ref.err(ys[k], y64), mlp_ref.err(y32, y64)
        for l, (got, r64, r32) in enumerate(zip(acts[k], a64, a32)):
            e_hip[f"act{k}.{l}"], e_f32[f"act{k}.{l}"] = mlp_ref.err(_dec_split(got) if split else got, r64), mlp_ref.err(r32, r64)
    _check(f"rows-fwd-{m0}x{m1}", "lt_mlp_forward_pair_rows", e_hip, e_f32, "split" if split else "f32")


@pytest.mark.parametrize("scaled", [False, True], ids=["scale_per_workgroup", "in_amax_dz_split"])
@pytest.mark.parametrize("m0,m1", ROWS, ids=[f"{a}x{b}" for a, b in ROWS])
def test_backward_pair_rows_matches_float64(m0, m1, scaled):
    seqs, nets = _networks()
    ms = (m0, m1)
    xs, dys = _inputs(ms)
    acts32 = [[a.float().contiguous() for a in mlp_ref.forward64(seqs[k], xs[k])[1]] for k in range(2)]  # both candidates gate with the same f32 activations
    dzs, amax, scales, nblk = _backward(nets, dys, acts32, scaled, rows_entry=True)
    rt = ROW_TILES.get(ms, 1)
    assert nblk == tuple(((m + 15) // 16 + rt - 1) // rt for m in ms)
    e_hip, e_f32 = {}, {}
    for k in range(2):
        rdz, _, _ = mlp_ref.ref_chain(seqs[k], xs[k], dys[k])
        dz32 = _chain32(seqs[k], xs[k], dys[k], acts32[k])
        for l, ref in rdz.items():
            got = _dec_split(dzs[k][l]) / scales[k].double() if scaled else dzs[k][l]
            e_hip[f"dz{k}.{l}"], e_f32[f"dz{k}.{l}"] = mlp_ref.err(got, ref), mlp_ref.err(dz32[l], ref)
            # the per-workgroup maxima lt_wgrad scales by: network k has nblk[k] of them, each its own rows'
            rows = 16 * rt
            pad = torch.zeros(nblk[k] * rows, ref.shape[1], device=ref.device, dtype=torch.float64)
            pad[:ms[k]] = got.double().abs()
            torch.testing.assert_close(amax[k][l].double(), pad.view(nblk[k], -1).max(1).values, rtol=1e-3, atol=0.0)
    _check(f"rows-bwd-{m0}x{m1}", "lt_mlp_backward_pair_rows", e_hip, e_f32, "in_amax, dz split" if scaled else "a scale per workgroup, dz f32")


@pytest.mark.parametrize("m", EQUAL_ROWS)
def test_equal_rows_are_bit_equal_to_the_equal_row_entries(m):
    seqs, nets = _networks()
    xs, dys = _inputs((m, m))
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for split in (False, True):
        new, old = _forward(nets, xs, split, rows_entry=True), _forward(nets, xs, split, rows_entry=False)
        for k in range(2):
            assert torch.equal(bits(new[0][k]), bits(old[0][k])), (split, k)
            for l in range(2):
                assert torch.equal(bits(new[1][k][l]), bits(old[1][k][l])), (split, k, l)
    acts32 = [[a.float().contiguous() for a in mlp_ref.forward64(seqs[k], xs[k])[1]] for k in range(2)]
    for scaled in (False, True):
        new, old = _backward(nets, dys, acts32, scaled, rows_entry=True), _backward(nets, dys, acts32, scaled, rows_entry=False)
        assert new[3] == old[3]
        for k in range(2):
            for l in range(2):
                assert torch.equal(bits(new[0][k][l]), bits(old[0][k][l])) and torch.equal(bits(new[1][k][l]), bits(old[1][k][l])), (scaled, k, l)
        if scaled:
            assert torch.equal(bits(new[2]), bits(old[2]))
