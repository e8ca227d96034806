"""The three entry points of include/lt_ppo_sym.h (`lt_sym_table_pack`, `lt_sym_gather_rows`, `lt_ppo_loss_sym`; csrc/lt_ppo_sym.hip)
straight through the C ABI.  The gather is copies, sign flips and the exact bf16 -> f32 widening: it is held to `rows[idx][:, src] * sign`
BIT FOR BIT.  The loss is held to the float64 statement of tests/ppo_sym_ref.py ARRAY BY ARRAY with the comparator, the guarded arrays
and the baselines of tests/test_hip_ppo_f64.py, unchanged:

    e_hip(X) <= 4 max(e_baseline(X)) + 4 * 2^-24        (FACTOR and EPS are tests/seq_ref.py's)

Beside that: the symmetry accumulator adds across calls, and refused calls launch nothing.  One line per loss case is printed (`-s`):
PPOF64, the worst ratio and its array, then e_hip/e_cpu32/e_gpu32[/e_seq32]=ratio per array."""
import pytest
import torch

from tests import ppo_sym_ref as S
from tests.guarded import NAN_BITS
from tests.test_hip_ppo_f64 import _Arrays, _judge, _stream
from tests.test_hip_ppo_opts_f64 import LOSS_INPUTS

pytestmark = pytest.mark.gpu


def _table(G, name, src, sign):
    """the packed device table of (src, sign), written by lt_sym_table_pack into a guarded array"""
    from locotouch_amd import _abi

    D = src.numel()
    table = G.output(name, (D,))  # (int32 words src | sign bit: no NaN pattern among them)
    _abi.call("lt_sym_table_pack", src.to(torch.int32).contiguous(), sign.float().contiguous(), D, table, _stream())
    return table


def test_table_pack_writes_src_and_the_sign_bit():
    src, sign = S.signed_permutation(1024, seed=3)
    G = _Arrays()
    table = _table(G, "table", src, sign)
    problems = G.problems()
    assert not problems, problems
    words = table.view(torch.int32).cpu().to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(words & 0x7FFFFFFF, src.to(torch.int64)) and torch.equal(words >> 31, (sign < 0).to(torch.int64))


@pytest.mark.parametrize("D,m,nmb,bf16", S.GATHER_CASES, ids=[f"{d}x{m}x{n}-{'bf16' if b else 'f32'}" for d, m, n, b in S.GATHER_CASES])
def test_gather_rows_is_bit_equal(D, m, nmb, bf16):
    from locotouch_amd import _abi

    case = S.make_gather_case(D, m, nmb, bf16, seed=1000 * D + 10 * m + nmb)
    if D in (270, 348) and not bf16:  # the two task families' own tables on their own widths
        from locotouch_amd.rl.symmetry import mirror_tables
        from tests.test_symmetry_table import _Env

        t = mirror_tables(_Env("locomotion" if D == 270 else "teacher"))
        case = S.make_gather_case(D, m, nmb, bf16, seed=1000 * D + 10 * m + nmb, table=(t.policy_src.long(), t.policy_sign))
    G = _Arrays()
    rows, idx = G.input("rows", case["rows"]), G.input("idx", case["idx"])
    table = _table(G, "table", case["src"], case["sign"])
    out = G.output("out", (nmb, 2, m, D))
    assert rows.data_ptr() % 16 == 0  # (the rows BEHIND the first are aligned to their width alone: 270 floats 8 bytes, 270 bf16 4 bytes)
    _abi.call("lt_sym_gather_rows", rows, int(bf16), case["rows"].shape[0], D, idx, nmb, m, table, out, _stream())
    problems = G.problems()
    assert not problems, problems
    want = S.sym_gather(case)
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))


def _loss_call(G, case, M, A, sym_sum, suffix=""):
    from locotouch_amd import _abi

    v = {n: G.input(n + suffix, case[n]) for n in LOSS_INPUTS}
    idx = G.input("idx" + suffix, case["idx"]) if case["idx"] is not None else None
    stats = G.input("adv_stats" + suffix, case["adv_stats"]) if case.get("adv_stats") is not None else None
    table = _table(G, "act_table" + suffix, case["act_src"], case["act_sign"])
    dmu, dvalue, acc = G.output("dmu" + suffix, (2 * M, A)), G.output("dvalue" + suffix, (2 * M,)), G.output("acc" + suffix, (24,))
    out = G.output("out" + suffix, (24,), whole=False)
    _abi.call("lt_ppo_loss_sym", *[v[n] for n in LOSS_INPUTS], idx, M, A, case["clip"], case["vcoef"], case["ecoef"], case["clipped"], case["std_is_log"],
              stats, table, case["mirror_coeff"], dmu, dvalue, acc, out, sym_sum, _stream())
    G.written("out[0:6]" + suffix, out[:6])
    G.written("out[8:8+A]" + suffix, out[8:8 + A])
    return dmu, dvalue, acc, out


@pytest.mark.parametrize("M,A,clipped,variant,opts,coeff", S.SYM_CASES, ids=[f"{m}x{a}-c{c}-{v}-{o}-k{k}" for m, a, c, v, o, k in S.SYM_CASES])
def test_ppo_loss_sym(M, A, clipped, variant, opts, coeff):
    case = S.sym_case(M, A, clipped, variant, opts, coeff)
    G = _Arrays()
    sym_sum = G.state("sym_sum", torch.tensor([0.25]))
    dmu, dvalue, acc, out = _loss_call(G, case, M, A, sym_sum)
    got = dict(dmu=dmu, dvalue=dvalue, acc_surrogate=acc[0], acc_value_loss=acc[1], acc_kl=acc[2], acc_sym=acc[3], acc_dstd=acc[4:4 + A], amax_mu=acc[20],
               amax_v=acc[21], loss=out[0], surrogate=out[1], value_loss=out[2], entropy=out[3], kl=out[4], symmetry=out[5], dstd=out[8:8 + A])
    _judge(f"lt_ppo_loss_sym ({M},{A}) clipped={clipped} {variant} {opts} coeff={coeff}", S.ppo_loss_sym, case, got, G.problems())
    assert float(sym_sum) == float(torch.tensor(0.25) + out[5].cpu())  # one float32 addition to what the accumulator held
    assert int((out.view(torch.int32) == NAN_BITS).sum()) == 24 - 6 - A  # every other word of `out` is left alone


def test_symmetry_accumulator_adds_across_two_calls():
    M, A = 257, 12
    a, b = S.sym_case(M, A, 1, "index", "both", 0.5), S.sym_case(255, A, 0, "index", "plain", 0.0)
    G = _Arrays()
    sym_sum = G.state("sym_sum", torch.zeros(1))
    out_a = _loss_call(G, a, M, A, sym_sum, suffix="_a")[3]
    out_b = _loss_call(G, b, 255, A, sym_sum, suffix="_b")[3]
    none = _loss_call(G, b, 255, A, None, suffix="_c")[3]  # no accumulator: the scalars are the same, nothing is added
    problems = G.problems()
    assert not problems, problems
    assert float(sym_sum) == float(out_a[5].cpu() + out_b[5].cpu()) and float(out_a[5]) > 0.0 and float(out_b[5]) > 0.0
    assert torch.equal(none[:6].view(torch.int32), out_b[:6].view(torch.int32))


def test_refused_calls_launch_nothing():
    """A bad table, D = 0, D = 1025, A = 17 and a misaligned pointer: LT_EINVAL with the stated text, and every output still holds the
    NaN pattern it started with."""
    from locotouch_amd import _abi

    M, A, D = 64, 12, 270
    case = S.sym_case(M, A, 1, "plain", "both", 0.5)
    G = _Arrays()
    v = {n: G.input(n, case[n]) for n in LOSS_INPUTS}
    stats_in = G.input("adv_stats", case["adv_stats"])
    good_table = _table(G, "good_table", case["act_src"], case["act_sign"])
    rows, idx = G.input("rows", torch.randn(2 * M, D)), G.input("idx", torch.randperm(2 * M)[:M])
    src, sign = S.signed_permutation(D, seed=1)
    row_table = _table(G, "row_table", src, sign)
    outs = [G.output(n, s, whole=False) for n, s in (("dmu", (2 * M, A)), ("dvalue", (2 * M,)), ("acc", (24,)), ("out", (24,)), ("sym_sum", (1,)),
                                                      ("table", (1025,)), ("gathered", (1, 2, M, D)))]
    dmu, dvalue, acc, out, sym_sum, table, gathered = outs
    head = [v[n] for n in LOSS_INPUTS]
    tail = [case["clip"], case["vcoef"], case["ecoef"], 1, 1, stats_in, good_table, 0.5, dmu, dvalue, acc, out, sym_sum, _stream()]

    def refused(text, name, *args):
        with pytest.raises(RuntimeError) as e:
            _abi.call(name, *args)
        assert f"code {_abi.CONSTS['LT_EINVAL']}" in str(e.value) and text in str(e.value), str(e.value)

    i32 = lambda t: t.to(torch.int32).contiguous()  # noqa: E731
    twice = src.clone()
    twice[5] = twice[6]
    half = sign.clone()
    half[7] = 0.5
    refused("lt_sym_table_pack: invalid argument: src must be a permutation of 0 .. D - 1", "lt_sym_table_pack", i32(twice), sign, D, table, _stream())
    refused("lt_sym_table_pack: invalid argument: sign must be +1 or -1 in every column", "lt_sym_table_pack", i32(src), half, D, table, _stream())
    refused("lt_sym_table_pack: invalid argument: D must be in [1, 1024]", "lt_sym_table_pack", i32(src), sign, 0, table, _stream())
    wide = torch.arange(1025)
    refused("lt_sym_table_pack: invalid argument: D must be in [1, 1024]", "lt_sym_table_pack", i32(wide), torch.ones(1025), 1025, table, _stream())
    refused("lt_sym_table_pack: invalid argument: table must be non-null and 4-byte aligned", "lt_sym_table_pack", i32(src), sign, D, table.data_ptr() + 2, _stream())
    refused("lt_sym_gather_rows: invalid argument: D must be in [1, 1024]", "lt_sym_gather_rows", rows, 0, 2 * M, 0, idx, 1, M, row_table, gathered, _stream())
    refused("lt_sym_gather_rows: invalid argument: D must be in [1, 1024]", "lt_sym_gather_rows", rows, 0, 2 * M, 1025, idx, 1, M, row_table, gathered, _stream())
    refused("lt_sym_gather_rows: invalid argument: rows must be non-null and 4-byte aligned", "lt_sym_gather_rows", rows.data_ptr() + 2, 0, 2 * M, D, idx, 1, M,
            row_table, gathered, _stream())
    refused("lt_sym_gather_rows: invalid argument: out must be non-null and 4-byte aligned", "lt_sym_gather_rows", rows, 0, 2 * M, D, idx, 1, M, row_table,
            gathered.data_ptr() + 1, _stream())
    refused("lt_ppo_loss_sym: invalid argument: A must be in [1, 16]", "lt_ppo_loss_sym", *head, None, M, 17, *tail)
    refused("lt_ppo_loss_sym: invalid argument: adv must be non-null and 4-byte aligned", "lt_ppo_loss_sym",
            *[v[n].data_ptr() + 2 if n == "adv" else v[n] for n in LOSS_INPUTS], None, M, A, *tail)
    refused("lt_ppo_loss_sym: invalid argument: act_table must be non-null and 4-byte aligned", "lt_ppo_loss_sym", *head, None, M, A, *tail[:6], None, *tail[7:])
    problems = G.problems()
    assert not problems, problems
    for t in outs:
        assert bool((t.view(torch.int32) == NAN_BITS).all())
