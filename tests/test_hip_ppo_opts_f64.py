"""The three entry points of include/lt_ppo_opts.h (`lt_std_from_log`, `lt_ppo_loss_opts`, `lt_adv_stats`; csrc/lt_ppo.hip) straight
through the C ABI, held to the float64 statements of tests/ppo_opts_ref.py ARRAY BY ARRAY with the comparator, the guarded arrays and
the baselines of tests/test_hip_ppo_f64.py, unchanged:

    e_hip(X) <= 4 max(e_baseline(X)) + 4 * 2^-24        (FACTOR and EPS are tests/seq_ref.py's)

Beside that: `lt_ppo_loss_opts(0, NULL)` leaves the bits `lt_ppo_loss` leaves, and refused calls launch nothing.  One line per case is
printed (`-s`): PPOF64, the worst ratio and its array, then e_hip/e_cpu32/e_gpu32[/e_seq32]=ratio per array."""
import pytest
import torch

from tests import ppo_opts_ref as O
from tests import ppo_ref as R
from tests.guarded import NAN_BITS
from tests.test_hip_ppo_f64 import _Arrays, _judge, _stream

pytestmark = pytest.mark.gpu
LOSS_INPUTS = ("mu", "std", "value", "actions", "old_logp", "adv", "returns", "old_values", "old_mu", "old_sigma")


def _loss_call(G, case, M, A, entry="lt_ppo_loss_opts", suffix=""):
    """the guarded arrays of one loss call and the call itself -> (dmu, dvalue, acc, out)"""
    from locotouch_amd import _abi

    v = {n: G.input(n + suffix, case[n]) for n in LOSS_INPUTS}
    idx = G.input("idx" + suffix, case["idx"]) if case["idx"] is not None else None
    stats = G.input("adv_stats" + suffix, case["adv_stats"]) if case.get("adv_stats") is not None else None
    dmu, dvalue, acc = G.output("dmu" + suffix, (M, A)), G.output("dvalue" + suffix, (M,)), G.output("acc" + suffix, (24,))
    out = G.output("out" + suffix, (24,), whole=False)
    head = [v[n] for n in LOSS_INPUTS] + [idx, M, A, case["clip"], case["vcoef"], case["ecoef"], case["clipped"]]
    opts = [case["std_is_log"], stats] if entry == "lt_ppo_loss_opts" else []
    _abi.call(entry, *head, *opts, dmu, dvalue, acc, out, _stream())
    G.written("out[0:5]" + suffix, out[:5])
    G.written("out[8:8+A]" + suffix, out[8:8 + A])
    return dmu, dvalue, acc, out


@pytest.mark.parametrize("M,A,clipped,variant,opts", O.OPTS_CASES, ids=[f"{m}x{a}-c{c}-{v}-{o}" for m, a, c, v, o in O.OPTS_CASES])
def test_ppo_loss_opts(M, A, clipped, variant, opts):
    case = O.opts_case(M, A, clipped, variant, opts)
    G = _Arrays()
    dmu, dvalue, acc, out = _loss_call(G, case, M, A)
    got = dict(dmu=dmu, dvalue=dvalue, acc_surrogate=acc[0], acc_value_loss=acc[1], acc_kl=acc[2], acc_dstd=acc[4:4 + A], amax_mu=acc[20],
               amax_v=acc[21], loss=out[0], surrogate=out[1], value_loss=out[2], entropy=out[3], kl=out[4], dstd=out[8:8 + A])
    _judge(f"lt_ppo_loss_opts ({M},{A}) clipped={clipped} {variant} {opts}", O.ppo_loss_opts, case, got, G.problems())


def test_ppo_loss_opts_with_both_options_off_leaves_the_bits_of_ppo_loss():
    """One block (M = 255: the sums of a single block meet in one fixed order; several blocks add through float atomics in any order,
    in either entry), the index form.  Every output word, the unwritten ones of `out` included."""
    M, A = 255, 12
    case = O.make_opts_case(M, A, seed=41, clipped=1, std_is_log=False, normalise=False, rows=3 * M, vcoef=0.5)
    G = _Arrays()
    a = _loss_call(G, case, M, A, entry="lt_ppo_loss", suffix="_a")
    b = _loss_call(G, case, M, A, entry="lt_ppo_loss_opts", suffix="_b")
    problems = G.problems()
    assert not problems, problems
    for name, x, y in zip(("dmu", "dvalue", "acc", "out"), a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert int((a[3].view(torch.int32) == NAN_BITS).sum()) == 24 - 5 - A


@pytest.mark.parametrize("M,nmb,kind,storage", O.ADV_CASES, ids=[f"{m}x{n}-{k}{'-idx' if s else ''}" for m, n, k, s in O.ADV_CASES])
def test_adv_stats(M, nmb, kind, storage):
    from locotouch_amd import _abi

    case = O.adv_case(M, nmb, kind, storage)
    dev_adv = case["adv"].clone()
    if storage is not None:
        dev_adv[case["unread"]] = float("nan")  # rows no minibatch refers to: never read
    G = _Arrays()
    adv = G.input("adv", dev_adv)
    idx = G.input("idx", case["idx"]) if case["idx"] is not None else None
    stats = G.output("stats", (nmb, 2))
    _abi.call("lt_adv_stats", adv, idx, M, nmb, stats, _stream())
    _judge(f"lt_adv_stats ({M},{nmb}) {kind} {'idx' if storage else 'rows'}", O.adv_stats, case, dict(mean=stats[:, 0], inv_std=stats[:, 1]),
           G.problems())
    again = G.output("stats_again", (nmb, 2))
    _abi.call("lt_adv_stats", adv, idx, M, nmb, again, _stream())
    torch.cuda.synchronize()
    assert torch.equal(stats.view(torch.int32), again.view(torch.int32)), "a fixed summation order gives the same bits every run"


@pytest.mark.parametrize("A", [1, 12, 16])
def test_std_from_log(A):
    from locotouch_amd import _abi

    case = O.make_log_std_case(A, seed=A)
    G = _Arrays()
    log_std, std = G.input("log_std", case["log_std"]), G.output("std", (A,))
    _abi.call("lt_std_from_log", log_std, A, std, _stream())
    _judge(f"lt_std_from_log ({A})", O.std_from_log, case, dict(std=std), G.problems())


def test_refused_calls_launch_nothing():
    """M == 1 for the statistics, A == 17 and a misaligned pointer: LT_EINVAL with the stated text, and every output still holds the
    NaN pattern it started with."""
    from locotouch_amd import _abi

    M, A = 64, 12
    case = O.make_opts_case(M, A, seed=5, clipped=1, std_is_log=True, normalise=True)
    G = _Arrays()
    v = {n: G.input(n, case[n]) for n in LOSS_INPUTS}
    stats_in = G.input("adv_stats", case["adv_stats"])
    outs = [G.output(n, s, whole=False) for n, s in (("dmu", (M, A)), ("dvalue", (M,)), ("acc", (24,)), ("out", (24,)), ("stats", (4, 2)), ("std_out", (16,)))]
    dmu, dvalue, acc, out, stats, std = outs
    head = [v[n] for n in LOSS_INPUTS]
    tail = [case["clip"], case["vcoef"], case["ecoef"], 1, 1, stats_in, dmu, dvalue, acc, out, _stream()]
    wide = G.input("wide", torch.randn(M + 1))

    def refused(text, name, *args):
        with pytest.raises(RuntimeError) as e:
            _abi.call(name, *args)
        assert f"code {_abi.CONSTS['LT_EINVAL']}" in str(e.value) and text in str(e.value), str(e.value)

    refused("lt_adv_stats: invalid argument: M must be >= 2", "lt_adv_stats", v["adv"], None, 1, 4, stats, _stream())
    refused("lt_adv_stats: invalid argument: adv must be non-null and 4-byte aligned", "lt_adv_stats", v["adv"].data_ptr() + 2, None, 16, 4, stats, _stream())
    refused("lt_ppo_loss_opts: invalid argument: A must be in [1, 16]", "lt_ppo_loss_opts", *head, None, M, 17, *tail)
    refused("lt_ppo_loss_opts: invalid argument: adv must be non-null and 4-byte aligned", "lt_ppo_loss_opts",
            *[wide.data_ptr() + 2 if n == "adv" else v[n] for n in LOSS_INPUTS], None, M, A, *tail)
    refused("lt_std_from_log: invalid argument: A must be in [1, 16]", "lt_std_from_log", v["std"], 17, std, _stream())
    refused("lt_std_from_log: invalid argument: std must be non-null and 4-byte aligned", "lt_std_from_log", v["std"], A, std.data_ptr() + 1, _stream())
    problems = G.problems()
    assert not problems, problems
    for t in outs:
        assert bool((t.view(torch.int32) == NAN_BITS).all())
