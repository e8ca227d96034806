"""The PPO-update entry points of csrc/lt_ppo.hip, straight through the C ABI (`lt_ppo_loss`, `lt_ppo_lr_rule`, `lt_gae`,
`lt_adam_clip_step(_dev)`, `lt_elu_backward_bias(2)`, `lt_head_wgrad`, `lt_partial_sums`), held to the float64 oracle of
tests/ppo_ref.py ARRAY BY ARRAY.  Per array X the kernel passes when

    e_hip(X) <= 4 max(e_baseline(X)) + 4 * 2^-24        (FACTOR and EPS are tests/seq_ref.py's)

with e(X) = max |X - X64| / max |X64| for elementwise outputs and max |X - X64| / sum |summands of X64| for reduced ones (means, sums,
dstd, db, dw, grad_norm^2, the partial sums).  The baselines are the same plain-torch text in float32 on the CPU and on the GPU and, for
reduced outputs, the float32 sum in row order.  Three things are held with NO tolerance: acc[20] / acc[21] of lt_ppo_loss against the
maxima of the kernel's own dmu / dvalue, amax_blocks of lt_elu_backward_bias2 against the kernel's own dz block by block, and
lt_ppo_lr_rule against the same rule in numpy.float32.

Every input, output and workspace is a view into a larger allocation with 64 words of a NaN bit pattern on each side; outputs and
workspaces start as that NaN.  After the calls every guard and every input is bit-identical and no output holds a NaN.

One line per case is printed (`-s`): PPOF64, the worst ratio and its array, then e_hip/e_cpu32/e_gpu32[/e_seq32]=ratio per array;
DESIGN.md records them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ppo_ref as R
from tests.guarded import DEV, NAN_BITS, guard_problem, guarded, guarded_like

pytestmark = pytest.mark.gpu
F32 = torch.float32


class _Arrays:
    """the guarded device arrays of one case"""

    def __init__(self):
        self.bufs, self.inputs, self.checked = {}, {}, []

    def input(self, name, data):
        """an array the kernels only read: bit-identical afterwards"""
        self.inputs[name] = data
        return self.state(name, data)

    def state(self, name, data):
        """an array updated in place: holds `data` before the call"""
        self.bufs[name] = guarded(data.shape, data) if data.dtype == F32 else guarded_like(data)
        return self.bufs[name][1]

    def output(self, name, shape, whole=True):
        """starts as NaN; `whole`: every element is written (else the test says which with `written`)"""
        self.bufs[name] = guarded(shape)
        if whole:
            self.checked.append((name, self.bufs[name][1]))
        return self.bufs[name][1]

    def written(self, name, view):
        self.checked.append((name, view))

    def problems(self):
        torch.cuda.synchronize()
        out = [p for p in (guard_problem(n, buf, view) for n, (buf, view) in self.bufs.items()) if p]
        for n, data in self.inputs.items():
            if not torch.equal(self.bufs[n][1].cpu().contiguous().view(torch.uint8), data.contiguous().view(torch.uint8)):
                out.append(f"input {n} changed")
        for n, view in self.checked:
            if bool(torch.isnan(view).any()):
                out.append(f"output {n} holds {int(torch.isnan(view).sum())} NaN of {view.numel()}")
        return out


def _stream():
    from locotouch_amd import _abi

    return _abi.stream(torch.device(DEV))


def _judge(tag, fn, case, got, problems, block_rows=None, cut=None):
    """print the case's line; then guards, exact checks and the comparator, in that order.  `cut`: applied to the oracle's and the
    baselines' results (a job of lt_partial_sums that keeps only its first elements)."""
    cut = cut or (lambda r: r)
    ref64, cpu32, gpu32 = cut(fn(case)), cut(fn(case, dtype=F32)), cut(fn(case, dtype=F32, device=DEV))
    got = {k: v.detach().cpu() for k, v in got.items()}
    report = R.compare(got, ref64, [cpu32, gpu32, R.sequential(cpu32)])
    name, ratio = R.worst(report)
    exact = R.exact_problems(got, block_rows)
    checked = [n for n in R.EXACT_ONLY if n in got]
    print(f"\nPPOF64 {tag}: worst ratio {ratio:.2f} at {name} | {R.format_report(report)}"
          + (f" | exact {'/'.join(checked)}: {'differ' if exact else 'equal'}" if checked else ""))
    assert not problems, problems
    assert not exact, exact
    bad = R.failures(report)
    assert not bad, {n: f"e_hip {e:.3e} baselines {[f'{b:.3e}' for b in eb]} ratio {r:.2f} > {R.FACTOR}" for n, (e, eb, r) in bad.items()}
    return ratio


# ---- lt_ppo_loss -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,A,clipped,variant", R.LOSS_CASES, ids=[f"{m}x{a}-c{c}-{v}" for m, a, c, v in R.LOSS_CASES])
def test_ppo_loss(M, A, clipped, variant):
    from locotouch_amd import _abi

    case = R.loss_case(M, A, clipped, variant)
    G = _Arrays()
    v = {n: G.input(n, case[n]) for n in ("mu", "std", "value", "actions", "old_logp", "adv", "returns", "old_values", "old_mu", "old_sigma")}
    idx = G.input("idx", case["idx"]) if case["idx"] is not None else None
    dmu, dvalue, acc = G.output("dmu", (M, A)), G.output("dvalue", (M,)), G.output("acc", (24,))  # (the call clears all 24 of acc)
    out = None if variant == "no_out" else G.output("out", (24,), whole=False)
    _abi.call("lt_ppo_loss", v["mu"], v["std"], v["value"], v["actions"], v["old_logp"], v["adv"], v["returns"], v["old_values"], v["old_mu"],
              v["old_sigma"], idx, M, A, case["clip"], case["vcoef"], case["ecoef"], case["clipped"], dmu, dvalue, acc, out, _stream())
    got = dict(dmu=dmu, dvalue=dvalue, acc_surrogate=acc[0], acc_value_loss=acc[1], acc_kl=acc[2], acc_dstd=acc[4:4 + A], amax_mu=acc[20],
               amax_v=acc[21])
    if out is not None:
        G.written("out[0:5]", out[:5])
        G.written("out[8:8+A]", out[8:8 + A])
        got.update(loss=out[0], surrogate=out[1], value_loss=out[2], entropy=out[3], kl=out[4], dstd=out[8:8 + A])
    _judge(f"lt_ppo_loss ({M},{A}) clipped={clipped} {variant}", R.ppo_loss, case, got, G.problems())


# ---- lt_ppo_lr_rule --------------------------------------------------------------------------------------------------------------------
_f = np.float32
_D = 0.01  # desired KL
LR_CASES = [  # (name, kl or None, desired, lr before, A, scalars given, calls)
    *[(f"kl_above_2d_lr{lr:g}", 0.03, _D, lr, 12, True, 1) for lr in (1e-3, 3.7e-4, 5.123e-3, 2.5e-5)],   # lr / 1.5: a true division
    *[(f"kl_below_half_d_lr{lr:g}", 0.004, _D, lr, 12, True, 1) for lr in (1e-3, 3.7e-4, 5.123e-3)],
    ("kl_exactly_2d", float(_f(_D) * _f(2)), _D, 1e-3, 12, True, 1), ("kl_exactly_half_d", float(_f(_D) * _f(0.5)), _D, 1e-3, 12, True, 1),
    ("kl_zero", 0.0, _D, 1e-3, 12, True, 1),
    ("lr_at_min", 0.03, _D, 1e-5, 12, True, 1), ("lr_just_above_min", 0.03, _D, 1.2e-5, 12, True, 1),
    ("lr_at_max", 0.004, _D, 1e-2, 12, True, 1), ("lr_just_below_max", 0.004, _D, 9e-3, 12, True, 1),
    ("desired_zero", 0.03, 0.0, 1e-3, 12, True, 1), ("kl_null", None, _D, 1e-3, 12, True, 1),
    ("stats_over_two_calls", 0.03, _D, 1e-3, 12, True, 2),
    ("A0", 0.03, _D, 1e-3, 0, True, 1), ("A1", 0.03, _D, 1e-3, 1, True, 1), ("A16", 0.004, _D, 1e-3, 16, True, 1),
    ("scalars_null", 0.03, _D, 1e-3, 12, False, 1),
]


@pytest.mark.parametrize("name,kl,desired,lr0,A,with_scalars,calls", LR_CASES, ids=[c[0] for c in LR_CASES])
def test_ppo_lr_rule_is_bit_equal_to_numpy_float32(name, kl, desired, lr0, A, with_scalars, calls):
    """One launch per case (two where the statistics accumulate): the rate, the statistics sums and the dstd_out copy against
    `ppo_ref.lr_rule`, compared as bit patterns; dstd_out has guards right behind its A floats."""
    from locotouch_amd import _abi

    lr_min, lr_max, factor = 1e-5, 1e-2, 1.5
    gen = torch.Generator().manual_seed(len(name))
    scalars0, stats0 = torch.randn(24, generator=gen), torch.tensor([0.5, -0.25, 3.0])
    G = _Arrays()
    kl_dev = G.input("kl", torch.tensor([kl], dtype=F32)) if kl is not None else None
    scalars = G.input("scalars", scalars0) if with_scalars else None
    lr, stats, dstd_out = G.state("lr", torch.tensor([lr0], dtype=F32)), G.state("stats", stats0), G.output("dstd_out", (A,), whole=with_scalars)
    want_lr, want_stats = _f(lr0), stats0.numpy().copy()
    for _ in range(calls):
        _abi.call("lt_ppo_lr_rule", kl_dev, desired, lr_min, lr_max, factor, lr, stats, scalars, dstd_out, A, _stream())
        want_lr, want_stats = R.lr_rule(kl, desired, lr_min, lr_max, factor, want_lr, want_stats, scalars0.numpy() if with_scalars else None)
    problems = G.problems()
    bits = lambda t: np.asarray(t, dtype=_f).view(np.int32).tolist()  # noqa: E731
    got_lr, got_stats, got_dstd = lr.cpu().numpy(), stats.cpu().numpy(), dstd_out.cpu()
    print(f"\nPPOF64 lt_ppo_lr_rule {name}: lr {lr0:g} -> {float(got_lr[0]):.9g} (numpy float32 {float(want_lr):.9g}) stats {got_stats.tolist()}")
    assert not problems, problems
    assert bits(got_lr) == bits([want_lr]), (float(got_lr[0]), float(want_lr))
    assert bits(got_stats) == bits(want_stats if with_scalars else stats0.numpy())
    if with_scalars:
        assert torch.equal(got_dstd.view(torch.int32), scalars0[8:8 + A].view(torch.int32))
    else:
        assert bool((got_dstd.view(torch.int32) == NAN_BITS - (1 << 32)).all() or (got_dstd.view(torch.int32) == NAN_BITS).all())


# ---- lt_gae ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,small_rewards", R.GAE_CASES, ids=[f"{t}x{n}{'-small_rewards' if s else ''}" for t, n, s in R.GAE_CASES])
def test_gae(T, N, small_rewards):
    from locotouch_amd import _abi

    case = R.make_gae_case(T, N, seed=T + N, small_rewards=small_rewards)
    G = _Arrays()
    v = {n: G.input(n, case[n]) for n in ("rewards", "dones", "values", "last_values")}
    returns, advantages = G.output("returns", (T, N)), G.output("advantages", (T, N))
    _abi.call("lt_gae", v["rewards"], v["dones"], v["values"], v["last_values"], case["gamma"], case["lam"], T, N, returns, advantages, _stream())
    _judge(f"lt_gae ({T},{N}) {'small_rewards' if small_rewards else 'plain'}", R.gae, case, dict(returns=returns, advantages=advantages), G.problems())


# ---- lt_adam_clip_step / _dev ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,regime,variant", R.ADAM_CASES, ids=[f"{n}-{r}-{v}" for n, r, v in R.ADAM_CASES])
def test_adam_clip_step(n, regime, variant):
    from locotouch_amd import _abi

    case = R.make_adam_case(n, seed=n, regime=regime)
    G = _Arrays()
    p, g, m, v = (G.state(k, case[k]) for k in "pgmv")
    ws = G.output("ws", (_abi.load().lt_adam_clip_step_ws_floats(n),))
    norm = None if variant == "null_norm" else G.output("grad_norm", (1,))
    lr_dev = G.input("lr_dev", torch.tensor([case["lr"]], dtype=F32)) if variant == "dev" else None
    cases = [case]
    for step in range(2 if variant == "two_steps" else 1):
        c = cases[0]
        tail = (c["b1"], c["b2"], c["eps"], c["wd"], c["step"] + step, ws, norm, _stream())
        if lr_dev is not None:
            _abi.call("lt_adam_clip_step_dev", p, g, m, v, n, c["max_norm"], lr_dev, *tail)
        else:
            _abi.call("lt_adam_clip_step", p, g, m, v, n, c["max_norm"], c["lr"], *tail)
        got = dict(p=p.clone(), g=g.clone(), m=m.clone(), v=v.clone())
        for k in "pgmv":
            G.written(k, G.bufs[k][1])
        if norm is not None:
            got["grad_norm_sq"] = norm[0].double() ** 2
        if step == 0:
            _judge(f"lt_adam_clip_step ({n}) {regime} {variant}", R.adam_clip_step, c, got, G.problems())
        else:  # step 2 reads the state step 1 wrote; the oracle and every baseline run the same two steps, each on its own state
            def two(cs, dtype=torch.float64, device="cpu"):
                first = R.adam_clip_step(cs, dtype=dtype, device=device)
                return R.adam_clip_step(dict(cs, step=cs["step"] + 1, **{k: first[k] for k in "pgmv"}), dtype=dtype, device=device)

            _judge(f"lt_adam_clip_step ({n}) {regime} second_step", two, c, got, G.problems())


# ---- lt_elu_backward_bias / lt_elu_backward_bias2 --------------------------------------------------------------------------------------
def _one_sum(ws, nblk, stride, count, split, out0, out1):
    from locotouch_amd import _abi

    _abi.call("lt_partial_sums", 1, _abi.ptr_array([ws]), (ctypes.c_int * 1)(nblk), (ctypes.c_int64 * 1)(stride), (ctypes.c_int * 1)(count),
              (ctypes.c_int * 1)(split), _abi.ptr_array([out0]), _abi.ptr_array([out1]), _stream())


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("M,N", R.ELU_SHAPES, ids=[f"{m}x{n}" for m, n in R.ELU_SHAPES])
def test_elu_backward_bias(M, N, alpha):
    """`lt_elu_backward_bias` with db direct, and `lt_elu_backward_bias2` with db deferred (db == NULL, then lt_partial_sums) and the
    per-block maxima.  No case has dz aliasing da: the header allows it, but no caller in locotouch_amd/rl does it today."""
    from locotouch_amd import _abi

    lib = _abi.load()
    rows, nblk = R.elu_block_rows(), lib.lt_elu_backward_bias_nblk(M)
    assert nblk == (M + rows - 1) // rows and lib.lt_elu_backward_bias_ws_floats(M, N) == nblk * N
    case = R.make_elu_case(M, N, seed=M + N, alpha=alpha, block_rows=rows)
    G = _Arrays()
    da, a = G.input("da", case["da"]), G.input("a", case["a"])
    dz1, db1, ws1 = G.output("dz", (M, N)), G.output("db", (N,)), G.output("ws", (nblk * N,))
    _abi.call("lt_elu_backward_bias", da, a, M, N, case["alpha"], dz1, db1, ws1, _stream())
    dz2, db2, ws2, amax = G.output("dz2", (M, N)), G.output("db2", (N,)), G.output("ws2", (nblk * N,)), G.output("amax_blocks", (nblk,))
    _abi.call("lt_elu_backward_bias2", da, a, M, N, case["alpha"], dz2, None, ws2, amax, _stream())
    _one_sum(ws2, nblk, N, N, N, db2, None)
    problems = G.problems()
    _judge(f"lt_elu_backward_bias ({M},{N}) alpha={alpha} direct", R.elu_backward_bias, case, dict(dz=dz1, db=db1), problems, rows)
    _judge(f"lt_elu_backward_bias2 ({M},{N}) alpha={alpha} deferred", R.elu_backward_bias, case, dict(dz=dz2, db=db2, amax_blocks=amax), problems, rows)
    assert torch.equal(dz1, dz2) and torch.equal(db1, db2), "the direct and the deferred bias sum differ"


# ---- lt_head_wgrad ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n,k,split", R.HEAD_CASES, ids=[f"{m}x{n}x{k}{'-x_split' if s else ''}" for m, n, k, s in R.HEAD_CASES])
def test_head_wgrad(M, n, k, split):
    """Direct (dw, db given) and deferred (NULL, then lt_partial_sums over the blocks of n * k + 16 floats): the same bits.  x_split:
    the rows come from lt_split_rows, and the oracle decodes those very dwords exactly."""
    from locotouch_amd import _abi

    lib = _abi.load()
    case = R.make_head_case(M, n, k, seed=M + n + k)
    G = _Arrays()
    dy, x = G.input("dy", case["dy"]), G.input("x", case["x"])
    if split:
        xs = G.output("x_words", (M, k))
        _abi.call("lt_split_rows", x, xs, M * k, _stream())
        case = dict(case, x_words=xs.view(torch.int32).cpu())
        assert float((R.decode_split(case["x_words"]) - case["x"].double()).abs().max()) <= 2.0 ** -20 * float(case["x"].abs().max())
        x = xs
    nblk, blk = lib.lt_head_wgrad_nblk(M), n * k + 16
    assert lib.lt_head_wgrad_ws_floats(M, n, k) == nblk * blk
    dw1, db1, ws1 = G.output("dw", (n, k)), G.output("db", (n,)), G.output("ws", (nblk * blk,), whole=False)
    _abi.call("lt_head_wgrad", dy, x, int(split), M, n, k, dw1, db1, ws1, _stream())
    dw2, db2, ws2 = G.output("dw2", (n, k)), G.output("db2", (n,)), G.output("ws2", (nblk * blk,), whole=False)
    _abi.call("lt_head_wgrad", dy, x, int(split), M, n, k, None, None, ws2, _stream())
    _one_sum(ws2, nblk, blk, n * k + n, n * k, dw2, db2)
    G.written("ws[.][:n k + n]", ws1.view(nblk, blk)[:, :n * k + n])
    G.written("ws2[.][:n k + n]", ws2.view(nblk, blk)[:, :n * k + n])
    problems = G.problems()
    _judge(f"lt_head_wgrad ({M},{n},{k}) {'x_split' if split else 'f32'} direct", R.head_wgrad, case, dict(dw=dw1, db=db1), problems)
    _judge(f"lt_head_wgrad ({M},{n},{k}) {'x_split' if split else 'f32'} deferred", R.head_wgrad, case, dict(dw=dw2, db=db2), problems)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2), "the direct and the deferred sums differ"


# ---- lt_partial_sums -------------------------------------------------------------------------------------------------------------------
def test_partial_sums_one_launch_of_24_jobs():
    from locotouch_amd import _abi

    jobs = R.SUMS_JOBS
    assert len(jobs) == 24
    G = _Arrays()
    cases, ws, out0, out1 = [], [], [], []
    for j, (nblk, stride, count, split, with_out1, misaligned) in enumerate(jobs):
        case = R.make_sums_case(nblk, stride, count, seed=j)
        cases.append(case)
        if misaligned:  # one float in front: the partials start 4 bytes behind a 16-byte boundary
            w = G.input(f"ws{j}", torch.cat([torch.zeros(1), case["ws"]]))[1:]
            assert w.data_ptr() % 16 == 4
        else:
            w = G.input(f"ws{j}", case["ws"])
        ws.append(w)
        out0.append(G.output(f"out0_{j}", (split,)))
        out1.append(G.output(f"out1_{j}", (count - split,)) if with_out1 else None)
    n = len(jobs)
    _abi.call("lt_partial_sums", n, _abi.ptr_array(ws), (ctypes.c_int * n)(*[j[0] for j in jobs]), (ctypes.c_int64 * n)(*[j[1] for j in jobs]),
              (ctypes.c_int * n)(*[j[2] for j in jobs]), (ctypes.c_int * n)(*[j[3] for j in jobs]), _abi.ptr_array(out0), _abi.ptr_array(out1), _stream())
    problems = G.problems()
    for j, (nblk, stride, count, split, with_out1, misaligned) in enumerate(jobs):
        kept = count if with_out1 else split  # without out1 the elements from `split` on are dropped
        got = torch.cat([out0[j], out1[j]]) if with_out1 else out0[j]
        cut = lambda r, kept=kept: {"sum": r["sum"][:kept], "_terms": {"sum": r["_terms"]["sum"][:, :kept]}}  # noqa: E731
        _judge(f"lt_partial_sums job {j} nblk={nblk} stride={stride} count={count} split={split} out1={int(with_out1)} misaligned={int(misaligned)}",
               R.partial_sums, cases[j], dict(sum=got), problems, cut=cut)
