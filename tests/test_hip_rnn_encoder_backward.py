"""include/lt_rnn_encoder_train.h on the GPU (csrc/lt_encoder.hip).

a. `lt_rnn_encoder_forward_train`: `out` equals `lt_rnn_encoder_forward`'s and `acts` equal those of `lt_encoder_forward` on rows
   [obs[r, :flat_dim] | h[r]], bit for bit.
b. `lt_rnn_encoder_backward`: every dz_l and dh against the float64 statement of tests/rnn_encoder_backward_ref.py on the SAME stored
   activations (the training form's own f32 arrays, promoted), beside the same chain in f32 torch ops on the GPU.  Bound, per array (the
   rule of tests/test_hip_direct_recurrent_update.py): the kernel's largest error is at most max(4 x the torch chain's, 1e-5 x max |ref|).
   All three figures are printed.  Every output array stands between guard words and is NaN beforehand.
The contract: a second run, the rows shared by n = 37 and n = 70, the actor with and without a critic, and launches of 10 007 and
20 011 repeated rows (32- and 64-row blocks, where n <= 70 runs on 16-row blocks) are held to `torch.equal`; what
the host refuses is refused by its field's name before anything is launched."""
import ctypes
import re

import pytest

from tests import rnn_encoder_backward_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NMAX = 70


def _ids():
    from locotouch_amd import _abi

    C = _abi.CONSTS
    return {None: C["LT_ACT_NONE"], "elu": C["LT_ACT_ELU"], "relu": C["LT_ACT_RELU"], "tanh": C["LT_ACT_TANH"]}


class Enc:
    """One network: a seeded encoder (f32 on the device), memory rows h, observation rows, and the gradient rows dx of the stack's input
    (`flat` head columns, the embedding's E columns, `pad` floats more: row stride flat + E + pad)."""

    def __init__(self, enc_in, dims, act="elu", final="tanh", flat=0, pad=0, seed=0):
        import torch

        c = R.case(enc_in, dims, act, final, NMAX, seed=seed, dtype=torch.float32)
        self.enc_in, self.dims, self.act, self.final, self.flat = enc_in, list(dims), act, final, flat
        self.E = dims[-1]
        self.w, self.b = [w.to(DEV) for w in c["weights"]], [b.to(DEV) for b in c["biases"]]
        self.h = c["h"].to(DEV)
        gen = torch.Generator().manual_seed(77 + seed)
        self.obs_dim = flat + 3
        self.obs = torch.randn(NMAX, self.obs_dim, generator=gen).to(DEV)
        self.dx = torch.randn(NMAX, flat + self.E + pad, generator=gen).to(DEV)
        self.dx[:, flat:flat + self.E] = c["g"].to(DEV)

    def repeated(self, n):
        """The same network on n rows: its NMAX rows over and over (row r is row r % NMAX)."""
        import copy

        big = copy.copy(self)
        reps = -(-n // NMAX)
        big.h, big.obs, big.dx = (t.repeat(reps, 1)[:n].contiguous() for t in (self.h, self.obs, self.dx))
        assert big.dx.stride(0) == self.dx.stride(0)
        return big

    def net(self, out, acts=()):
        from locotouch_amd import _abi

        ids = _ids()
        n = _abi.LtRnnEncoderNet()
        n.obs_dim, n.flat_dim, n.enc_in, n.num_layers = self.obs_dim, self.flat, self.enc_in, len(self.dims)
        for l, w in enumerate(self.dims):
            n.dims[l], n.weight[l], n.bias[l] = w, self.w[l].data_ptr(), self.b[l].data_ptr()
        n.activation, n.final_activation = ids[self.act], ids[self.final]
        n.obs, n.obs_stride, n.h, n.h_stride, n.out = self.obs.data_ptr(), self.obs.stride(0), self.h.data_ptr(), self.h.stride(0), out.data_ptr()
        for l, a in enumerate(acts):
            n.acts[l] = a.data_ptr()
        return n

    def empty_record(self, n, train):
        import torch

        nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        count = (len(self.dims) if self.final else len(self.dims) - 1) if train else 0
        return nan(n, self.flat + self.E), [nan(n, self.dims[l]) for l in range(count)]

    def grad(self, n, out, acts, outputs=None):
        """(LtRnnEncoderGrad, [(name, allocation, view)] of its guarded outputs)."""
        from locotouch_amd import _abi
        from tests.guarded import guarded

        ids = _ids()
        g = _abi.LtRnnEncoderGrad()
        g.flat_dim, g.enc_in, g.num_layers, g.activation, g.final_activation = self.flat, self.enc_in, len(self.dims), ids[self.act], ids[self.final]
        g.dx, g.dx_stride, g.out = self.dx.data_ptr(), self.dx.stride(0), out.data_ptr()
        outs = outputs or [(f"dz[{l}]", *guarded((n, w))) for l, w in enumerate(self.dims)] + [("dh", *guarded((n, self.enc_in)))]
        for l, w in enumerate(self.dims):
            g.dims[l], g.weight[l], g.dz[l] = w, self.w[l].data_ptr(), outs[l][2].data_ptr()
        for l, a in enumerate(acts):
            g.acts[l] = a.data_ptr()
        g.dh = outs[-1][2].data_ptr()
        return g, outs


def forward_train(encs, n):
    import torch

    from locotouch_amd import _abi

    recs = [e.empty_record(n, True) for e in encs]
    nets = [e.net(out, acts) for e, (out, acts) in zip(encs, recs)]
    _abi.call("lt_rnn_encoder_forward_train", nets[0], nets[1] if len(nets) > 1 else None, n, _abi.stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return recs


def backward(encs, n, recs):
    """One launch for `encs` = (actor,) or (actor, critic) from the training form's records: per network {name: view}, after the check
    that every element was written and no guard word touched."""
    import torch

    from locotouch_amd import _abi
    from tests.guarded import guard_problem

    built = [e.grad(n, out, acts) for e, (out, acts) in zip(encs, recs)]
    _abi.call("lt_rnn_encoder_backward", built[0][0], built[1][0] if len(built) > 1 else None, n, _abi.stream(torch.device(DEV)))
    torch.cuda.synchronize()
    res = []
    for k, (_, outs) in enumerate(built):
        for name, buf, view in outs:
            assert guard_problem(name, buf, view) is None, (k, guard_problem(name, buf, view))
            assert not bool(torch.isnan(view).any()), (k, name, "an element was left unwritten")
        res.append({name: view for name, _, view in outs})
    return res


def statement(e, n, rec, dtype):
    """{name: array} of the statement on network e's stored activations, in `dtype` on the device."""
    out, acts = rec
    L = len(e.dims)
    cast = lambda t: t[:n].to(dtype)  # noqa: E731
    pre = cast(acts[L - 1]) if e.final else cast(out[:, e.flat:])
    dzs, dh = R.backward([w.to(dtype) for w in e.w], [cast(a) for a in acts[:L - 1]], pre, cast(out[:, e.flat:]),
                         cast(e.dx[:, e.flat:e.flat + e.E]), e.act, e.final)
    return {"dh": dh, **{f"dz[{l}]": d for l, d in enumerate(dzs)}}


def held_to_float64(tag, encs, n):
    import torch

    recs = forward_train(encs, n)
    got = backward(encs, n, recs)
    for k, e in enumerate(encs):
        ref, chain = statement(e, n, recs[k], torch.float64), statement(e, n, recs[k], torch.float32)
        assert set(got[k]) == set(ref)
        for name in sorted(ref):
            top = float(ref[name].abs().max())
            e_kernel = float((got[k][name].double() - ref[name]).abs().max())
            e_chain = float((chain[name].double() - ref[name]).abs().max())
            print(f"\n[rnn encoder backward {tag} n={n} net {k}] {name}: max |err| vs f64  kernel {e_kernel:.3e}  f32 torch chain {e_chain:.3e}  max |ref| {top:.3e}")
            assert top > 0 and e_kernel <= max(4.0 * e_chain, 1e-5 * top), (tag, n, k, name, e_kernel, e_chain, top)
    return recs, got


# ---- a. the training form of the forward launch ----
@pytest.mark.parametrize("n", [1, 17, 70])
def test_forward_train_equals_the_inference_form_and_the_tail_encoder_bit_for_bit(n):
    import torch

    from locotouch_amd import _abi
    from locotouch_amd.rl import encoder

    encs = [Enc(64, [32, 16, 16], "elu", "tanh", flat=5, seed=1), Enc(256, [256, 128, 64, 64], "elu", None, flat=3, seed=2)]
    recs = forward_train(encs, n)
    plain = [e.empty_record(n, False)[0] for e in encs]
    _abi.call("lt_rnn_encoder_forward", encs[0].net(plain[0]), encs[1].net(plain[1]), n, _abi.stream(torch.device(DEV)))
    ids = _ids()
    tail = []
    for e in encs:  # lt_encoder_forward, training form, on rows [obs[:, :flat] | h]
        rows = torch.cat([e.obs[:n, :e.flat], e.h[:n]], dim=1).contiguous()
        desc = encoder.make_desc(e.flat + e.enc_in, e.flat, e.enc_in, e.dims, ids[e.act], ids[e.final])
        out, acts = e.empty_record(n, True)
        tail.append((encoder.make_net(desc, rows, e.w, e.b, out, acts), out, acts, rows))  # (rows: kept alive until the launch has run)
    _abi.call("lt_encoder_forward", tail[0][0], tail[1][0], n, _abi.stream(torch.device(DEV)))
    torch.cuda.synchronize()
    for k, e in enumerate(encs):
        out, acts = recs[k]
        assert len(acts) == (len(e.dims) if e.final else len(e.dims) - 1)
        assert not bool(torch.isnan(out).any()) and torch.equal(out, plain[k]) and torch.equal(out, tail[k][1])
        assert torch.equal(out[:, :e.flat], e.obs[:n, :e.flat])
        for l, (a, b) in enumerate(zip(acts, tail[k][2])):
            assert not bool(torch.isnan(a).any()) and torch.equal(a, b), (k, l)
    # the actor alone: the same bits
    alone = forward_train(encs[:1], n)
    assert torch.equal(alone[0][0], recs[0][0]) and all(torch.equal(a, b) for a, b in zip(alone[0][1], recs[0][1]))


def test_forward_train_asks_for_every_buffer_by_name():
    from locotouch_amd import _abi

    e = Enc(64, [24, 8], "elu", "tanh")
    out, acts = e.empty_record(4, True)
    for missing, field in ((0, r"actor\.acts\[0\]"), (1, r"actor\.acts\[1\]")):
        net = e.net(out, acts)
        net.acts[missing] = None
        with pytest.raises(RuntimeError, match=r"lt_rnn_encoder_forward_train: invalid argument: " + field + " must be"):
            _abi.call("lt_rnn_encoder_forward_train", net, None, 4, None)
    plain = Enc(64, [24, 8], "elu", None)
    out, acts = plain.empty_record(4, True)
    net = plain.net(out, acts)
    net.acts[1] = out.data_ptr()  # no final activation: the embedding has no buffer
    with pytest.raises(RuntimeError, match=r"lt_rnn_encoder_forward_train: invalid argument: actor\.acts\[1\] must be NULL"):
        _abi.call("lt_rnn_encoder_forward_train", net, None, 4, None)


# ---- b. the backward launch, array by array ----
SHAPES = {"64-8": (64, [8]), "64-24-8": (64, [24, 8]), "64-32-16-16": (64, [32, 16, 16])}


@pytest.mark.parametrize("n", [1, 15, 17, 37, 70])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_backward_is_held_to_float64_at_every_row_count(shape, n):
    """n: a partial 16-row sub-tile, a partial row block, more than one block; [8] and [24, 8]: blocks of the summed index with zero
    padding; the critic of the launch is another shape each time."""
    enc_in, dims = SHAPES[shape]
    other = [s for s in SHAPES if s != shape][0]
    held_to_float64(shape, [Enc(enc_in, dims, seed=3), Enc(*SHAPES[other], "relu", "elu", flat=2, seed=4)], n)


def test_backward_at_the_reference_shape():
    held_to_float64("reference", [Enc(256, [256, 128, 64, 64], "elu", "tanh", flat=270, seed=5), Enc(256, [256, 128, 64, 64], "elu", "tanh", flat=270, seed=6)], 37)


def test_backward_with_512_wide_layers():
    held_to_float64("512", [Enc(512, [512, 16], "elu", "tanh", seed=7), Enc(64, [8, 512], "tanh", None, seed=8)], 17)


@pytest.mark.parametrize("final", R.FINALS, ids=lambda f: f"final-{f}")
@pytest.mark.parametrize("act", R.ACTS)
def test_backward_for_every_pair_of_activations(act, final):
    held_to_float64(f"{act}-{final}", [Enc(64, [24, 16, 8], act, final, seed=9), Enc(40, [16, 8], act, final, flat=1, seed=10)], 17)


@pytest.mark.parametrize("flat,pad", [(0, 0), (5, 2)], ids=["flat-0", "flat-5-stride-15"])
def test_backward_reads_the_gradient_columns_in_place(flat, pad):
    """flat 5, E 8, pad 2: rows of dx 15 floats apart, so the g columns start at 4-byte aligned addresses only."""
    e = Enc(64, [32, 16, 8], "elu", "tanh", flat=flat, pad=pad, seed=11)
    assert e.dx.stride(0) == flat + 8 + pad and (flat == 0 or e.dx.stride(0) % 2 == 1)
    held_to_float64(f"flat{flat}", [e, Enc(64, [16, 8], "relu", "relu", flat=flat, pad=pad, seed=12)], 37)


# ---- the contract ----
def test_same_bits_on_a_second_run_for_shared_rows_and_without_the_critic():
    import torch

    encs = [Enc(64, [32, 16, 16], "elu", "tanh", flat=5, pad=2, seed=13), Enc(256, [256, 128, 64, 64], "elu", "tanh", flat=3, seed=14)]
    recs70 = forward_train(encs, 70)
    a, b = backward(encs, 70, recs70), backward(encs, 70, recs70)
    for k in range(2):
        for name in a[k]:
            assert torch.equal(a[k][name], b[k][name]), (k, name)
    recs37 = forward_train(encs, 37)
    c = backward(encs, 37, recs37)
    for k in range(2):
        for name in a[k]:
            assert torch.equal(a[k][name][:37], c[k][name]), (k, name)  # a row's bits depend neither on n nor on where it stands
    alone = backward(encs[:1], 70, recs70[:1])
    for name in a[0]:
        assert torch.equal(a[0][name], alone[0][name]), name


@pytest.mark.parametrize("n,nets", [(10007, 1), (20011, 1), (10007, 2)], ids=["10007-rows-32-row-blocks", "20011-rows-64-row-blocks", "two-nets-10007-rows-64-row-blocks"])
def test_larger_batches_take_larger_row_blocks_and_keep_the_bits(n, nets):
    """The launch takes the largest row block that still gives each of the chip's 256 CUs a workgroup: one network at 10 007 rows 32-row
    blocks (313 of them; 157 blocks of 64 would not do), at 20 011 rows 64-row blocks (313), two networks at 10 007 rows 64-row blocks
    (2 x 157) - several 16-row sub-tiles per workgroup, and a ragged last block each time (10 007 = 312 x 32 + 23 = 156 x 64 + 23,
    20 011 = 312 x 64 + 43).  The rows repeat those of the n = 70 launch, which runs on 16-row blocks: every dz_l and dh keeps its bits,
    and so do the training form's arrays the backward reads."""
    import torch

    encs = [Enc(256, [256, 128, 64, 64], "elu", "tanh", flat=5, pad=2, seed=15), Enc(64, [24, 16, 8], "tanh", "elu", flat=3, seed=16)][:nets]
    recs70 = forward_train(encs, NMAX)
    small = backward(encs, NMAX, recs70)
    big_encs = [e.repeated(n) for e in encs]
    recs = forward_train(big_encs, n)
    big = backward(big_encs, n, recs)
    reps = -(-n // NMAX)
    for k in range(nets):
        assert torch.equal(recs[k][0], recs70[k][0].repeat(reps, 1)[:n]), k
        for l, (a, b) in enumerate(zip(recs[k][1], recs70[k][1])):
            assert torch.equal(a, b.repeat(reps, 1)[:n]), (k, l)
        for name in small[k]:
            assert torch.equal(big[k][name], small[k][name].repeat(reps, 1)[:n]), (k, name)


def _refused(args, field):
    from locotouch_amd import _abi

    fn, conv = _abi._calls["lt_rnn_encoder_backward"]
    rc = fn(*[x if c is None else c(x) for c, x in zip(conv, args, strict=True)])
    msg = _abi.load().lt_last_error().decode()
    assert rc == _abi.CONSTS["LT_EINVAL"], rc
    assert msg.startswith("lt_rnn_encoder_backward: invalid argument:") and re.search(rf"(?<![\w.]){re.escape(field)} must be\b", msg), msg


def test_host_refusals_name_the_field_before_anything_is_launched():
    import torch

    from locotouch_amd import _abi

    e = Enc(64, [24, 8], "elu", "tanh", flat=5, pad=2)
    n = 17
    (out, acts), = forward_train([e], n)
    lib = _abi.load()

    def grad(**kw):
        g, outs = e.grad(n, out, acts)
        keep.append(outs)
        for k, v in kw.items():
            if isinstance(v, dict):
                for l, x in v.items():
                    getattr(g, k)[l] = x
            else:
                setattr(g, k, v)
        return g

    keep = []
    good = grad()
    _refused([grad(dh=None), None, n, None], "actor.dh")
    _refused([grad(dh=keep[-1][-1][2].data_ptr() + 4), None, n, None], "actor.dh")  # 4-byte aligned only
    _refused([good, grad(dh=None), n, None], "critic.dh")
    _refused([grad(dims={0: 20}), None, n, None], "actor.dims[0]")  # not a multiple of 8
    _refused([grad(dx_stride=5 + 8 - 1), None, n, None], "actor.dx_stride")
    _refused([grad(dx=None), None, n, None], "actor.dx")
    _refused([grad(out=None), None, n, None], "actor.out")  # tanh behind the last layer reads the embedding
    _refused([grad(acts={0: None}), None, n, None], "actor.acts[0]")
    _refused([grad(dz={1: None}), None, n, None], "actor.dz[1]")
    _refused([grad(weight={0: None}), None, n, None], "actor.weight[0]")
    _refused([grad(dz={1: e.dx.data_ptr() + 4 * 15}), None, n, None], "actor.dz[1]")  # inside the rows of dx
    _refused([grad(dh=acts[0].data_ptr()), None, n, None], "actor.dh")  # an array the launch reads
    _refused([grad(dz={0: out.data_ptr()}), None, n, None], "actor.dz[0]")
    _refused([grad(dz={1: e.w[0].data_ptr()}), None, n, None], "actor.dz[1]")  # a weight is read too
    twice = grad()
    twice.dz[1] = twice.dz[0]  # two outputs in one place
    _refused([twice, None, n, None], "actor.dz[1]")
    twice = grad()
    twice.dh = twice.dz[0]
    _refused([good, twice, n, None], "critic.dh")
    _refused([good, None, 0, None], "n")
    _refused([None, None, n, None], "actor")
    assert lib.lt_rnn_encoder_backward_launches(ctypes.byref(good), None) == 1
    torch.cuda.synchronize()
