"""csrc/lt_encoder.hip (`lt_encoder_forward`): out[r] = [ obs[r, :flat_dim] | enc(obs[r, -enc_in:]) ] for one or two networks in one
launch, against the float64 restatement of tests/encoder_ref.py, beside the eager f32 composition the kernel replaces (`torch.cat` of
the slice and the `MLP` module) on the same inputs.

Bound, per output array (the rule of tests/test_hip_memory_step.py with the floor of tests/test_hip_obs_norm.py): the kernel sums the
same exact f32 products as the eager composition in another order, so its largest error against f64 may be at most the larger of TWICE
the composition's on the same inputs and one f32 ulp of the array's magnitude.  Both figures are printed.  The head columns, a second
run, the rows shared by n = 17 and n = 130 and the training form's activations are held to `torch.equal`."""
import pytest

from tests.encoder_ref import encoder_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS = (1, 17, 130)  # one row; a ragged 16-row tile; more than one row block at every block size (16, 32, 64), ragged again
# (obs_dim, flat_dim, enc_in): the synthetic case of tests/rl_synth.py; the reference's teacher rows; an odd tail offset (no 8-byte alignment)
ROWS = {"14-9-5": (14, 9, 5), "348-270-78": (348, 270, 78), "277-200-77": (277, 200, 77)}
# hidden widths, embedding width, activation, final activation
ENCODERS = {"16-8-8": ([16, 8], 8, "elu", None), "256-128-64-64-tanh": ([256, 128, 64], 64, "elu", "tanh"), "8-elu": ([], 8, "relu", "elu")}
CASES = [(r, e) for r in ROWS for e in ENCODERS]
# beside the issue's three: widths that are multiples of 8 but not of 16 (a half-empty last k block and feature tile), a 32-feature panel,
# tanh between the layers and ReLU behind them
OTHER_ENCODERS = {"32-24-16-relu": ([32, 24], 16, "tanh", "relu")}


def _ulp(x: float) -> float:
    """One f32 ulp at magnitude x."""
    import math

    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


class Net:
    """One network's module, rows and descriptor.  `pad`: extra floats between rows (a row stride larger than obs_dim)."""

    def __init__(self, rows, enc, seed, pad=0):
        import torch

        from locotouch_amd.rl import encoder
        from locotouch_amd.rl.models import MLP

        self.obs_dim, self.flat, self.enc_in = ROWS[rows]
        self.hidden, self.emb, self.act, self.final = {**ENCODERS, **OTHER_ENCODERS}[enc]
        torch.manual_seed(seed)
        self.mlp = MLP(self.enc_in, self.hidden, self.emb, activation=self.act, final_layer_activation=self.final).to(DEV)
        with torch.no_grad():
            for m in self.mlp.model:
                if isinstance(m, torch.nn.Linear):
                    m.bias.uniform_(-0.3, 0.3)
        gen = torch.Generator().manual_seed(seed + 1)
        self.store = torch.randn(max(NS), self.obs_dim + pad, generator=gen).to(DEV)
        self.obs = self.store[:, :self.obs_dim]  # a view: row stride obs_dim + pad
        self.desc, self.linears = encoder.describe(self.mlp, self.obs_dim, self.flat)
        self.weights, self.biases = [m.weight for m in self.linears], [m.bias for m in self.linears]

    def launch_net(self, n, train, desc=None):
        import torch

        from locotouch_amd.rl import encoder

        desc = self.desc if desc is None else desc
        layers = desc.num_layers
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        out = nan(n, self.flat + desc.dims[layers - 1])
        count = (layers if desc.final_activation else layers - 1) if train else 0
        acts = [nan(n, desc.dims[l]) for l in range(count)]
        return encoder.make_net(desc, self.obs, self.weights[:layers], self.biases[:layers], out, acts), out, acts

    def truncated(self, layers):
        """The first `layers` layers as an encoder of their own, the hidden activation behind the last: its embedding IS hidden value
        `layers - 1` of the whole encoder in the inference form."""
        from locotouch_amd import _abi
        from locotouch_amd.rl import encoder

        return encoder.make_desc(self.obs_dim, self.flat, self.enc_in, [m.out_features for m in self.linears[:layers]], self.desc.activation,
                                 self.desc.activation if layers < len(self.linears) else _abi.CONSTS["LT_ACT_NONE"])

    def eager(self, n):
        """The f32 composition on the same rows: (out, hidden activations, pre-activation embedding)."""
        import torch

        with torch.no_grad():
            x = self.obs[:n, self.obs_dim - self.enc_in:]
            hidden, pre, mods = [], None, list(self.mlp.model)
            for k, m in enumerate(mods):
                x = m(x)
                if isinstance(m, torch.nn.Linear) and m is self.linears[-1]:
                    pre = x
                elif not isinstance(m, torch.nn.Linear) and k < len(mods) - 1:
                    hidden.append(x)
            want = torch.cat([self.obs[:n, :self.flat], self.mlp(self.obs[:n, self.obs_dim - self.enc_in:])], dim=-1)
            assert torch.equal(want[:, self.flat:], x)
        return want, hidden, pre

    def ref(self, n):
        return encoder_ref(self.obs[:n], self.flat, self.enc_in, self.weights, self.biases, self.act, self.final)


def forward(nets, n, train=False):
    """One launch for `nets` = (actor,) or (actor, critic): [(out, acts)] per network, every output NaN beforehand."""
    import torch

    from locotouch_amd import _abi

    built = [net.launch_net(n, train) for net in nets]
    _abi.call("lt_encoder_forward", built[0][0], built[1][0] if len(built) > 1 else None, n, _abi.stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return [(out, acts) for _, out, acts in built]


def _pair(rows, enc, with_critic):
    """The actor of the case and, with a critic encoder, a critic of ANOTHER shape and encoder on padded rows (a swapped pointer shows)."""
    nets = [Net(rows, enc, seed=11)]
    if with_critic:
        k = CASES.index((rows, enc))
        r2, e2 = CASES[(k + 4) % len(CASES)]
        nets.append(Net(r2, e2, seed=23, pad=3))
    return nets


@pytest.mark.parametrize("with_critic", [False, True], ids=["actor", "actor+critic"])
@pytest.mark.parametrize("rows, enc", CASES, ids=[f"{r}/{e}" for r, e in CASES])
def test_rows_match_float64_as_closely_as_the_eager_composition(rows, enc, with_critic):
    _check(_pair(rows, enc, with_critic))


def test_widths_that_are_no_multiple_of_16_and_the_other_activations():
    _check([Net("277-200-77", "32-24-16-relu", seed=31)])


def _check(nets):
    import torch

    kept = {}
    for n in NS:
        got = forward(nets, n, train=True)
        again = forward(nets, n, train=True)
        infer = forward(nets, n, train=False)
        for name, net, (out, acts), (out2, acts2), (out3, _) in zip(("actor", "critic"), nets, got, again, infer):
            tag = f"lt_encoder_forward {name} n={n} rows={net.obs_dim}/{net.flat}/{net.enc_in} enc={net.hidden}->{net.emb} final={net.final}"
            assert not torch.isnan(out).any() and not any(torch.isnan(a).any() for a in acts), (tag, "an element was not written")
            # the head columns are copies; a second run and the inference form give the same bits
            assert torch.equal(out[:, :net.flat], net.obs[:n, :net.flat]), tag
            assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(acts, acts2)), tag
            assert torch.equal(out, out3), tag
            want64, hidden64, pre64 = net.ref(n)
            want32, hidden32, pre32 = net.eager(n)
            arrays = [("embedding", out[:, net.flat:], want32[:, net.flat:], want64[:, net.flat:])] + [(f"acts[{l}]", acts[l], hidden32[l], hidden64[l]) for l in range(len(hidden64))]
            if net.final is not None:
                arrays.append((f"acts[{len(hidden64)}] (pre-activation)", acts[len(hidden64)], pre32, pre64))
            assert len(acts) == len(arrays) - 1
            for what, k, e, r in arrays:
                r = r.to(DEV)
                err_k, err_e = float((k.double() - r).abs().max()), float((e.double() - r).abs().max())
                bound = max(2.0 * err_e, _ulp(float(r.abs().max())))
                print(f"\n{tag} {what}: max |err| vs f64  kernel {err_k:.3e}  eager composition {err_e:.3e}  bound {bound:.3e}")
                assert err_k <= bound, (tag, what, err_k, err_e, bound)
            kept[(name, n)] = (out, acts)
    # a row's bits depend neither on n nor on where its workgroup stands
    for name in ("actor", "critic")[:len(nets)]:
        (o17, a17), (o130, a130) = kept[(name, 17)], kept[(name, 130)]
        assert torch.equal(o130[:17], o17) and all(torch.equal(b[:17], a) for a, b in zip(a17, a130)), name
        assert torch.equal(kept[(name, 130)][0][:1], kept[(name, 1)][0]), name


@pytest.mark.parametrize("rows, enc", [("348-270-78", "256-128-64-64-tanh"), ("277-200-77", "16-8-8")], ids=str)
def test_training_form_activations_are_the_inference_forms_hidden_values(rows, enc):
    """acts[l] of the training form against the embedding of the first l + 1 layers run as an encoder of their own in the inference
    form (hidden activation behind its last layer): the same bits."""
    import torch

    from locotouch_amd import _abi

    net, n = Net(rows, enc, seed=5), 130
    (out, acts), = forward([net], n, train=True)
    for l in range(len(net.hidden)):
        sub, sub_out, _ = net.launch_net(n, False, desc=net.truncated(l + 1))
        _abi.call("lt_encoder_forward", sub, None, n, _abi.stream(torch.device(DEV)))
        torch.cuda.synchronize()
        assert torch.equal(sub_out[:, net.flat:], acts[l]), l
    if net.final is not None:  # the pre-activation embedding: the whole encoder without its final activation
        sub, sub_out, _ = net.launch_net(n, False, desc=net.truncated(len(net.linears)))
        _abi.call("lt_encoder_forward", sub, None, n, _abi.stream(torch.device(DEV)))
        torch.cuda.synchronize()
        assert torch.equal(sub_out[:, net.flat:], acts[len(net.hidden)])


def test_larger_batches_take_larger_row_blocks_and_keep_the_bits():
    """At 10 000 rows the launch takes 32-row blocks, at 20 000 rows 64-row blocks (the largest that still gives each of the chip's 256
    CUs a workgroup); every row keeps the bits of the 16-row-block launch."""
    import torch

    from locotouch_amd import _abi
    from locotouch_amd.rl import encoder

    net = Net("348-270-78", "256-128-64-64-tanh", seed=11)
    (small, _), = forward([net], 130)
    for n in (10000, 20000):  # 32-row blocks (313 of them), then 64-row blocks
        rows = net.obs[:130].repeat(154, 1)[:n].contiguous()
        out = torch.full((n, net.flat + net.emb), float("nan"), device=DEV)
        _abi.call("lt_encoder_forward", encoder.make_net(net.desc, rows, net.weights, net.biases, out), None, n, _abi.stream(torch.device(DEV)))
        torch.cuda.synchronize()
        assert torch.equal(out[:130], small) and torch.equal(out[130:260], small), n
        assert torch.equal(out[n - n % 130:], small[:n % 130]), n  # the ragged last block
