"""The backward pass of include/lt_rnn_encoder_train.h, section b, stated in float64 torch ops: from the gradient g w.r.t. an encoder's
embedding to every layer's dz_l and to dh, the gradient w.r.t. the rows the encoder read - with every derivative taken from the STORED
OUTPUT of its activation, as the kernel takes it (the final ELU and RELU from the pre-activation embedding, the final TANH from the
embedding itself).  `forward` is the record that pass reads.  `MUTATIONS` are the planted errors
tests/test_direct_rnn_encoder_update_cpu.py rejects.  Nothing here needs a GPU or the library."""
import torch

ACTS = ("elu", "relu", "tanh")
FINALS = (None, "tanh", "elu", "relu")

MUTATIONS = ("elu_derivative_of_relu", "relu_derivative_of_tanh", "tanh_derivative_of_elu", "final_elu_from_emb_where_pre_belongs",
             "final_tanh_from_pre_where_emb_belongs", "weight_transposed", "a_layer_dropped", "final_activation_skipped", "dh_from_dz1",
             "hidden_derivative_skipped")


def _apply(kind, x):
    if kind == "elu":
        return torch.where(x > 0, x, torch.expm1(x))
    if kind == "relu":
        return torch.clamp_min(x, 0)
    if kind == "tanh":
        return torch.tanh(x)
    assert kind is None
    return x


def forward(weights, biases, h, act, final):
    """(acts, pre, emb): the outputs of the hidden activations, the pre-activation embedding and the embedding, in h's dtype."""
    x, acts = h, []
    for w, b in zip(weights[:-1], biases[:-1]):
        x = _apply(act, x @ w.t() + b)
        acts.append(x)
    pre = x @ weights[-1].t() + biases[-1]
    return acts, pre, _apply(final, pre)


def hidden_grad(kind, a):
    """act'(.) from the activation's OUTPUT a."""
    if kind == "elu":
        return torch.where(a > 0, torch.ones_like(a), a + 1)
    if kind == "relu":
        return (a > 0).to(a.dtype)
    assert kind == "tanh"
    return 1 - a * a


def final_grad(kind, pre, emb):
    """f'(pre) of the final activation (emb = f(pre)), as `PPO._final_activation_grad` states it."""
    if kind is None:
        return torch.ones_like(pre)
    if kind == "tanh":
        return 1 - emb * emb
    if kind == "elu":
        return torch.where(pre > 0, torch.ones_like(pre), torch.exp(pre))
    assert kind == "relu"
    return (pre > 0).to(pre.dtype)


def backward(weights, acts, pre, emb, g, act, final, mutate=None):
    """([dz_0 .. dz_{L-1}], dh) from g = d loss / d embedding.  weights[l]: [dims[l], dims[l - 1]]; acts: the L - 1 hidden outputs.
    Everything is computed in g's dtype (float64 for the reference; the comparator's stand-in for a kernel runs it in float32)."""
    L = len(weights)
    assert len(acts) == L - 1 and mutate in (None, *MUTATIONS)
    if mutate == "hidden_derivative_skipped":
        hid = lambda a: torch.ones_like(a)  # noqa: E731
    else:
        kind = {"elu_derivative_of_relu": {"relu": "elu"}, "relu_derivative_of_tanh": {"tanh": "relu"},
                "tanh_derivative_of_elu": {"elu": "tanh"}}.get(mutate, {}).get(act, act)
        hid = lambda a: hidden_grad(kind, a)  # noqa: E731
    if mutate == "final_activation_skipped":
        dz = g.clone()
    elif mutate == "final_elu_from_emb_where_pre_belongs":
        dz = g * final_grad(final, emb, emb)
    elif mutate == "final_tanh_from_pre_where_emb_belongs":
        dz = g * final_grad(final, pre, pre)
    else:
        dz = g * final_grad(final, pre, emb)
    dzs = [None] * L
    dzs[L - 1] = dz
    for l in range(L - 1, 0, -1):
        w = weights[l]
        if mutate == "a_layer_dropped" and l == L - 1 and w.shape[0] == w.shape[1]:
            da = dz  # (the layer's product left out: only a square layer lets the shapes pass)
        elif mutate == "weight_transposed" and w.shape[0] == w.shape[1]:
            da = dz @ w.t()
        else:
            da = dz @ w
        dz = da * hid(acts[l - 1])
        dzs[l - 1] = dz
    dh = (dzs[1] if mutate == "dh_from_dz1" and L > 1 and weights[0].shape[0] == weights[1].shape[0] else dzs[0]) @ weights[0]
    return dzs, dh


def case(enc_in, dims, act, final, n, seed=0, dtype=torch.float64):
    """A seeded encoder and batch: weights of order 1 / sqrt(fan-in) scaled so that pre-activations reach both branches of every
    activation, g of order 1.  -> dict(weights, biases, h, g)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    widths = [enc_in, *dims]
    ws = [(1.5 * torch.randn(o, k, generator=gen, dtype=torch.float64) / k ** 0.5).to(dtype) for k, o in zip(widths[:-1], widths[1:])]
    bs = [(0.3 * torch.randn(o, generator=gen, dtype=torch.float64)).to(dtype) for o in widths[1:]]
    h = torch.randn(n, enc_in, generator=gen, dtype=torch.float64).to(dtype)
    g = torch.randn(n, dims[-1], generator=gen, dtype=torch.float64).to(dtype)
    return dict(weights=ws, biases=bs, h=h, g=g, act=act, final=final)
