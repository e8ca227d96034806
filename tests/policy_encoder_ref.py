"""Float64 restatement of include/lt_policy_encoder.h on the CPU, in torch - one inference step of an encoder policy:

    x        = obs[r], or (obs[r] - mean) / (std + eps) over the whole row
    RNN form:   (h, c) = where(done[r], 0, (h_in[r], c_in[r]));  (h', c') = cell(x[obs_dim - tail_dim :], h, c);  e = encoder(h')
    plain form: e = encoder(x[obs_dim - tail_dim :])
    a        = actor([ x[: flat_dim] | e ])

Inputs are taken as they are stored (f32 values widened exactly); every product and sum is float64.  The cells are nn.LSTM's (gates
i, f, g, o) and nn.GRU's (r, z, n; b_hn inside r * (...)), as tests/test_hip_policy_step.py::cell64 states them; the Linear stacks as
tests/encoder_ref.py."""
import torch

from tests.encoder_ref import ACTIVATIONS


def _f64(t):
    return t.detach().cpu().double()


def cell64(cell, x, h, c, w_ih, w_hh, b_ih, b_hh):
    """(h', c' or None) of one step of a one-layer memory, everything float64."""
    if cell == "lstm":
        i, f, g, o = (x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh).chunk(4, dim=1)
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c2), c2
    (ir, iz, i_n), (hr, hz, hn) = (x @ w_ih.t() + b_ih).chunk(3, dim=1), (h @ w_hh.t() + b_hh).chunk(3, dim=1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(i_n + r * hn)
    return (1 - z) * n + z * h, None


def stack64(x, weights, biases, activation, final_activation=None):
    """A Linear stack in float64: `activation` behind every layer but the last, `final_activation` (None: none) behind the last."""
    for l, (w, b) in enumerate(zip(weights, biases)):
        x = x @ _f64(w).t() + _f64(b)
        x = ACTIVATIONS[activation if l < len(weights) - 1 else final_activation](x)
    return x


_ACT_NAMES = {torch.nn.ELU: "elu", torch.nn.ReLU: "relu", torch.nn.Tanh: "tanh"}


def _stack_of(mods):
    """(weights, biases, hidden activation, final activation or None) of a Linear / activation module list."""
    mods = list(mods)
    linears = [m for m in mods if isinstance(m, torch.nn.Linear)]
    hidden = [_ACT_NAMES[type(m)] for m in mods[:-1] if not isinstance(m, torch.nn.Linear)]
    final = None if isinstance(mods[-1], torch.nn.Linear) else _ACT_NAMES[type(mods[-1])]
    return [m.weight for m in linears], [m.bias for m in linears], (hidden[0] if hidden else "elu"), final


def operands_of(ac):
    """(encoder, actor, memory) of an ActorCriticEncoder / ActorCriticRNNEncoder module, as `policy_encoder_ref` takes them."""
    encoder = _stack_of(ac.actor_encoder.model)
    actor = _stack_of(ac.actor)[:3]
    memory = None
    if hasattr(ac, "memory_a"):
        rnn = ac.memory_a.rnn
        memory = ("lstm" if isinstance(rnn, torch.nn.LSTM) else "gru", rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)
    return encoder, actor, memory


def policy_encoder_ref(obs, flat_dim, tail_dim, encoder, actor, memory=None, state=None, done=None, norm=None):
    """One step.  `obs` [n, obs_dim] (a strided view is fine); `encoder` = (weights, biases, activation, final activation or None) and
    `actor` = (weights, biases, activation), weights in torch's [out, in] layout; `memory` = (cell, w_ih, w_hh, b_ih, b_hh) or None (the
    plain form); `state` = (h, c or None), the RAW state the step reads, and `done` [n] or None its reset mask; `norm` = (mean, std, eps)
    or None.  Returns a dict of float64 CPU tensors: actions, embedding, h, c (None without a memory / for a GRU)."""
    x = _f64(obs)
    if norm is not None:
        x = (x - _f64(norm[0]).reshape(-1)) / (_f64(norm[1]).reshape(-1) + float(norm[2]))
    tail = x[:, x.shape[1] - tail_dim:]
    h2 = c2 = None
    if memory is not None:
        cell, *params = memory
        keep = torch.ones(x.shape[0], 1, dtype=torch.float64) if done is None else (_f64(done).reshape(-1, 1) == 0).double()
        h = _f64(state[0]) * keep
        c = _f64(state[1]) * keep if cell == "lstm" else None
        h2, c2 = cell64(cell, tail, h, c, *(_f64(p) for p in params))
        tail = h2
    e = stack64(tail, *encoder)
    a = stack64(torch.cat([x[:, :flat_dim], e], dim=1), *actor)
    return dict(actions=a, embedding=e, h=h2, c=c2)
