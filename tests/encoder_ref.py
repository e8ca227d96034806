"""Float64 restatement of include/lt_encoder.h on the CPU, in torch:

    e      = enc(obs[r, obs_dim - enc_in : obs_dim])     Linear stack, one activation between layers, optional final activation
    out[r] = [ obs[r, 0 : flat_dim] | e ]

Inputs are taken as they are stored (f32 values widened exactly); every product and sum is float64."""
import torch

ACTIVATIONS = {"elu": torch.nn.functional.elu, "relu": torch.relu, "tanh": torch.tanh, None: lambda x: x}


def encoder_ref(obs, flat_dim, enc_in, weights, biases, activation, final_activation=None):
    """(out [n, flat_dim + E], hidden: the activation behind every hidden layer, pre: the embedding in front of the final activation),
    all float64 on the CPU.  `obs` [n, obs_dim] (a strided view is fine); `weights[l]` in torch's [out, in] layout."""
    obs = obs.detach().cpu().double()
    x = obs[:, obs.shape[1] - enc_in:]
    hidden = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        x = x @ w.detach().cpu().double().t() + b.detach().cpu().double()
        if l < len(weights) - 1:
            x = ACTIVATIONS[activation](x)
            hidden.append(x)
    pre = x
    e = ACTIVATIONS[final_activation](pre)
    return torch.cat([obs[:, :flat_dim], e], dim=1), hidden, pre
