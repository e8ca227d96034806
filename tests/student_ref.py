"""Float64 numpy restatement of ONE env step of the student (helper of the student-step tests), written from
locotouch_amd/rl/models.py and distill/student.py: CNN2dHead (conv / ReLU / max-pool, Linear head) -> GRU cell (PyTorch's gate order
r, z, n; b_hn inside the r product) -> ELU MLP -> concatenation with the proprioception -> ELU MLP; the done-mask reset zeroes a
row's hidden state BEFORE the step."""
import numpy as np
import torch.nn as nn


def params_of(student):
    """The student's parameters as float64 numpy arrays, by role."""
    f = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
    pre, enc, bb = student.pre_encoder, student.student_encoder, student.student_backbone
    seq, convs, pool = list(pre.conv.conv), [], {}
    for m in seq:
        if isinstance(m, nn.Conv2d):
            convs.append((f(m.weight), f(m.bias), m.stride[0]))
        elif isinstance(m, nn.MaxPool2d):
            pool[len(convs) - 1] = m.kernel_size if isinstance(m.kernel_size, int) else m.kernel_size[0]
    lin = lambda mlp: [(f(m.weight), f(m.bias)) for m in mlp.model if isinstance(m, nn.Linear)]  # noqa: E731
    r = enc.memory.rnn
    return dict(img=tuple(student.tactile_signal_img_shape), convs=convs, pool=pool, head=lin(pre.head),
                gru=(f(r.weight_ih_l0), f(r.weight_hh_l0), f(r.bias_ih_l0), f(r.bias_hh_l0)), enc=lin(enc.mlp), bb=lin(bb))


def conv2d(x, w, b, stride):
    n, c, h, wd = x.shape
    co, _, k, _ = w.shape
    ho, wo = (h - k) // stride + 1, (wd - k) // stride + 1
    cols = np.empty((n, c, k, k, ho, wo))
    for ky in range(k):
        for kx in range(k):
            cols[:, :, ky, kx] = x[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
    return np.einsum("nckyhw,ocky->nohw", cols, w) + b[None, :, None, None]


def maxpool(x, p):
    n, c, h, w = x.shape
    ho, wo = h // p, w // p
    return x[:, :, :ho * p, :wo * p].reshape(n, c, ho, p, wo, p).max(axis=(3, 5))


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def mlp(x, layers):
    for i, (w, b) in enumerate(layers):
        x = x @ w.T + b
        if i < len(layers) - 1:
            x = elu(x)
    return x


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def step(P, proprio, tactile, h, done=None):
    """(actions, new hidden state) of one step; `h` [n][H] float64, `done` [n] (non-zero: the row starts from zeros)."""
    proprio, tactile, h = np.asarray(proprio, np.float64), np.asarray(tactile, np.float64), np.asarray(h, np.float64)
    if done is not None:
        h = h * (np.asarray(done).reshape(-1) == 0)[:, None]
    x = tactile.reshape(tactile.shape[0], *P["img"])
    for i, (w, b, s) in enumerate(P["convs"]):
        x = np.maximum(conv2d(x, w, b, s), 0.0)
        if i in P["pool"]:
            x = maxpool(x, P["pool"][i])
    x = mlp(x.reshape(x.shape[0], -1), P["head"])
    w_ih, w_hh, b_ih, b_hh = P["gru"]
    H = w_hh.shape[1]
    gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    r = sigmoid(gi[:, :H] + gh[:, :H])
    z = sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    h_new = (1.0 - z) * n + z * h
    emb = mlp(h_new, P["enc"])
    return mlp(np.concatenate([proprio, emb], axis=1), P["bb"]), h_new
