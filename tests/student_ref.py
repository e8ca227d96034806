"""Float64 numpy restatement of ONE env step of the student (helper of the student-step tests), written from
locotouch_amd/rl/models.py and distill/student.py: CNN2dHead (conv / ReLU / max-pool, Linear head) -> GRU cell (PyTorch's gate order
r, z, n; b_hn inside the r product) -> ELU MLP -> concatenation with the proprioception -> ELU MLP; the done-mask reset SELECTS a
zero hidden state for a row BEFORE the step (whatever the row held, a NaN included, never reaches the arithmetic).

Beside it: the descriptor family of include/lt_student.h as plain numbers (`CASES`), random parameters and inputs for a case, the
descriptor and the packed layout of a case, a torch composition of the same step (`compose`, the f32 yardstick of the GPU tests) and
named single-line mutations of the restatement (`faults`), with which tests/test_student_ref.py shows that the inputs of a case have
the power to expose a kernel that is wrong in that way."""
import math

import numpy as np
import torch.nn as nn

# The family lt_student_validate admits, at its edges.  img: C x H x W; convs: (channels, kernel, CONFIGURED stride) - with `pool` the
# conv runs at stride 1 and a max-pool of that size follows; D: head_out; enc / bb: the MLPs' widths, input first.
CASES = {
    # D below one k group of the GRU launch, one GRU workgroup per row tile, one-layer encoder and backbone, odd P, kpad 16, one unit tile
    "tiny": dict(img=(1, 9, 8), convs=[(5, 3, 1)], pool=False, D=16, H=64, enc=(64, 13), P=3, bb=(16, 12)),
    # D = 3 k blocks, two GRU workgroups, P = 0 (proprio NULL), the pool's floor drops a row and a column, widths 100, 17, 33, one action
    "odd": dict(img=(2, 11, 9), convs=[(5, 3, 2), (7, 2, 1)], pool=True, D=48, H=128, enc=(128, 100, 17), P=0, bb=(17, 33, 1)),
    # D = one k group + one block, six layers each, 17 unit tiles (wave 0 goes round twice), kpad 144, widths 9, 5, 3
    "str": dict(img=(2, 12, 11), convs=[(5, 3, 2), (6, 2, 2)], pool=False, D=80, H=64, enc=(64, 272, 144, 24, 40, 9, 5), P=270,
                bb=(275, 17, 512, 16, 100, 3, 12)),
    # encoder LDS above 64 KB (8 x (1600 + 1444) floats), cat_pad 528 above every layer width, flat 1444
    "wide": dict(img=(1, 40, 40), convs=[(4, 3, 2)], pool=False, D=16, H=512, enc=(512, 13), P=499, bb=(512, 512, 7)),
    # the registered student
    "reg": dict(img=(2, 17, 13), convs=[(24, 4, 2), (24, 3, 1), (24, 2, 1)], pool=True, D=64, H=512, enc=(512, 256, 128, 64, 64), P=270,
                bb=(334, 512, 256, 128, 12)),
}
NS = (1, 9, 17, 130)  # one row; two conv tiles inside one row tile; a ragged second row tile; nine row tiles, ragged
# The seed of a case's parameters and inputs: FIXED by test_student_ref.py::test_inputs_have_the_power_to_show_every_fault, which
# requires every fault of faults() to move an output by 1000 f32 errors at this seed.  At seed 1 the last position of the
# last conv channel of tiny, wide and reg is zero behind the ReLU for every row, so a dropped last head column would not show; reg
# fails the condition at seeds 2 and 4 too.
SEEDS = {"tiny": 2, "odd": 1, "str": 1, "wide": 2, "reg": 3}
FACTOR = 2.0  # the house rule: kernel error <= max(FACTOR x the f32 composition's, one f32 ulp of the array's magnitude)


def pad16(v):
    return (v + 15) // 16 * 16


def pad4(v):
    return (v + 3) // 4 * 4


def ulp32(x):
    """One f32 ulp at magnitude x."""
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


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


def geometry(case):
    """[(C, H, W)] of the input and of every conv's output (after its pool)."""
    maps = [tuple(case["img"])]
    for ch, k, s in case["convs"]:
        _, h, w = maps[-1]
        cs, pool = (1, s) if case["pool"] else (s, 1)
        maps.append((ch, ((h - k) // cs + 1) // pool, ((w - k) // cs + 1) // pool))
    return maps


def random_params(case, seed):
    """Float64 arrays in torch's layouts (the dict of `params_of`) for a case: weights normal with deviation 2 / sqrt(fan_in), biases
    uniform in +-0.3 (the convention of tests/test_hip_memory_step.py), every value rounded to float32 so that the kernel, the f32
    composition and the float64 restatement see the same numbers."""
    rng = np.random.RandomState(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    w = lambda *s, fan: f32(rng.standard_normal(s) * (2.0 / math.sqrt(fan)))  # noqa: E731
    b = lambda n: f32(rng.uniform(-0.3, 0.3, n))  # noqa: E731
    maps = geometry(case)
    convs, pool = [], {}
    for i, (ch, k, s) in enumerate(case["convs"]):
        cin = maps[i][0]
        convs.append((w(ch, cin, k, k, fan=cin * k * k), b(ch), 1 if case["pool"] else s))
        if case["pool"] and s > 1:
            pool[i] = s
    flat, D, H = int(np.prod(maps[-1])), case["D"], case["H"]
    lin = lambda dims: [(w(o, i, fan=i), b(o)) for i, o in zip(dims[:-1], dims[1:])]  # noqa: E731
    return dict(img=tuple(case["img"]), convs=convs, pool=pool, head=[(w(D, flat, fan=flat), b(D))],
                gru=(w(3 * H, D, fan=D), w(3 * H, H, fan=H), b(3 * H), b(3 * H)), enc=lin(case["enc"]), bb=lin(case["bb"]))


def random_inputs(case, n, seed):
    """(proprio [n][P], tactile [n][img], h [n][H]) float64 holding float32 values; row r depends on (seed, r) only through the
    generator's order, so the first rows of a larger draw are NOT those of a smaller one: slice the largest."""
    rng = np.random.RandomState(1000 + seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    return (f32(rng.standard_normal((n, case["P"]))), f32(rng.uniform(0.0, 1.0, (n, int(np.prod(case["img"]))))),
            f32(0.5 * np.tanh(rng.standard_normal((n, case["H"])))))


def mixed_mask(n, seed):
    """uint8 [n]: about 40 % done, row 0 done and the last row not (n > 1)."""
    m = (np.random.RandomState(2000 + seed).uniform(size=n) < 0.4).astype(np.uint8)
    if n > 1:
        m[0], m[-1] = 1, 0
    return m


def desc_of(case):
    """The LtStudentDesc of a case."""
    from locotouch_amd import _abi

    C = _abi.CONSTS
    d = _abi.LtStudentDesc()
    d.img_channels, d.img_height, d.img_width = case["img"]
    d.num_convs, d.use_maxpool = len(case["convs"]), int(case["pool"])
    for i, (c, k, s) in enumerate(case["convs"]):
        d.conv_channels[i], d.conv_kernel[i], d.conv_stride[i], d.conv_padding[i] = c, k, s, 0
    d.conv_activation, d.conv_norm, d.head_out = C["LT_ACT_RELU"], 0, case["D"]
    d.rnn_type, d.rnn_layers, d.rnn_hidden, d.proprio_dim = _abi.LT_STUDENT_RNN_GRU, 1, case["H"], case["P"]
    for m, dims in ((d.encoder, case["enc"]), (d.backbone, case["bb"])):
        m.num_layers, m.activation, m.input_format = len(dims) - 1, C["LT_ACT_ELU"], C["LT_ROWS_F32"]
        for i, v in enumerate(dims):
            m.dims[i] = v
    return d


def cat_pad(case):
    return pad16(case["P"] + pad16(case["enc"][-1]))


def packed_blocks(case):
    """[(name, offset, rows, row length)] of the packed buffer in its documented order: per conv the transposed weight
    [Cin K K][Cout] and the bias; the transposed head [flat][D] and its bias; [W_ih | W_hh] as [3H][D + H], b_ih, b_hh; per MLP layer
    the weight zero-padded to [pad16(out)][pad16(in)] (backbone layer 0: [pad16(out)][cat_pad]) and the bias [pad16(out)].  Every
    block starts on a multiple of 4 floats.  -> (blocks, total floats)"""
    maps, blocks, off = geometry(case), [], 0

    def take(name, rows, cols):
        nonlocal off
        blocks.append((name, off, rows, cols))
        off += pad4(rows * cols)

    for i, (ch, k, _) in enumerate(case["convs"]):
        take(f"conv_w{i}", maps[i][0] * k * k, ch)
        take(f"conv_b{i}", 1, ch)
    D, H = case["D"], case["H"]
    take("head_w", int(np.prod(maps[-1])), D)
    take("head_b", 1, D)
    take("gru_w", 3 * H, D + H)
    take("gru_bi", 1, 3 * H)
    take("gru_bh", 1, 3 * H)
    for tag, dims in (("enc", case["enc"]), ("bb", case["bb"])):
        for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
            take(f"{tag}_w{l}", pad16(b), cat_pad(case) if (tag, l) == ("bb", 0) else pad16(a))
            take(f"{tag}_b{l}", 1, pad16(b))
    return blocks, off


def pack(case, P):
    """(the packed buffer as float32 [total], bool [total]: the floats the layout defines - the gaps that round a block up to 4 floats
    are nobody's) for the parameters P, by the layout of `packed_blocks`."""
    blocks, total = packed_blocks(case)
    out, known = np.zeros(total, np.float32), np.zeros(total, bool)
    src = {}
    for i, (w, b, _) in enumerate(P["convs"]):
        src[f"conv_w{i}"], src[f"conv_b{i}"] = w.reshape(w.shape[0], -1).T, b[None]
    src["head_w"], src["head_b"] = P["head"][0][0].T, P["head"][0][1][None]
    w_ih, w_hh, b_ih, b_hh = P["gru"]
    src["gru_w"], src["gru_bi"], src["gru_bh"] = np.concatenate([w_ih, w_hh], axis=1), b_ih[None], b_hh[None]
    for tag in ("enc", "bb"):
        for l, (w, b) in enumerate(P[tag]):
            src[f"{tag}_w{l}"], src[f"{tag}_b{l}"] = w, b[None]
    for name, off, rows, cols in blocks:
        block = np.zeros((rows, cols), np.float32)
        s = src[name]
        block[:s.shape[0], :s.shape[1]] = s
        out[off:off + rows * cols], known[off:off + rows * cols] = block.reshape(-1), True
    return out, known


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


def stages(P, proprio, tactile, h, done=None):
    """Every intermediate of one step in float64: dict(maps=[each conv map after ReLU and pool], head, r, z, n, h_new, emb, actions).
    `h` [n][H]; `done` [n] or None (non-zero: the row starts from zeros, selected - not multiplied).  P["fault"], if present, names
    the one line of `faults()` that is computed wrongly."""
    fault = P.get("fault")
    proprio, tactile, h = np.asarray(proprio, np.float64), np.asarray(tactile, np.float64), np.asarray(h, np.float64)
    n = tactile.shape[0]
    if done is not None and fault != "done mask ignored":
        h = np.where((np.asarray(done).reshape(-1) != 0)[:, None], 0.0, h)
    x, maps = tactile.reshape(n, *P["img"]), []
    for i, (w, b, s) in enumerate(P["convs"]):
        x = np.maximum(conv2d(x, w, b, s), 0.0)
        if i in P["pool"]:
            p = P["pool"][i]
            if fault == "pool takes the row the floor drops" and x.shape[2] % p:
                x = np.concatenate([x[:, :, :x.shape[2] // p * p - p], np.repeat(x[:, :, -(p + 1):].max(axis=2, keepdims=True), p, axis=2)], axis=2)
            x = maxpool(x, p)
        maps.append(x)
    head = mlp(x.reshape(n, -1), P["head"])
    w_ih, w_hh, b_ih, b_hh = P["gru"]
    H = w_hh.shape[1]
    gi, gh = head @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    r = sigmoid(gi[:, :H] + gh[:, :H])
    z = sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    if fault == "r and z gates swapped":
        r, z = z, r
    if fault == "b_hn outside the r product":
        g = np.tanh(gi[:, 2 * H:] + r * (gh[:, 2 * H:] - b_hh[2 * H:]) + b_hh[2 * H:])
    else:
        g = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    h_new = (1.0 - z) * g + z * h
    emb = mlp(h_new, P["enc"])
    cat = np.concatenate([proprio.reshape(n, -1), emb], axis=1)
    if fault == "embedding read at column pad16(P)":
        pd = pad16(proprio.shape[1]) - proprio.shape[1]
        cat = np.concatenate([proprio.reshape(n, -1), np.zeros((n, pd)), emb], axis=1)[:, :cat.shape[1]]
    return dict(maps=maps, head=head, r=r, z=z, n=g, h_new=h_new, emb=emb, actions=mlp(cat, P["bb"]))


def step(P, proprio, tactile, h, done=None):
    """(actions, new hidden state) of one step; `h` [n][H] float64, `done` [n] (non-zero: the row starts from zeros)."""
    s = stages(P, proprio, tactile, h, done)
    return s["actions"], s["h_new"]


def _zeroed(a, idx):
    a = a.copy()
    a[idx] = 0.0
    return a


def _layer(P, key, l, w_idx=None, b_idx=None):
    """P with elements of layer l of the MLP `key` (or of P["convs"]) zeroed."""
    layers = list(P[key])
    w, b, *rest = layers[l]
    layers[l] = (w if w_idx is None else _zeroed(w, w_idx), b if b_idx is None else _zeroed(b, b_idx), *rest)
    return {**P, key: layers}


def faults():
    """[(name, applies(P), mutate(P) -> P')]: single-line mutations of the REFERENCE, each what a kernel with one wrong index, a
    short loop or a wrong operand order would compute.  `applies` is False where the case cannot tell the fault from the truth by
    construction (a proprio_dim that is a multiple of 16, a pool whose floor drops nothing)."""
    last_col = (slice(None), -1)
    always = lambda P: True  # noqa: E731
    flag = lambda name: (lambda P: {**P, "fault": name})  # noqa: E731
    gru = lambda P, i, idx: {**P, "gru": tuple(_zeroed(a, idx) if k == i else a for k, a in enumerate(P["gru"]))}  # noqa: E731
    return [
        ("last k element of the head dropped", always, lambda P: _layer(P, "head", 0, w_idx=last_col)),
        ("last k element of encoder layer 0 dropped", always, lambda P: _layer(P, "enc", 0, w_idx=last_col)),
        ("last k element of the encoder's last layer dropped", always, lambda P: _layer(P, "enc", -1, w_idx=last_col)),
        ("last embedding column of backbone layer 0 dropped", always, lambda P: _layer(P, "bb", 0, w_idx=last_col)),
        ("last k element of the backbone's last layer dropped", always, lambda P: _layer(P, "bb", -1, w_idx=last_col)),
        ("last tap of the last conv's last channel dropped", always, lambda P: _layer(P, "convs", -1, w_idx=(-1, -1, -1, -1))),
        ("last column of W_hh dropped", always, lambda P: gru(P, 1, last_col)),
        ("r and z gates swapped", always, flag("r and z gates swapped")),
        ("b_hn outside the r product", always, flag("b_hn outside the r product")),
        ("last action's bias dropped", always, lambda P: _layer(P, "bb", -1, b_idx=-1)),
        ("embedding read at column pad16(P)", lambda P: (P["bb"][0][0].shape[1] - P["enc"][-1][0].shape[0]) % 16 != 0,
         flag("embedding read at column pad16(P)")),
        ("done mask ignored", always, flag("done mask ignored")),
        ("pool takes the row the floor drops", _pool_drops_a_row, flag("pool takes the row the floor drops")),
    ]


def _pool_drops_a_row(P):
    h = P["img"][1]
    for i, (w, _, s) in enumerate(P["convs"]):
        h = (h - w.shape[2]) // s + 1
        if i in P["pool"]:
            if h % P["pool"][i]:
                return True
            h //= P["pool"][i]
    return False


# ---- the same step from torch ops, in the dtype and on the device of its tensors ------------------------------------------------------
def to_torch(P, device, dtype):
    """P's arrays as tensors (strides and pool sizes stay numbers)."""
    import torch

    t = lambda a: torch.as_tensor(a, dtype=dtype, device=device).contiguous()  # noqa: E731
    pair = lambda layers: [(t(w), t(b)) for w, b in layers]  # noqa: E731
    return dict(img=P["img"], convs=[(t(w), t(b), s) for w, b, s in P["convs"]], pool=P["pool"], head=pair(P["head"]),
                gru=tuple(t(a) for a in P["gru"]), enc=pair(P["enc"]), bb=pair(P["bb"]))


def compose(T, proprio, tactile, h, done=None):
    """(actions, h_new) of one step from plain torch ops on the tensors of `to_torch`: convolutions as unfold + matmul (no
    convolution library and no solver search per shape), the pool as a reshape and two maxima, the GRU as two `F.linear` and the gate
    arithmetic, the MLPs as `F.linear` + `F.elu`.  The yardstick of the house rule: what a plain composition in this dtype gives."""
    import torch
    import torch.nn.functional as F

    n = tactile.shape[0]
    if done is not None:
        h = torch.where((done.reshape(-1) != 0)[:, None], torch.zeros_like(h), h)
    x = tactile.reshape(n, *T["img"])
    for i, (w, b, s) in enumerate(T["convs"]):
        co, _, k, _ = w.shape
        ho, wo = (x.shape[2] - k) // s + 1, (x.shape[3] - k) // s + 1
        x = torch.relu(torch.matmul(w.reshape(co, -1), F.unfold(x, k, stride=s)) + b[None, :, None]).reshape(n, co, ho, wo)
        if i in T["pool"]:
            p = T["pool"][i]
            x = x[:, :, :ho // p * p, :wo // p * p].reshape(n, co, ho // p, p, wo // p, p).amax(dim=(3, 5))
    x = F.linear(x.reshape(n, -1), *T["head"][0])
    w_ih, w_hh, b_ih, b_hh = T["gru"]
    H = w_hh.shape[1]
    gi, gh = F.linear(x, w_ih, b_ih), F.linear(h, w_hh, b_hh)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    g = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    h_new = (1.0 - z) * g + z * h
    x = h_new
    for tag, layers in (("enc", T["enc"]), ("bb", T["bb"])):
        if tag == "bb":
            x = torch.cat([proprio.reshape(n, -1), x], dim=1)
        for l, (w, b) in enumerate(layers):
            x = F.linear(x, w, b)
            if l < len(layers) - 1:
                x = F.elu(x)
    return x, h_new
