"""The two kernel additions of include/lt_rnn_encoder.h on the GPU, each held to the entry point it generalises by `torch.equal`:

* the memory step on STRIDED rows (`lt_memory_step_strided`, `lt_memory_gru_step_strided`) equals `lt_memory_step` /
  `lt_memory_gru_step` on a contiguous copy of the rows - every output and saved array.  The contiguous kernels are held to float64 by
  tests/test_hip_memory_step.py and tests/test_hip_memory_gru_step.py; equality carries that over.
* the encoder on a second array (`lt_rnn_encoder_forward`) equals `lt_encoder_forward` on the concatenated rows [obs[:, :flat] | h]:
  lt_encoder.h promises that a sum's order depends on the layer's input width alone.

What the views do not cover is NaN in the wide buffers, so a read outside the view would show in the outputs."""
import pytest

from locotouch_amd import _abi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# N, H, I, column offset, row stride
STEP_SHAPES = [(1, 64, 78, 270, 348),    # the scalar path
               (37, 64, 78, 270, 348),   # the scalar path, 8-byte-aligned start
               (80, 128, 80, 16, 96),    # the 16-byte path
               (33, 64, 80, 18, 99),     # I % 4 == 0, but neither the start nor the stride allows the vector path
               (37, 64, 78, 0, 78)]      # x_stride == I: the old call itself


def _memory_operands(lstm, N, H, I, off, stride, seed):
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(DEV)  # noqa: E731
    G = 4 if lstm else 3
    nets = []
    for _ in range(2):
        wide = torch.full((N, stride), float("nan"), device=DEV)
        wide[:, off:off + I] = rnd(N, I)
        state = [rnd(N, H, scale=0.5) for _ in range(2 if lstm else 1)]
        nets.append(dict(wide=wide, x=wide[:, off:off + I], w_ih=rnd(G * H, I, scale=0.1), w_hh=rnd(G * H, H, scale=0.1), b_ih=rnd(G * H, scale=0.3),
                         b_hh=rnd(G * H, scale=0.3), state=state))
    dones = torch.zeros(N, dtype=torch.uint8, device=DEV)
    dones[[0, N // 2, N - 1]] = 1
    return nets, dones


def _run_step(lstm, strided, nets, dones, N, H):
    """(outputs, saved) of both networks from one launch of the strided or the contiguous entry point."""
    import torch

    ns = 2 if lstm else 1
    structs, results, keep = [], [], []
    for net in nets:
        out = [torch.full((N, H), float("nan"), device=DEV) for _ in range(ns)]
        saved = [torch.full((N, H), float("nan"), device=DEV) for _ in range(ns)]
        if strided:
            m = _abi.LtRnnEncoderMemory()
            x = net["x"]
            m.x_stride = x.stride(0)
        else:
            m = (_abi.LtMemoryNet if lstm else _abi.LtMemoryGruNet)()
            x = net["x"].contiguous()
            keep.append(x)
        assert not torch.isnan(x).any()
        m.x, m.I = x.data_ptr(), x.shape[1]
        m.w_ih, m.w_hh, m.b_ih, m.b_hh = (net[k].data_ptr() for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
        m.h_in, m.h_out, m.saved_h = net["state"][0].data_ptr(), out[0].data_ptr(), saved[0].data_ptr()
        if lstm:
            m.c_in, m.c_out, m.saved_c = net["state"][1].data_ptr(), out[1].data_ptr(), saved[1].data_ptr()
        structs.append(m)
        results.append((out, saved))
    name = ("lt_memory_step" if lstm else "lt_memory_gru_step") + ("_strided" if strided else "")
    _abi.call(name, structs[0], structs[1], dones, N, H, _abi.stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return results


@pytest.mark.parametrize("lstm", [True, False], ids=["lstm", "gru"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_strided_step_equals_the_contiguous_step(lstm, shape):
    import torch

    N, H, I, off, stride = shape
    assert off + I <= stride
    nets, dones = _memory_operands(lstm, N, H, I, off, stride, seed=100 + N + H)
    for d in ((dones, None) if shape == STEP_SHAPES[1] else (dones,)):  # dones = NULL once
        want = _run_step(lstm, False, nets, d, N, H)
        got = _run_step(lstm, True, nets, d, N, H)
        for k, ((out_w, saved_w), (out_g, saved_g)) in enumerate(zip(want, got)):
            for what, w, g in [("out", a, b) for a, b in zip(out_w, out_g)] + [("saved", a, b) for a, b in zip(saved_w, saved_g)]:
                assert not torch.isnan(w).any() and torch.equal(w, g), (k, what)
            if d is not None:  # the planted dones: the saved pre-step state of those rows is an exact zero, of the others the state itself
                rows = dones != 0
                assert torch.count_nonzero(saved_g[0][rows]) == 0
                assert torch.equal(saved_g[0][~rows], nets[k]["state"][0][~rows])
            else:
                assert torch.equal(saved_g[0], nets[k]["state"][0])


# flat, H, dims, activation, final activation, obs stride, h stride
ENC_CASES = [(270, 256, [256, 128, 64, 64], "LT_ACT_ELU", "LT_ACT_TANH", 348, 256),
             (0, 64, [16, 8], "LT_ACT_ELU", "LT_ACT_NONE", 4, 64),
             (9, 64, [16, 8], "LT_ACT_ELU", "LT_ACT_TANH", 14, 72)]


def _encoder_operands(flat, H, dims, n, obs_stride, h_stride, seed):
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(DEV)  # noqa: E731
    obs = rnd(n, obs_stride)
    hw = torch.full((n, h_stride), float("nan"), device=DEV)
    hw[:, :H] = rnd(n, H, scale=0.5)
    widths = [H] + dims
    return dict(obs=obs, h=hw[:, :H], cat=torch.cat([obs[:, :flat], hw[:, :H]], dim=1).contiguous(),
                w=[rnd(o, i, scale=i ** -0.5) for i, o in zip(widths[:-1], widths[1:])], b=[rnd(o, scale=0.2) for o in dims])


def _from_h(case, ops, out):
    flat, H, dims, act, final, obs_stride, _ = case
    net = _abi.LtRnnEncoderNet()
    net.obs_dim, net.flat_dim, net.enc_in, net.num_layers = max(flat, 1), flat, H, len(dims)
    for l, w in enumerate(dims):
        net.dims[l] = w
        net.weight[l], net.bias[l] = ops["w"][l].data_ptr(), ops["b"][l].data_ptr()
    net.activation, net.final_activation = _abi.CONSTS[act], _abi.CONSTS[final]
    net.obs, net.obs_stride, net.h, net.h_stride, net.out = ops["obs"].data_ptr(), ops["obs"].stride(0), ops["h"].data_ptr(), ops["h"].stride(0), out.data_ptr()
    return net


def _from_rows(case, ops, out):
    from locotouch_amd.rl import encoder

    flat, H, dims, act, final, *_ = case
    desc = encoder.make_desc(flat + H, flat, H, dims, _abi.CONSTS[act], _abi.CONSTS[final])
    return encoder.make_net(desc, ops["cat"], ops["w"], ops["b"], out)


@pytest.mark.parametrize("n", [1, 37, 80])
@pytest.mark.parametrize("case", ENC_CASES, ids=lambda c: f"flat{c[0]}-h{c[1]}-" + "-".join(map(str, c[2])))
def test_encoder_from_h_equals_the_encoder_on_concatenated_rows(case, n):
    import torch

    flat, H, dims, _, _, obs_stride, h_stride = case
    a = _encoder_operands(flat, H, dims, n, obs_stride, h_stride, seed=7 + n)
    c = _encoder_operands(flat, H, dims, n, obs_stride, h_stride, seed=70 + n)
    width = flat + dims[-1]
    stream = _abi.stream(torch.device(DEV))
    for nets in ((a,), (a, c)):  # the actor alone, and actor + critic in one launch
        want = [torch.full((n, width), float("nan"), device=DEV) for _ in nets]
        got = [torch.full((n, width), float("nan"), device=DEV) for _ in nets]
        rows = [_from_rows(case, ops, out) for ops, out in zip(nets, want)]
        hs = [_from_h(case, ops, out) for ops, out in zip(nets, got)]
        _abi.call("lt_encoder_forward", rows[0], rows[1] if len(nets) == 2 else None, n, stream)
        _abi.call("lt_rnn_encoder_forward", hs[0], hs[1] if len(nets) == 2 else None, n, stream)
        torch.cuda.synchronize()
        for k, (w, g, ops) in enumerate(zip(want, got, nets)):
            assert not torch.isnan(w).any() and torch.equal(w, g), k
            assert torch.equal(g[:, :flat], ops["obs"][:, :flat])  # the head columns are copies
    assert _abi.load().lt_rnn_encoder_forward_launches(hs[0], hs[1]) == 1
