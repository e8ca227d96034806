"""The two LSTM memories of a recurrent policy over a WHOLE ROLLOUT of an env block: what `PPO._recurrent_update` runs per optimizer step
instead of padded trajectories (`split_and_pad_trajectories` -> two `lstm_sequence` -> two `unpad_trajectories`).

Why this equals the padded form: `PolicyMemory.reset(dones)` zeroes the state of done envs, so the hidden state saved at the first step
of a trajectory that starts after a done is all zeros.  The padded batch of trajectories that starts from the saved states therefore
equals, row for row, ONE pass over the block's envs for all T steps that starts from `saved_hidden_states[0][:, e0:e1]` and replaces the
carried (h, c) by zeros wherever `dones[t - 1]` is set.  No gradient crosses a done in either form (the padded tail has dout = 0, the
reset state is a constant), and the output [T, E, H] is already in the row order `unpad_trajectories` produces
(tests/test_recurrent_update_form.py).

`memory_rollout_sequence` is one `torch.autograd.Function` over both memories' `nn.LSTM` parameters (the modules' own: checkpoints are
unaffected), in two forms as rl/lstm.py:
  * a PyTorch-op time loop with `where(dones[t - 1], 0, .)` on the carry: the CPU, any dtype, shapes the kernels do not cover;
  * csrc/lt_memory.hip (the LSTM cell on the kernels of csrc/lt_memory_tile.h; include/lt_memory_seq.h): `lt_memory_seq_forward`
    (T launches, both networks in each, the observation rows read in place) and `lt_memory_seq_backward` (T launches).  What is not sequential stays outside the loop, one call each:
    dW_hh = dgates^T h_prev and dW_ih = dgates^T X through rl/gru.py `_wgrad`, the bias gradients as column sums.
The observations and the initial states carry no gradient: dX, dh0 and dc0 are not computed.

GRU memories (`gru_memories=True`, the opt-in `fused_gru_memories` of rl/ppo.py) have the same two forms: the op loop `_gru_forward_ops`
/ `_gru_backward_ops` and csrc/lt_memory_gru.hip (the GRU cell on the same kernels; include/lt_memory_gru.h).  The state is one tensor, the forward record is (out, gates
= r | z | n | hn, h_prev), and the backward pass leaves TWO gate-gradient arrays, dig = (dr, dz, dn) and dhg = (dr, dz, dn * r): dW_ih =
dig^T X and db_ih come from the first, dW_hh = dhg^T h_prev and db_hh from the second, each as the kernel wrote it.
"""
from __future__ import annotations

import torch

from .gru import _wgrad

MIN_HIDDEN, MAX_HIDDEN, MAX_K = 64, 512, 1248  # include/lt_memory_seq.h


def _params(memory):
    rnn = memory.rnn
    return rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0


def _state(hc0, E):
    """(h0, c0) as [E, H] from `saved_hidden_states[i][0][:, e0:e1]`-shaped ([1, E, H]) or [E, H] tensors."""
    h0, c0 = hc0
    return h0.reshape(E, -1), c0.reshape(E, -1)


def _dones2d(dones, T, E):
    if dones is None:
        return None
    d = dones[..., 0] if dones.dim() == 3 else dones
    assert d.shape == (T, E), "dones must be [T, E] (or [T, E, 1])"
    return d


def _dones_bytes(d):
    """dones [T, E] as the kernels read them: uint8, E contiguous bytes per step, any stride between steps."""
    if d is not None:
        d = d if d.dtype == torch.uint8 else (d != 0).to(torch.uint8)
        d = d if d.stride(1) == 1 else d.contiguous()
    return d


# ---- the PyTorch-op form --------------------------------------------------------------------------------------------------------------
def _forward_ops(x, done_rows, h0, c0, w_ih, w_hh, b_ih, b_hh):
    """One network.  done_rows: bool [T, E, 1] or None.  Returns the forward record (out, cell, gates, h_prev, c_prev)."""
    T, E, _ = x.shape
    H = w_hh.shape[1]
    ig = (x.reshape(T * E, -1) @ w_ih.t()).view(T, E, 4 * H)
    w_hh_t = w_hh.t().contiguous()
    bias = b_ih + b_hh
    out, cell, h_prev, c_prev = (x.new_empty(T, E, H) for _ in range(4))
    gates = x.new_empty(T, E, 4 * H)
    h, c = h0, c0
    for t in range(T):
        if t > 0 and done_rows is not None:
            h = torch.where(done_rows[t - 1], torch.zeros_like(h), h)
            c = torch.where(done_rows[t - 1], torch.zeros_like(c), c)
        h_prev[t], c_prev[t] = h, c
        a = torch.addmm(ig[t] + bias, h, w_hh_t)
        torch.sigmoid(a[:, :2 * H], out=gates[t, :, :2 * H])
        torch.tanh(a[:, 2 * H:3 * H], out=gates[t, :, 2 * H:3 * H])
        torch.sigmoid(a[:, 3 * H:], out=gates[t, :, 3 * H:])
        i, f, g, o = gates[t].split(H, dim=1)
        c = f * c + i * g
        h = o * torch.tanh(c)
        out[t], cell[t] = h, c
    return out, cell, gates, h_prev, c_prev


def _backward_ops(dout, done_rows, w_hh, cell, gates, c_prev):
    """dgates [T, E, 4H] of one network from the forward record."""
    T, E, H = cell.shape
    dgates = cell.new_empty(T, E, 4 * H)
    dh_next = dc_next = None  # what step t + 1 hands to step t: dgates[t+1] W_hh and dc_{t+1} f_{t+1}
    for t in range(T - 1, -1, -1):
        dh = dout[t]
        dc = None
        if dh_next is not None:
            if done_rows is not None:
                dh_next = torch.where(done_rows[t], torch.zeros_like(dh_next), dh_next)
                dc_next = torch.where(done_rows[t], torch.zeros_like(dc_next), dc_next)
            dh, dc = dh + dh_next, dc_next
        i, f, g, o = gates[t].split(H, dim=1)
        tc = torch.tanh(cell[t])
        dc = dh * o * (1 - tc * tc) if dc is None else dc + dh * o * (1 - tc * tc)
        dgates[t] = torch.cat([dc * g * i * (1 - i), dc * c_prev[t] * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], dim=1)
        dh_next, dc_next = dgates[t] @ w_hh, dc * f
    return dgates


def _finish(x, dgates, h_prev):
    """(dW_ih, dW_hh, db_ih, db_hh) of one network: everything of the backward pass that is not sequential, one call each."""
    T, E, H = h_prev.shape
    dg2 = dgates.view(T * E, 4 * H)
    db = dg2.sum(0)
    return _wgrad(dg2, x.reshape(T * E, -1)), _wgrad(dg2, h_prev.view(T * E, H)), db, db.clone()


class _MemorySeq(torch.autograd.Function):
    """Both memories, time loop in PyTorch ops."""

    @staticmethod
    def forward(ctx, x_a, x_c, dones, h0_a, c0_a, h0_c, c0_c, *params):
        done_rows = None if dones is None else (dones != 0).unsqueeze(-1)
        ra = _forward_ops(x_a, done_rows, h0_a, c0_a, *params[:4])
        rc = _forward_ops(x_c, done_rows, h0_c, c0_c, *params[4:])
        ctx.save_for_backward(x_a, x_c, done_rows, params[1], params[5], *ra[1:], *rc[1:])
        ctx.set_materialize_grads(False)
        return ra[0], rc[0]

    @staticmethod
    def backward(ctx, dout_a, dout_c):
        x_a, x_c, done_rows, w_hh_a, w_hh_c, *rec = ctx.saved_tensors
        grads = []
        for x, dout, w_hh, (cell, gates, h_prev, c_prev) in ((x_a, dout_a, w_hh_a, rec[:4]), (x_c, dout_c, w_hh_c, rec[4:])):
            if dout is None:
                grads += [None] * 4
                continue
            grads += _finish(x, _backward_ops(dout, done_rows, w_hh, cell, gates, c_prev), h_prev)
        return (None,) * 7 + tuple(grads)


# ---- the HIP form ---------------------------------------------------------------------------------------------------------------------
def _rows(x):
    """x [T, E, I] as the kernels read it: rows of I contiguous floats, E rows per step, any stride between steps."""
    T, E, I = x.shape
    if x.stride(2) != 1 or x.stride(1) != I or x.stride(0) < E * I:
        x = x.contiguous()
    return x


def hip_forward(x_a, x_c, dones, h0_a, c0_a, h0_c, c0_c, params):
    """`lt_memory_seq_forward`: T launches.  x_*: [T, E, I] f32 (a block `[:, e0:e1]` of the storage is read in place); dones: uint8
    [T, E] (contiguous rows, any stride between steps) or None; params: the eight LSTM parameters (actor's four, critic's four).  Returns the two forward records
    {out, cell, gates, h_prev, c_prev}."""
    from .. import _abi

    T, E, _ = x_a.shape
    H = params[1].shape[1]
    recs, nets = [], []
    for x, h0, c0, (w_ih, w_hh, b_ih, b_hh) in ((x_a, h0_a, c0_a, params[:4]), (x_c, h0_c, c0_c, params[4:])):
        x = _rows(x)
        ops = [t.detach().contiguous() for t in (w_ih, w_hh, b_ih, b_hh, h0, c0)]
        rec = {k: x.new_empty(T, E, 4 * H if k == "gates" else H) for k in ("out", "cell", "gates", "h_prev", "c_prev")}
        nets.append(_abi.LtMemorySeqNet(x=x.data_ptr(), x_stride=x.stride(0), I=x.shape[2], w_ih=ops[0].data_ptr(), w_hh=ops[1].data_ptr(),
                                        b_ih=ops[2].data_ptr(), b_hh=ops[3].data_ptr(), h0=ops[4].data_ptr(), c0=ops[5].data_ptr(),
                                        **{k: v.data_ptr() for k, v in rec.items()}))
        recs.append(rec)
    assert dones is None or (dones.dtype == torch.uint8 and dones.stride(1) == 1)
    _abi.call("lt_memory_seq_forward", nets[0], nets[1], dones, 0 if dones is None else dones.stride(0), T, E, H, _abi.stream(x_a.device))
    return recs


def hip_backward(douts, dones, w_hhs, recs):
    """`lt_memory_seq_backward`: T launches.  Returns the two dgates [T, E, 4H]."""
    from .. import _abi

    T, E, H = recs[0]["out"].shape
    nets, dgs = [], []
    for dout, w_hh, rec in zip(douts, w_hhs, recs):
        dout = torch.zeros_like(rec["out"]) if dout is None else dout.contiguous()
        w = w_hh.detach().contiguous()
        dg, carry = torch.empty_like(rec["gates"]), dout.new_empty(E, H)
        nets.append(_abi.LtMemorySeqGrad(dout=dout.data_ptr(), w_hh=w.data_ptr(), cell=rec["cell"].data_ptr(), gates=rec["gates"].data_ptr(),
                                         c_prev=rec["c_prev"].data_ptr(), dgates=dg.data_ptr(), dc_carry=carry.data_ptr()))
        dgs.append(dg)
    _abi.call("lt_memory_seq_backward", nets[0], nets[1], dones, 0 if dones is None else dones.stride(0), T, E, H, _abi.stream(dgs[0].device))
    return dgs


class _MemorySeqHip(torch.autograd.Function):
    """Both memories, time loops in csrc/lt_memory.hip."""

    @staticmethod
    def forward(ctx, x_a, x_c, dones, h0_a, c0_a, h0_c, c0_c, *params):
        ra, rc = hip_forward(x_a, x_c, dones, h0_a, c0_a, h0_c, c0_c, params)
        ctx.save_for_backward(x_a, x_c, dones, params[1], params[5], *(r[k] for r in (ra, rc) for k in ("out", "cell", "gates", "h_prev", "c_prev")))
        ctx.set_materialize_grads(False)
        return ra["out"], rc["out"]

    @staticmethod
    def backward(ctx, dout_a, dout_c):
        x_a, x_c, dones, w_hh_a, w_hh_c, *rec = ctx.saved_tensors
        keys = ("out", "cell", "gates", "h_prev", "c_prev")
        recs = [dict(zip(keys, rec[:5])), dict(zip(keys, rec[5:]))]
        dgs = hip_backward((dout_a, dout_c), dones, (w_hh_a, w_hh_c), recs)
        grads = []
        for x, dg, r in zip((x_a, x_c), dgs, recs):
            grads += _finish(x, dg, r["h_prev"])
        return (None,) * 7 + tuple(grads)


# ---- GRU memories: the PyTorch-op form -------------------------------------------------------------------------------------------------
def _gru_state(h0, E):
    """h0 as [E, H] from a `saved_hidden_states[0][0][:, e0:e1]`-shaped ([1, E, H]) or [E, H] tensor, or a 1-tuple of one."""
    if isinstance(h0, (tuple, list)):
        (h0,) = h0
    return h0.reshape(E, -1)


def _gru_forward_ops(x, done_rows, h0, w_ih, w_hh, b_ih, b_hh):
    """One network (PyTorch's gate order r, z, n).  Returns the forward record (out, gates [T, E, 4H] = r | z | n | hn, h_prev)."""
    T, E, _ = x.shape
    H = w_hh.shape[1]
    ig = torch.addmm(b_ih, x.reshape(T * E, -1), w_ih.t()).view(T, E, 3 * H)
    w_hh_t = w_hh.t().contiguous()
    out, h_prev = x.new_empty(T, E, H), x.new_empty(T, E, H)
    gates = x.new_empty(T, E, 4 * H)
    h = h0
    for t in range(T):
        if t > 0 and done_rows is not None:
            h = torch.where(done_rows[t - 1], torch.zeros_like(h), h)
        h_prev[t] = h
        hg = torch.addmm(b_hh, h, w_hh_t)  # b_hn stays inside r * (...)
        r = torch.sigmoid(ig[t, :, :H] + hg[:, :H])
        z = torch.sigmoid(ig[t, :, H:2 * H] + hg[:, H:2 * H])
        hn = hg[:, 2 * H:]
        n = torch.tanh(ig[t, :, 2 * H:] + r * hn)
        h = (1 - z) * n + z * h
        gates[t] = torch.cat([r, z, n, hn], dim=1)
        out[t] = h
    return out, gates, h_prev


def _gru_backward_ops(dout, done_rows, w_hh, gates, h_prev):
    """(dig, dhg), each [T, E, 3H], of one network from the forward record."""
    T, E, H = h_prev.shape
    dig, dhg = h_prev.new_empty(T, E, 3 * H), h_prev.new_empty(T, E, 3 * H)
    back = None  # what step t + 1 hands to step t: dhg[t+1] W_hh + dh_{t+1} z_{t+1}
    for t in range(T - 1, -1, -1):
        dh = dout[t]
        if back is not None:
            if done_rows is not None:
                back = torch.where(done_rows[t], torch.zeros_like(back), back)
            dh = dh + back
        r, z, n, hn = gates[t].split(H, dim=1)
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * (h_prev[t] - n) * z * (1 - z)
        dr = dn * hn * r * (1 - r)
        dig[t] = torch.cat([dr, dz, dn], dim=1)
        dhg[t] = torch.cat([dr, dz, dn * r], dim=1)
        back = dhg[t] @ w_hh + dh * z
    return dig, dhg


def _gru_finish(x, dig, dhg, h_prev):
    """(dW_ih, dW_hh, db_ih, db_hh) of one network: everything of the backward pass that is not sequential, one call each."""
    T, E, H = h_prev.shape
    di2, dh2 = dig.view(T * E, 3 * H), dhg.view(T * E, 3 * H)
    return _wgrad(di2, x.reshape(T * E, -1)), _wgrad(dh2, h_prev.view(T * E, H)), di2.sum(0), dh2.sum(0)


class _GruMemorySeq(torch.autograd.Function):
    """Both GRU memories, time loop in PyTorch ops."""

    @staticmethod
    def forward(ctx, x_a, x_c, dones, h0_a, h0_c, *params):
        done_rows = None if dones is None else (dones != 0).unsqueeze(-1)
        ra = _gru_forward_ops(x_a, done_rows, h0_a, *params[:4])
        rc = _gru_forward_ops(x_c, done_rows, h0_c, *params[4:])
        ctx.save_for_backward(x_a, x_c, done_rows, params[1], params[5], *ra[1:], *rc[1:])
        ctx.set_materialize_grads(False)
        return ra[0], rc[0]

    @staticmethod
    def backward(ctx, dout_a, dout_c):
        x_a, x_c, done_rows, w_hh_a, w_hh_c, *rec = ctx.saved_tensors
        grads = []
        for x, dout, w_hh, (gates, h_prev) in ((x_a, dout_a, w_hh_a, rec[:2]), (x_c, dout_c, w_hh_c, rec[2:])):
            if dout is None:
                grads += [None] * 4
                continue
            grads += _gru_finish(x, *_gru_backward_ops(dout, done_rows, w_hh, gates, h_prev), h_prev)
        return (None,) * 5 + tuple(grads)


# ---- GRU memories: the HIP form --------------------------------------------------------------------------------------------------------
def gru_hip_forward(x_a, x_c, dones, h0_a, h0_c, params):
    """`lt_memory_gru_seq_forward`: T launches.  Arguments as `hip_forward` without the cell states; params: the eight GRU parameters.
    Returns the two forward records {out, gates, h_prev}."""
    from .. import _abi

    T, E, _ = x_a.shape
    H = params[1].shape[1]
    recs, nets = [], []
    for x, h0, (w_ih, w_hh, b_ih, b_hh) in ((x_a, h0_a, params[:4]), (x_c, h0_c, params[4:])):
        x = _rows(x)
        ops = [t.detach().contiguous() for t in (w_ih, w_hh, b_ih, b_hh, h0)]
        rec = {k: x.new_empty(T, E, 4 * H if k == "gates" else H) for k in ("out", "gates", "h_prev")}
        nets.append(_abi.LtMemoryGruSeqNet(x=x.data_ptr(), x_stride=x.stride(0), I=x.shape[2], w_ih=ops[0].data_ptr(), w_hh=ops[1].data_ptr(),
                                           b_ih=ops[2].data_ptr(), b_hh=ops[3].data_ptr(), h0=ops[4].data_ptr(),
                                           **{k: v.data_ptr() for k, v in rec.items()}))
        recs.append(rec)
    assert dones is None or (dones.dtype == torch.uint8 and dones.stride(1) == 1)
    _abi.call("lt_memory_gru_seq_forward", nets[0], nets[1], dones, 0 if dones is None else dones.stride(0), T, E, H, _abi.stream(x_a.device))
    return recs


def gru_hip_backward(douts, dones, w_hhs, recs):
    """`lt_memory_gru_seq_backward`: T launches.  Returns [(dig, dhg)] of the two networks, each [T, E, 3H]."""
    from .. import _abi

    T, E, H = recs[0]["out"].shape
    nets, dgs = [], []
    for dout, w_hh, rec in zip(douts, w_hhs, recs):
        dout = torch.zeros_like(rec["out"]) if dout is None else dout.contiguous()
        w = w_hh.detach().contiguous()
        dig, dhg, carry = dout.new_empty(T, E, 3 * H), dout.new_empty(T, E, 3 * H), dout.new_empty(E, H)
        nets.append(_abi.LtMemoryGruSeqGrad(dout=dout.data_ptr(), w_hh=w.data_ptr(), gates=rec["gates"].data_ptr(), h_prev=rec["h_prev"].data_ptr(),
                                            dig=dig.data_ptr(), dhg=dhg.data_ptr(), dh_carry=carry.data_ptr()))
        dgs.append((dig, dhg))
    _abi.call("lt_memory_gru_seq_backward", nets[0], nets[1], dones, 0 if dones is None else dones.stride(0), T, E, H,
              _abi.stream(dgs[0][0].device))
    return dgs


class _GruMemorySeqHip(torch.autograd.Function):
    """Both GRU memories, time loops in csrc/lt_memory_gru.hip."""

    @staticmethod
    def forward(ctx, x_a, x_c, dones, h0_a, h0_c, *params):
        ra, rc = gru_hip_forward(x_a, x_c, dones, h0_a, h0_c, params)
        ctx.save_for_backward(x_a, x_c, dones, params[1], params[5], *(r[k] for r in (ra, rc) for k in ("out", "gates", "h_prev")))
        ctx.set_materialize_grads(False)
        return ra["out"], rc["out"]

    @staticmethod
    def backward(ctx, dout_a, dout_c):
        x_a, x_c, dones, w_hh_a, w_hh_c, *rec = ctx.saved_tensors
        keys = ("out", "gates", "h_prev")
        recs = [dict(zip(keys, rec[:3])), dict(zip(keys, rec[3:]))]
        dgs = gru_hip_backward((dout_a, dout_c), dones, (w_hh_a, w_hh_c), recs)
        grads = []
        for x, (dig, dhg), r in zip((x_a, x_c), dgs, recs):
            grads += _gru_finish(x, dig, dhg, r["h_prev"])
        return (None,) * 5 + tuple(grads)


def unsupported(memory_a, memory_c, obs=None, critic_obs=None, kernels: bool = True, gru_memories: bool = False) -> str | None:
    """Why `PPO(fused_recurrent_update=True)` and `memory_rollout_sequence` refuse these memories / rows (None: they do not):
    include/lt_memory_seq.h covers two single-layer LSTMs with biases of one hidden size, a multiple of 64 in [64, 512], with
    I + H <= 1248, on observation rows - BOTH tensors - of the memories' dtype (the HIP form itself: f32 on a GPU, `serves`; the
    PyTorch-op form covers the same set on the CPU and in other dtypes).  `kernels=False`: what the PyTorch-op form refuses as well - all
    of the above but the bounds on the sizes.  `gru_memories=True` (the opt-in `fused_gru_memories`): two GRUs of the same description
    are served as well (include/lt_memory_gru.h), one LSTM beside one GRU is not."""
    kind = type(getattr(memory_a, "rnn", None)) if gru_memories and _is_gru(memory_a) else torch.nn.LSTM
    for name, m in (("memory_a", memory_a), ("memory_c", memory_c)):
        rnn = getattr(m, "rnn", None)
        if not isinstance(rnn, kind):
            if gru_memories and isinstance(rnn, (torch.nn.LSTM, torch.nn.GRU)):
                return f"{name} is a {type(rnn).__name__} beside a {kind.__name__}: the two memories must be of one kind"
            return f"{name} is a {type(rnn).__name__}: only LSTM memories are served"
        if rnn.num_layers != 1 or rnn.bidirectional or rnn.batch_first or not rnn.bias or getattr(rnn, "proj_size", 0) != 0:
            return (f"{name} must be a single-layer, unidirectional, time-major {kind.__name__} with biases and without projection "
                    f"(it has {rnn.num_layers} layers)")
        h = rnn.hidden_size
        if not kernels:
            continue
        if h % 64 or not MIN_HIDDEN <= h <= MAX_HIDDEN:
            return f"{name}: hidden size {h} is not a multiple of 64 in [{MIN_HIDDEN}, {MAX_HIDDEN}]"
        if rnn.input_size + h > MAX_K:
            return f"{name}: input size + hidden size exceeds {MAX_K}"
    if memory_a.rnn.hidden_size != memory_c.rnn.hidden_size:
        return "the two memories differ in hidden size"
    for what, rows, m in (("observation", obs, memory_a), ("critic observation", critic_obs, memory_c)):
        if rows is not None and rows.dtype != m.rnn.weight_ih_l0.dtype:
            return f"{str(rows.dtype).replace('torch.', '')} {what} rows: the memories read rows of their own dtype (f32 on the GPU)"
    return None


def _is_gru(memory) -> bool:
    return isinstance(getattr(memory, "rnn", None), torch.nn.GRU)


def serves(memory_a, memory_c, obs: torch.Tensor, critic_obs: torch.Tensor | None = None, gru_memories: bool = False) -> bool:
    """Whether `memory_rollout_sequence` sends (memories, obs, critic_obs) through the HIP form: f32 rows and parameters on a GPU, in
    the set `unsupported` describes."""
    critic_obs = obs if critic_obs is None else critic_obs
    return bool(use_hip_kernels and obs.is_cuda and critic_obs.is_cuda and obs.dtype == torch.float32 and memory_a.rnn.weight_ih_l0.is_cuda
                and unsupported(memory_a, memory_c, obs, critic_obs, gru_memories=gru_memories) is None)


def memory_rollout_sequence(memory_a, memory_c, obs, critic_obs, dones, hc0_a, hc0_c, gru_memories: bool = False):
    """(out_a, out_c), each [T, E, H]: `memory_a` over obs [T, E, I_a] and `memory_c` over critic_obs [T, E, I_c] for the whole rollout of
    an env block, from the states hc0_* = (h0, c0) saved at step 0 ([1, E, H] or [E, H]); the carried state is replaced by zeros wherever
    dones[t - 1] ([T, E] or [T, E, 1], any integer or bool dtype; None: no reset) is set.

    obs / critic_obs may be views `storage[:, e0:e1]`: the forward pass reads them in place.  The weight gradient dW_ih = dgates^T X
    wants contiguous rows, though, so the BACKWARD pass of a call on such a view copies the block (`reshape`) each time; a caller that
    runs the same blocks more than once hands over contiguous copies made once, as `PPO._recurrent_update` does per update.

    Rows whose dtype is not the memories' own, GRU or multi-layer memories raise `ValueError`; there is no quiet change of path on them.
    The HIP form runs where `serves` says so, the PyTorch-op form elsewhere (the CPU, other dtypes, `use_hip_kernels` off).

    `gru_memories=True`: two GRU memories are served too; hc0_* is then the one state tensor h0 ([1, E, H] or [E, H], or a 1-tuple)."""
    T, E, _ = obs.shape
    why = unsupported(memory_a, memory_c, obs, critic_obs, kernels=False, gru_memories=gru_memories)  # (a size outside the kernels' set has the PyTorch-op form)
    if why is not None:
        raise ValueError(f"memory_rollout_sequence: {why}")
    d = _dones2d(dones, T, E)
    if gru_memories and _is_gru(memory_a):
        states = (_gru_state(hc0_a, E), _gru_state(hc0_c, E))
        params = (*_params(memory_a), *_params(memory_c))
        if serves(memory_a, memory_c, obs, critic_obs, gru_memories=True):
            return _GruMemorySeqHip.apply(obs, critic_obs, _dones_bytes(d), *states, *params)
        return _GruMemorySeq.apply(obs, critic_obs, d, *states, *params)
    states = (*_state(hc0_a, E), *_state(hc0_c, E))
    params = (*_params(memory_a), *_params(memory_c))
    if serves(memory_a, memory_c, obs, critic_obs):
        return _MemorySeqHip.apply(obs, critic_obs, _dones_bytes(d), *states, *params)
    return _MemorySeq.apply(obs, critic_obs, d, *states, *params)


# False: `memory_rollout_sequence` takes the PyTorch-op time loop on the GPU as well.
use_hip_kernels = True
