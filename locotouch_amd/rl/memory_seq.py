"""The two memories of a recurrent policy over a WHOLE ROLLOUT of an env block: what `PPO._recurrent_update` runs per optimizer step
instead of padded trajectories (`split_and_pad_trajectories` -> two sequence passes -> two `unpad_trajectories`).

Why this equals the padded form: `PolicyMemory.reset(dones)` zeroes the state of done envs, so the hidden state saved at the first step
of a trajectory that starts after a done is all zeros.  The padded batch of trajectories that starts from the saved states therefore
equals, row for row, ONE pass over the block's envs for all T steps that starts from `saved_hidden_states[0][:, e0:e1]` and replaces the
carried state by zeros wherever `dones[t - 1]` is set.  No gradient crosses a done in either form (the padded tail has dout = 0, the
reset state is a constant), and the output [T, E, H] is already in the row order `unpad_trajectories` produces
(tests/test_recurrent_update_form.py, tests/test_gru_update_form.py).

Two kinds of memory are served, and everything this side knows about a kind stands once, in its `Cell`: `LSTM`, and `GRU` behind the
opt-in `gru_memories=True` (`fused_gru_memories` of rl/ppo.py and rl/fused.py).

    LSTM  state (h, c); forward record (out, cell, gates = i | f | g | o, h_prev, c_prev); the backward pass leaves ONE gate-gradient
          array, dgates [T, E, 4H], which feeds both dW_ih / db_ih and dW_hh / db_hh.  csrc/lt_memory.hip; include/lt_memory.h (one
          rollout step) and include/lt_memory_seq.h (whole rollouts).
    GRU   state h; forward record (out, gates = r | z | n | hn, h_prev); the backward pass leaves TWO arrays, dig = (dr, dz, dn) and dhg
          = (dr, dz, dn * r), each [T, E, 3H]: dW_ih = dig^T X and db_ih come from the first, dW_hh = dhg^T h_prev and db_hh from the
          second, each as the kernel wrote it.  csrc/lt_memory_gru.hip; include/lt_memory_gru.h.

`memory_rollout_sequence` is one `torch.autograd.Function` over both memories' `nn.LSTM` / `nn.GRU` parameters (the modules' own:
checkpoints are unaffected), in two forms as rl/lstm.py:
  * `_SeqOps`: a PyTorch-op time loop (the cell's `forward_ops` / `backward_ops`) with `where(dones[t - 1], 0, .)` on the carry: the
    CPU, any dtype, shapes the kernels do not cover;
  * `_SeqHip`: the cell's `seq_forward` (T launches, both networks in each, the observation rows read in place) and `seq_backward` (T
    launches) - both cells on the one row-block kernel of csrc/lt_memory_tile.h.  What is not sequential stays outside the loop, one
    call each (`_finish`): the two weight gradients through rl/gru.py `_wgrad`, the bias gradients as column sums.
The initial states carry no gradient.  The rows do where they ask for one (`requires_grad`: a layer stands in front of the memory):
dX = d_ih W_ih, `input_grad` - csrc/lt_memory_dx.hip, include/lt_memory_dx.h, ONE launch for both networks behind `seq_backward` - in
the HIP form, the same product as a PyTorch op in `_SeqOps`.  Rows that ask for none launch nothing more than before.

`direct_forward` / `direct_backward` are the HIP form WITHOUT the autograd Function, for `PPO._direct_recurrent_update`: the records out,
(dout_a, dout_c) in, the eight parameter gradients written in place into given views - and, given `dx_out`, the two input gradients.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import torch

from .. import _abi
from .gru import _wgrad

MIN_HIDDEN, MAX_HIDDEN, MAX_K = 64, 512, 1248  # include/lt_memory.h, include/lt_memory_seq.h, include/lt_memory_gru.h


@dataclass(frozen=True)
class Cell:
    """One kind of memory.  Widths are in units of H."""
    nn: type                # the module class of `PolicyMemory.rnn`
    state: tuple            # the initial-state fields of the sequence structure: as many tensors per memory, in this order
    record: tuple           # (key, width) of the forward record, in the order `forward_ops` returns it; keys are the structure's fields
    dgates: tuple           # (key, width) of the gate-gradient arrays, in the order `backward_ops` returns them; keys as above
    d_ih: str               # the gate-gradient array behind dW_ih and db_ih
    d_hh: str               # the one behind dW_hh and db_hh (times W_hh: what a step hands to the one before it)
    reads: tuple            # record keys the backward structure reads, in the order `backward_ops` takes them
    carry: str              # the backward structure's [E, H] scratch field
    step_net: type          # ctypes structures: one rollout step, the sequence forward pass, the sequence backward pass
    seq_net: type
    seq_grad: type
    step: str               # entry points
    finish: str
    seq_forward: str
    seq_backward: str
    backward_units: str
    forward_ops: Callable   # the PyTorch-op form: (x, done_rows, *state, w_ih, w_hh, b_ih, b_hh) -> the record
    backward_ops: Callable  # (dout, done_rows, w_hh, *reads) -> the gate-gradient arrays


def _params(memory):
    rnn = memory.rnn
    return rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0



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


# ---- the PyTorch-op forms -------------------------------------------------------------------------------------------------------------
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
    """(dgates,), [T, E, 4H], of one network from the forward record."""
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
    return (dgates,)


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

LSTM = Cell(nn=torch.nn.LSTM, state=("h0", "c0"), record=(("out", 1), ("cell", 1), ("gates", 4), ("h_prev", 1), ("c_prev", 1)),
            dgates=(("dgates", 4),), d_ih="dgates", d_hh="dgates", reads=("cell", "gates", "c_prev"), carry="dc_carry",
            step_net=_abi.LtMemoryNet, seq_net=_abi.LtMemorySeqNet, seq_grad=_abi.LtMemorySeqGrad,
            step="lt_memory_step", finish="lt_memory_finish", seq_forward="lt_memory_seq_forward", seq_backward="lt_memory_seq_backward",
            backward_units="lt_memory_seq_backward_units", forward_ops=_forward_ops, backward_ops=_backward_ops)
GRU = Cell(nn=torch.nn.GRU, state=("h0",), record=(("out", 1), ("gates", 4), ("h_prev", 1)),
           dgates=(("dig", 3), ("dhg", 3)), d_ih="dig", d_hh="dhg", reads=("gates", "h_prev"), carry="dh_carry",
           step_net=_abi.LtMemoryGruNet, seq_net=_abi.LtMemoryGruSeqNet, seq_grad=_abi.LtMemoryGruSeqGrad,
           step="lt_memory_gru_step", finish="lt_memory_gru_finish", seq_forward="lt_memory_gru_seq_forward",
           seq_backward="lt_memory_gru_seq_backward", backward_units="lt_memory_gru_seq_backward_units",
           forward_ops=_gru_forward_ops, backward_ops=_gru_backward_ops)


def cell_of(memory, gru_memories: bool = False) -> Cell:
    """The cell `memory` is held to: `GRU` for an `nn.GRU` behind the opt-in, `LSTM` for everything else (`memories_unsupported` says
    what does not fit it)."""
    return GRU if gru_memories and isinstance(getattr(memory, "rnn", None), torch.nn.GRU) else LSTM


def _state(cell, hc0, E):
    """The cell's state tensors as [E, H] from a tuple of `saved_hidden_states[i][0][:, e0:e1]`-shaped ([1, E, H]) or [E, H] tensors; a
    one-state cell takes the bare tensor as well."""
    hc0 = (hc0,) if torch.is_tensor(hc0) else tuple(hc0)
    if len(hc0) != len(cell.state):
        raise ValueError(f"a {cell.nn.__name__} memory starts from {len(cell.state)} state tensor(s), not {len(hc0)}")
    return tuple(s.reshape(E, -1) for s in hc0)


def _finish(cell, x, grads, h_prev):
    """(dW_ih, dW_hh, db_ih, db_hh) of one network from its gate-gradient arrays: everything of the backward pass that is not sequential,
    one call each."""
    T, E, H = h_prev.shape
    d_ih, d_hh = (grads[k].view(T * E, -1) for k in (cell.d_ih, cell.d_hh))
    db_ih = d_ih.sum(0)
    db_hh = db_ih.clone() if cell.d_hh == cell.d_ih else d_hh.sum(0)
    return _wgrad(d_ih, x.reshape(T * E, -1)), _wgrad(d_hh, h_prev.view(T * E, H)), db_ih, db_hh


def _records(cell, saved):
    """The two forward records, as dicts, from the tensors `save_for_backward` held."""
    keys = [k for k, _ in cell.record]
    return dict(zip(keys, saved[:len(keys)])), dict(zip(keys, saved[len(keys):]))


class _SeqOps(torch.autograd.Function):
    """Both memories, time loop in PyTorch ops.  Arguments behind the dones: the state tensors (the actor's, then the critic's), then
    the eight parameters."""

    @staticmethod
    def forward(ctx, cell, x_a, x_c, dones, *rest):
        ns = len(cell.state)
        states, params = rest[:2 * ns], rest[2 * ns:]
        done_rows = None if dones is None else (dones != 0).unsqueeze(-1)
        ra = cell.forward_ops(x_a, done_rows, *states[:ns], *params[:4])
        rc = cell.forward_ops(x_c, done_rows, *states[ns:], *params[4:])
        ctx.cell = cell
        ctx.save_for_backward(x_a, x_c, done_rows, params[1], params[5], params[0], params[4], *ra, *rc)
        ctx.set_materialize_grads(False)
        return ra[0], rc[0]

    @staticmethod
    def backward(ctx, dout_a, dout_c):
        cell = ctx.cell
        x_a, x_c, done_rows, w_hh_a, w_hh_c, w_ih_a, w_ih_c, *saved = ctx.saved_tensors
        grads, dxs = [], [None, None]
        for k, (x, dout, w_hh, w_ih, rec) in enumerate(zip((x_a, x_c), (dout_a, dout_c), (w_hh_a, w_hh_c), (w_ih_a, w_ih_c), _records(cell, saved))):
            if dout is None:
                grads += [None] * 4
                continue
            dgs = dict(zip((key for key, _ in cell.dgates), cell.backward_ops(dout, done_rows, w_hh, *(rec[key] for key in cell.reads))))
            grads += _finish(cell, x, dgs, rec["h_prev"])
            if ctx.needs_input_grad[1 + k]:  # the rows ask: dX = d_ih W_ih
                dxs[k] = (dgs[cell.d_ih].reshape(-1, w_ih.shape[0]) @ w_ih).view(x.shape).to(x.dtype)
        return (None, *dxs, None) + (None,) * (2 * len(cell.state)) + tuple(grads)


# ---- the HIP form ---------------------------------------------------------------------------------------------------------------------
def _rows(x):
    """x [T, E, I] as the kernels read it: rows of I contiguous floats, E rows per step, any stride between steps."""
    T, E, I = x.shape
    if x.stride(2) != 1 or x.stride(1) != I or x.stride(0) < E * I:
        x = x.contiguous()
    return x


def hip_forward(cell, x_a, x_c, dones, states, params):
    """The cell's `seq_forward`: T launches.  x_*: [T, E, I] f32 (a block `[:, e0:e1]` of the storage is read in place); dones: uint8
    [T, E] (contiguous rows, any stride between steps) or None; states: the [E, H] state tensors, the actor's then the critic's; params:
    the eight parameters (actor's four, critic's four).  Returns the two forward records, dicts over the keys of `cell.record`."""
    T, E, _ = x_a.shape
    H = params[1].shape[1]
    ns = len(cell.state)
    recs, nets = [], []
    for k, x in enumerate((x_a, x_c)):
        x = _rows(x)
        ops = [t.detach().contiguous() for t in (*params[4 * k:4 * k + 4], *states[ns * k:ns * k + ns])]
        rec = {key: x.new_empty(T, E, w * H) for key, w in cell.record}
        nets.append(cell.seq_net(x=x.data_ptr(), x_stride=x.stride(0), I=x.shape[2],
                                 **{f: t.data_ptr() for f, t in zip(("w_ih", "w_hh", "b_ih", "b_hh") + cell.state, ops)},
                                 **{key: v.data_ptr() for key, v in rec.items()}))
        recs.append(rec)
    assert dones is None or (dones.dtype == torch.uint8 and dones.stride(1) == 1)
    _abi.call(cell.seq_forward, nets[0], nets[1], dones, 0 if dones is None else dones.stride(0), T, E, H, _abi.stream(x_a.device))
    return recs


def hip_backward(cell, douts, dones, w_hhs, recs):
    """The cell's `seq_backward`: T launches.  Returns the gate-gradient arrays of the two networks, dicts over the keys of `cell.dgates`."""
    T, E, H = recs[0]["out"].shape
    nets, dgs = [], []
    for dout, w_hh, rec in zip(douts, w_hhs, recs):
        dout = torch.zeros_like(rec["out"]) if dout is None else dout.contiguous()
        w = w_hh.detach().contiguous()
        dg = {key: dout.new_empty(T, E, width * H) for key, width in cell.dgates}
        carry = dout.new_empty(E, H)
        nets.append(cell.seq_grad(dout=dout.data_ptr(), w_hh=w.data_ptr(), **{key: rec[key].data_ptr() for key in cell.reads},
                                  **{key: v.data_ptr() for key, v in dg.items()}, **{cell.carry: carry.data_ptr()}))
        dgs.append(dg)
    _abi.call(cell.seq_backward, nets[0], nets[1], dones, 0 if dones is None else dones.stride(0), T, E, H, _abi.stream(recs[0]["out"].device))
    return dgs


def input_grad(cell, dgs, w_ihs, outs=None):
    """The gradients of the two networks' input rows, dx_k = d_ih_k W_ih_k, in ONE launch (include/lt_memory_dx.h).  dgs: the two
    gate-gradient dicts `hip_backward` returns; w_ihs: the two [gates * H, I_k] weights (views of a flat bucket will do).  outs: None -
    two new [T, E, I_k] tensors - or a pair of f32 views to write, each [T, E, I_k] or [T * E, I_k] with unit stride along I_k and evenly
    spaced rows (the tail columns of a wider gradient row): every element of the views is written, nothing outside them.  Returns the
    pair."""
    d = [dg[cell.d_ih] for dg in dgs]
    T, E, K = d[0].shape
    gates = dict(cell.dgates)[cell.d_ih]
    ws = [w.detach().contiguous() for w in w_ihs]
    outs = [g.new_empty(T, E, w.shape[1]) for g, w in zip(d, ws)] if outs is None else list(outs)
    nets = []
    for g, w, out in zip(d, ws, outs):
        I = w.shape[1]
        assert g.is_contiguous() and g.shape == (T, E, K) and w.shape[0] == K
        assert out.dtype == torch.float32 and out.shape in ((T, E, I), (T * E, I)), "dx views: f32 [T, E, I] or [T * E, I]"
        rows = out.view(T * E, I)  # (raises unless the rows are evenly spaced)
        assert rows.stride(1) == 1 or I == 1, "dx views: unit stride along I"
        nets.append(_abi.LtMemoryDxNet(dg=g.data_ptr(), w_ih=w.data_ptr(), I=I, dx=rows.data_ptr(), dx_stride=rows.stride(0) if T * E > 1 else I))
    _abi.call("lt_memory_input_grad", nets[0], nets[1], T * E, K // gates, gates, _abi.stream(d[0].device))
    return tuple(outs)


def _wgrad_into(dst, dy2d, x2d) -> None:
    """`dst` = rl/gru.py `_wgrad(dy2d, x2d)`, the same operations in the same order, the last of them writing in place."""
    from .linear import pick_splits

    m = dy2d.shape[0]
    s = pick_splits(m) if dy2d.is_cuda else 1
    if s > 1:
        torch.sum(torch.bmm(dy2d.view(s, m // s, -1).transpose(1, 2), x2d.view(s, m // s, -1)), dim=0, out=dst)
    else:
        torch.mm(dy2d.t(), x2d, out=dst)


def direct_forward(cell, memory_a, memory_c, x_a, x_c, dones, hc0_a, hc0_c):
    """Both memories over a whole rollout of an env block WITHOUT an autograd graph (`PPO._direct_recurrent_update`): the cell's
    `seq_forward` on the live parameters.  x_*: contiguous [T, E, I] f32 blocks; dones: what `_dones_bytes` gives, or None; hc0_*: as
    `memory_rollout_sequence` takes them.  Returns the two forward records (`rec["out"]` [T, E, H] is the memory's output), which
    `direct_backward` consumes."""
    E = x_a.shape[1]
    with torch.no_grad():
        return hip_forward(cell, x_a, x_c, dones, (*_state(cell, hc0_a, E), *_state(cell, hc0_c, E)), (*_params(memory_a), *_params(memory_c)))


def direct_backward(cell, memory_a, memory_c, x_a, x_c, dones, recs, douts, grad_of, dx_out=None) -> None:
    """From (dout_a, dout_c), each [T, E, H] (or [T * E, H]) contiguous f32, to the eight parameter gradients, written IN PLACE into
    `grad_of[param]` (views of the flat gradient bucket; every element of each is written): the cell's `seq_backward`, then per network
    what `_finish` does - dW_ih, dW_hh as split-K GEMMs, db_ih, db_hh as column sums - with the last operation of each writing its
    view.  One code path for both cells, through the `Cell` table.  dx_out: None, or a pair of views as `input_grad` takes them: the
    gradients of the two networks' input rows are written there as well, from the gate gradients already at hand (one launch more)."""
    with torch.no_grad():
        T, E, H = recs[0]["out"].shape
        mems = (memory_a, memory_c)
        dgs = hip_backward(cell, tuple(d.view(T, E, H) for d in douts), dones, tuple(_params(m)[1] for m in mems), recs)
        for mem, x, dg, rec in zip(mems, (x_a, x_c), dgs, recs):
            w_ih, w_hh, b_ih, b_hh = _params(mem)
            d_ih, d_hh = (dg[k].view(T * E, -1) for k in (cell.d_ih, cell.d_hh))
            torch.sum(d_ih, dim=0, out=grad_of[b_ih])
            if cell.d_hh == cell.d_ih:
                grad_of[b_hh].copy_(grad_of[b_ih])
            else:
                torch.sum(d_hh, dim=0, out=grad_of[b_hh])
            _wgrad_into(grad_of[w_ih], d_ih, x.reshape(T * E, -1))
            _wgrad_into(grad_of[w_hh], d_hh, rec["h_prev"].view(T * E, H))
        if dx_out is not None:
            input_grad(cell, dgs, tuple(_params(m)[0] for m in mems), dx_out)


class _SeqHip(torch.autograd.Function):
    """Both memories, time loops in csrc/lt_memory.hip / csrc/lt_memory_gru.hip.  Arguments as `_SeqOps`."""

    @staticmethod
    def forward(ctx, cell, x_a, x_c, dones, *rest):
        ns = len(cell.state)
        ra, rc = hip_forward(cell, x_a, x_c, dones, rest[:2 * ns], rest[2 * ns:])
        ctx.cell = cell
        ctx.save_for_backward(x_a, x_c, dones, rest[2 * ns + 1], rest[2 * ns + 5], rest[2 * ns], rest[2 * ns + 4], *ra.values(), *rc.values())
        ctx.set_materialize_grads(False)
        return ra["out"], rc["out"]

    @staticmethod
    def backward(ctx, dout_a, dout_c):
        cell = ctx.cell
        x_a, x_c, dones, w_hh_a, w_hh_c, w_ih_a, w_ih_c, *saved = ctx.saved_tensors
        recs = _records(cell, saved)
        dgs = hip_backward(cell, (dout_a, dout_c), dones, (w_hh_a, w_hh_c), recs)
        grads = []
        for x, dg, rec in zip((x_a, x_c), dgs, recs):
            grads += _finish(cell, x, dg, rec["h_prev"])
        dxs = (None, None)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:  # one launch serves both; a row's bits do not depend on the other network
            dxs = tuple(dx if need else None for dx, need in zip(input_grad(cell, dgs, (w_ih_a, w_ih_c)), ctx.needs_input_grad[1:3]))
        return (None, *dxs, None) + (None,) * (2 * len(cell.state)) + tuple(grads)


# ---- what is served, and the entry point ----------------------------------------------------------------------------------------------
def memories_unsupported(memory_a, memory_c, gru_memories: bool = False, kernels: bool = True, layer_count: bool = False) -> str | None:
    """What `unsupported` here and `recurrent_unsupported` of rl/fused.py ask of the memories themselves (None: nothing is amiss): both of
    the one kind `cell_of(memory_a)` names, single-layer and plain, and - `kernels` - of one hidden size within the limits of the
    headers.  `layer_count`: the message about the layers ends in the number the memory has."""
    kind = cell_of(memory_a, gru_memories).nn
    for name, m in (("memory_a", memory_a), ("memory_c", memory_c)):
        rnn = getattr(m, "rnn", None)
        if not isinstance(rnn, kind):
            if gru_memories and isinstance(rnn, (torch.nn.LSTM, torch.nn.GRU)):
                return f"{name} is a {type(rnn).__name__} beside a {kind.__name__}: the two memories must be of one kind"
            return f"{name} is a {type(rnn).__name__}: only LSTM memories are served"
        if rnn.num_layers != 1 or rnn.bidirectional or rnn.batch_first or not rnn.bias or getattr(rnn, "proj_size", 0) != 0:
            return (f"{name} must be a single-layer, unidirectional, time-major {kind.__name__} with biases and without projection"
                    + (f" (it has {rnn.num_layers} layers)" if layer_count else ""))
        h = rnn.hidden_size
        if not kernels:
            continue
        if h % 64 or not MIN_HIDDEN <= h <= MAX_HIDDEN:
            return f"{name}: hidden size {h} is not a multiple of 64 in [{MIN_HIDDEN}, {MAX_HIDDEN}]"
        if rnn.input_size + h > MAX_K:
            return f"{name}: input size + hidden size exceeds {MAX_K}"
    if memory_a.rnn.hidden_size != memory_c.rnn.hidden_size:
        return "the two memories differ in hidden size"
    return None


def unsupported(memory_a, memory_c, obs=None, critic_obs=None, kernels: bool = True, gru_memories: bool = False) -> str | None:
    """Why `PPO(fused_recurrent_update=True)` and `memory_rollout_sequence` refuse these memories / rows (None: they do not):
    include/lt_memory_seq.h covers two single-layer LSTMs with biases of one hidden size, a multiple of 64 in [64, 512], with
    I + H <= 1248, on observation rows - BOTH tensors - of the memories' dtype (the HIP form itself: f32 on a GPU, `serves`; the
    PyTorch-op form covers the same set on the CPU and in other dtypes).  `kernels=False`: what the PyTorch-op form refuses as well - all
    of the above but the bounds on the sizes.  `gru_memories=True` (the opt-in `fused_gru_memories`): two GRUs of the same description
    are served as well (include/lt_memory_gru.h), one LSTM beside one GRU is not."""
    why = memories_unsupported(memory_a, memory_c, gru_memories=gru_memories, kernels=kernels, layer_count=True)
    if why is not None:
        return why
    for what, rows, m in (("observation", obs, memory_a), ("critic observation", critic_obs, memory_c)):
        if rows is not None and rows.dtype != m.rnn.weight_ih_l0.dtype:
            return f"{str(rows.dtype).replace('torch.', '')} {what} rows: the memories read rows of their own dtype (f32 on the GPU)"
    return None


def serves(memory_a, memory_c, obs: torch.Tensor, critic_obs: torch.Tensor | None = None, gru_memories: bool = False) -> bool:
    """Whether `memory_rollout_sequence` sends (memories, obs, critic_obs) through the HIP form: f32 rows and parameters on a GPU, in
    the set `unsupported` describes."""
    critic_obs = obs if critic_obs is None else critic_obs
    return bool(use_hip_kernels and obs.is_cuda and critic_obs.is_cuda and obs.dtype == torch.float32 and memory_a.rnn.weight_ih_l0.is_cuda
                and unsupported(memory_a, memory_c, obs, critic_obs, gru_memories=gru_memories) is None)


def memory_rollout_sequence(memory_a, memory_c, obs, critic_obs, dones, hc0_a, hc0_c, gru_memories: bool = False):
    """(out_a, out_c), each [T, E, H]: `memory_a` over obs [T, E, I_a] and `memory_c` over critic_obs [T, E, I_c] for the whole rollout of
    an env block, from the states hc0_* saved at step 0 (a tuple of the cell's state tensors, (h0, c0) or (h0,), each [1, E, H] or [E, H];
    for a GRU the tensor h0 itself will do); the carried state is replaced by zeros wherever dones[t - 1] ([T, E] or [T, E, 1], any
    integer or bool dtype; None: no reset) is set.

    obs / critic_obs may be views `storage[:, e0:e1]`: the forward pass reads them in place.  The weight gradient dW_ih = dgates^T X
    wants contiguous rows, though, so the BACKWARD pass of a call on such a view copies the block (`reshape`) each time; a caller that
    runs the same blocks more than once hands over contiguous copies made once, as `PPO._recurrent_update` does per update.

    Rows that require a gradient get it: dX = d_ih W_ih, one launch more in the HIP form (`input_grad`); rows that require none cost
    nothing more than before, and the parameter gradients are the same bits either way.  The initial states get none.

    Rows whose dtype is not the memories' own, multi-layer memories, and GRU memories without `gru_memories=True` raise `ValueError`;
    there is no quiet change of path on them.  The HIP form runs where `serves` says so, the PyTorch-op form elsewhere (the CPU, other
    dtypes, `use_hip_kernels` off)."""
    T, E, _ = obs.shape
    why = unsupported(memory_a, memory_c, obs, critic_obs, kernels=False, gru_memories=gru_memories)  # (a size outside the kernels' set has the PyTorch-op form)
    if why is not None:
        raise ValueError(f"memory_rollout_sequence: {why}")
    cell = cell_of(memory_a, gru_memories)
    d = _dones2d(dones, T, E)
    states = (*_state(cell, hc0_a, E), *_state(cell, hc0_c, E))
    params = (*_params(memory_a), *_params(memory_c))
    if serves(memory_a, memory_c, obs, critic_obs, gru_memories=gru_memories):
        return _SeqHip.apply(cell, obs, critic_obs, _dones_bytes(d), *states, *params)
    return _SeqOps.apply(cell, obs, critic_obs, d, *states, *params)


# False: `memory_rollout_sequence` takes the PyTorch-op time loop on the GPU as well.
use_hip_kernels = True
