"""What tests/test_memory_seq_input_grad_cpu.py and tests/test_hip_memory_dx.py share: a seeded case of `memory_rollout_sequence` on rows
that may require a gradient, the `nn.LSTMCell` / `nn.GRUCell` loop it is held to, and the project's float64 bound
(tests/test_hip_rnn_encoder_backward.py `held_to_float64`)."""
import torch

from locotouch_amd.rl.memory_seq import memory_rollout_sequence
from locotouch_amd.rl.modules import PolicyMemory

PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


class Case:
    """Two memories of `kind` ("lstm" / "gru"), rows [T, E, I_a] and [T, E, I_c], dones with resets at t = 0 and t = T - 1 among them,
    non-zero initial states and the two output gradients of a made-up loss.  Everything is drawn in float64 on the CPU from `seed`, so
    every (dtype, device) of one case holds the same numbers, rounded.  The case itself is never changed by a run."""

    def __init__(self, kind, T, E, I_a, I_c, H, seed=0, x_width=None):
        g = torch.Generator().manual_seed(seed)
        self.kind, self.T, self.E, self.H, self.widths = kind, T, E, H, (I_a, I_c)
        self.gates = 3 if kind == "gru" else 4
        self.ns = 1 if kind == "gru" else 2
        rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g, dtype=torch.float64) * scale)
        self.x = [rnd(T, E, x_width or I) for I in self.widths]  # x_width: rows for a layer in front of the memories
        self.params = [[rnd(self.gates * H, I, scale=I ** -0.5), rnd(self.gates * H, H, scale=H ** -0.5), rnd(self.gates * H, scale=0.1),
                        rnd(self.gates * H, scale=0.1)] for I in self.widths]
        self.state = [[rnd(E, H, scale=0.5) for _ in range(self.ns)] for _ in self.widths]
        self.dout = [rnd(T, E, H) for _ in self.widths]
        self.dones = torch.rand(T, E, generator=g) < 0.25
        self.dones[0, 0] = self.dones[T - 1, E - 1] = self.dones[T - 1, 0] = True
        self.dones[0, E - 1] = False

    def memories(self, dtype, device):
        mems = []
        for I, ps in zip(self.widths, self.params):
            m = PolicyMemory(I, type=self.kind, hidden_size=self.H).to(device=device, dtype=dtype)
            with torch.no_grad():
                for name, p in zip(PARAMS, ps):
                    getattr(m.rnn, name).copy_(p)
            mems.append(m)
        return mems

    def rows(self, dtype, device, requires_grad):
        return [x.to(device=device, dtype=dtype, copy=True).requires_grad_(requires_grad) for x in self.x]

    def run(self, dtype, device, requires_grad=True, rows=None, mems=None):
        """`memory_rollout_sequence` and the backward pass of sum(out_k * dout_k) -> (row gradients or [None, None], the eight parameter
        gradients, the rows, the memories)."""
        mems = self.memories(dtype, device) if mems is None else mems
        rows = self.rows(dtype, device, requires_grad) if rows is None else rows
        to = lambda t: t.to(device=device, dtype=dtype)
        hc = [tuple(to(s).unsqueeze(0) for s in st) for st in self.state]
        outs = memory_rollout_sequence(mems[0], mems[1], rows[0], rows[1], self.dones.to(device), hc[0], hc[1], gru_memories=self.kind == "gru")
        for m in mems:
            m.zero_grad(set_to_none=True)
        sum((o * to(d)).sum() for o, d in zip(outs, self.dout)).backward()
        return [r.grad if r.is_leaf else None for r in rows], [getattr(m.rnn, n).grad for m in mems for n in PARAMS], rows, mems

    def loop(self, dtype=torch.float64, front=None):
        """The same loss through an `nn.LSTMCell` / `nn.GRUCell` loop on the CPU that zeroes the state behind a done -> (row gradients,
        the eight parameter gradients).  front: a module applied to both networks' rows first (its parameters collect gradients)."""
        rows = [x.to(dtype, copy=True).requires_grad_(True) for x in self.x]
        grads, cells = [], []
        loss = 0.0
        for x, ps, st, dout in zip(rows, self.params, self.state, self.dout):
            xin = x if front is None else front(x)
            cell = (torch.nn.GRUCell if self.kind == "gru" else torch.nn.LSTMCell)(xin.shape[-1], self.H).to(dtype)
            with torch.no_grad():
                for name, p in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), ps):
                    getattr(cell, name).copy_(p)
            cells.append(cell)
            s = [t.to(dtype) for t in st]
            for t in range(self.T):
                if t > 0:
                    s = [torch.where(self.dones[t - 1].unsqueeze(-1), torch.zeros_like(v), v) for v in s]
                s = [cell(xin[t], s[0])] if self.kind == "gru" else list(cell(xin[t], (s[0], s[1])))
                loss = loss + (s[0] * dout[t].to(dtype)).sum()
        loss.backward()
        for cell in cells:
            grads += [getattr(cell, n).grad for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return [r.grad for r in rows], grads


def held(tag, got, ref64, chain32):
    """The project's bound: max|got - f64| <= max(4 max|f32 torch form - f64|, 1e-5 max|ref|).  Prints the two errors."""
    top = float(ref64.abs().max())
    e_got = float((got.double().cpu() - ref64.cpu()).abs().max())
    e_chain = float((chain32.double().cpu() - ref64.cpu()).abs().max())
    print(f"\n[memory dx {tag}] max |err| vs f64  kernel {e_got:.3e}  f32 torch form {e_chain:.3e}  max |ref| {top:.3e}")
    assert top > 0 and e_got <= max(4.0 * e_chain, 1e-5 * top), (tag, e_got, e_chain, top)
