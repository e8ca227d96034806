"""The numpy twin of csrc/lt_episode_stats.hip (include/lt_episode_stats.h states the arithmetic): the per-step term in float32, every
operation rounded on its own and summed left to right from +0.0; the finish and the fold in float64; the reduce over the envs in the
header's ONE order (thread t of 256 walks the envs t, t + 256, ... and a stride-halving tree joins the 256 partials).  The GPU tests
compare the device's state and result with this bit for bit, so nothing here may be reordered."""
import numpy as np

VALUE, ABS, SQUARE, DIFF_SQUARE, ABS_PRODUCT = range(5)
MEAN, SUM, MAX, LAST = range(4)
F_N, F_SUM, F_SUMSQ, F_MIN, F_MAX, FIELDS = range(6)
CAUSES, THREADS = 18, 256
MAX_METRICS, MAX_PAIRS, MAX_ENVS = 16, 12, 16 * 65535 * 16


def plan_bytes(nmetrics):
    return 112 + 784 * nmetrics


def state_bytes(nmetrics, nenvs):
    return nenvs * (40 * (nmetrics + 1) + 8 * nmetrics + 4 + 72 + 1)


def result_bytes(nmetrics):
    return 40 * (nmetrics + 1) + 144


def as_f32(a):
    """A channel's conversion by value (integers round to nearest, ties to even)."""
    return np.asarray(a).astype(np.float32)


def term(kind, pairs):
    """s of one step for all envs: `pairs` is a list of (a, b) float32 arrays [N] (b is None where the term reads none)."""
    s = np.zeros_like(pairs[0][0], dtype=np.float32)
    for a, b in pairs:
        a = a.astype(np.float32)
        if kind == VALUE:
            g = a
        elif kind == ABS:
            g = np.abs(a)
        elif kind == SQUARE:
            g = a * a
        elif kind == DIFF_SQUARE:
            d = a - b.astype(np.float32)
            g = d * d
        else:
            g = np.abs(a * b.astype(np.float32))
        s = (s + g).astype(np.float32)
    return s


class Twin:
    """`metrics`: a list of (term, reduce, sqrt, include_done_step).  `step` takes the per-metric pair arrays of this step."""

    def __init__(self, metrics, nenvs, skip_running):
        self.metrics, self.n, m = list(metrics), nenvs, len(metrics)
        self.fin = np.zeros((m + 1, 5, nenvs), np.float64)
        self.run = np.zeros((m, nenvs), np.float32)
        self.count = np.zeros((m, nenvs), np.int32)
        self.steps = np.zeros(nenvs, np.int32)
        self.causes = np.zeros((CAUSES, nenvs), np.int32)
        self.armed = np.full(nenvs, 0 if skip_running else 1, np.uint8)

    def state(self) -> bytes:
        """The device state's bytes, array behind array."""
        return b"".join(a.tobytes() for a in (self.fin, self.run, self.count, self.steps, self.causes, self.armed))

    def _fold(self, m, mask, v):
        with np.errstate(invalid="ignore"):
            f = self.fin[m]
            first = f[F_N] == 0.0
            lo = np.where(first, v, np.where(v < f[F_MIN], v, f[F_MIN]))
            hi = np.where(first, v, np.where(v > f[F_MAX], v, f[F_MAX]))
            f[F_MIN] = np.where(mask, lo, f[F_MIN])
            f[F_MAX] = np.where(mask, hi, f[F_MAX])
            f[F_N] = np.where(mask, f[F_N] + 1.0, f[F_N])
            f[F_SUM] = np.where(mask, f[F_SUM] + v, f[F_SUM])
            f[F_SUMSQ] = np.where(mask, f[F_SUMSQ] + v * v, f[F_SUMSQ])

    def step(self, pairs_per_metric, dones, time_out, term_bits):
        """dones, time_out, term_bits: the three channels' values [N] as stored (converted by value here)."""
        done = as_f32(dones) != 0
        armed = self.armed != 0
        steps = self.steps + 1
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for m, ((kind, reduce, sqrt, incl), pairs) in enumerate(zip(self.metrics, pairs_per_metric)):
                s = term(kind, pairs)
                if reduce == LAST:
                    v = s.astype(np.float64)
                    self._fold(m, done & armed, np.sqrt(v) if sqrt else v)
                    continue
                sampled = ~done | bool(incl)
                run, count = self.run[m], self.count[m]
                if reduce == MAX:
                    new = np.where(count == 0, s, np.where(s > run, s, run))
                else:
                    new = (run + s).astype(np.float32)
                run = np.where(sampled, new, run).astype(np.float32)
                count = np.where(sampled, count + 1, count).astype(np.int32)
                v = run.astype(np.float64)
                if reduce == MEAN:
                    v = v / np.where(count > 0, count, 1).astype(np.float64)
                if sqrt:
                    v = np.sqrt(v)
                self._fold(m, done & armed & (count > 0), v)
                self.run[m] = np.where(done, np.float32(0), run)
                self.count[m] = np.where(done, 0, count)
        fin = done & armed
        self._fold(len(self.metrics), fin, steps.astype(np.float64))
        bits = as_f32(term_bits).astype(np.int64) & 0xFFFF
        for b in range(16):
            self.causes[b] += (fin & (((bits >> b) & 1) != 0)).astype(np.int32)
        self.causes[16] += (fin & (as_f32(time_out) != 0)).astype(np.int32)
        self.causes[17] += fin.astype(np.int32)
        self.steps = np.where(done, 0, steps).astype(np.int32)
        self.armed = np.where(done, 1, self.armed).astype(np.uint8)

    def restart_running(self, skip_running):
        self.run[:], self.count[:], self.steps[:] = 0, 0, 0
        self.armed[:] = 0 if skip_running else 1

    def clear_finished(self):
        self.fin[:] = 0
        self.causes[:] = 0

    def reduce(self):
        """(totals float64 [M + 1][5], causes int64 [18]) in the header's order."""
        n, rows = self.n, -(-self.n // THREADS)
        totals = np.zeros((len(self.metrics) + 1, 5), np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for m in range(len(self.metrics) + 1):
                part = np.zeros((5, THREADS), np.float64)
                for r in range(rows):  # thread t takes env r * 256 + t, in the order of r
                    k = min(THREADS, n - r * THREADS)
                    f = self.fin[m][:, r * THREADS:r * THREADS + k]
                    a = part[:, :k]
                    has, first = f[F_N] != 0.0, a[F_N] == 0.0
                    lo = np.where(first, f[F_MIN], np.where(f[F_MIN] < a[F_MIN], f[F_MIN], a[F_MIN]))
                    hi = np.where(first, f[F_MAX], np.where(f[F_MAX] > a[F_MAX], f[F_MAX], a[F_MAX]))
                    a[F_MIN], a[F_MAX] = np.where(has, lo, a[F_MIN]), np.where(has, hi, a[F_MAX])
                    a[F_N], a[F_SUM], a[F_SUMSQ] = a[F_N] + f[F_N], a[F_SUM] + f[F_SUM], a[F_SUMSQ] + f[F_SUMSQ]
                stride = THREADS // 2
                while stride >= 1:
                    a, b = part[:, :stride], part[:, stride:2 * stride].copy()
                    has, first = b[F_N] != 0.0, a[F_N] == 0.0
                    lo = np.where(first, b[F_MIN], np.where(b[F_MIN] < a[F_MIN], b[F_MIN], a[F_MIN]))
                    hi = np.where(first, b[F_MAX], np.where(b[F_MAX] > a[F_MAX], b[F_MAX], a[F_MAX]))
                    a[F_MIN], a[F_MAX] = np.where(has, lo, a[F_MIN]), np.where(has, hi, a[F_MAX])
                    a[F_N], a[F_SUM], a[F_SUMSQ] = a[F_N] + b[F_N], a[F_SUM] + b[F_SUM], a[F_SUMSQ] + b[F_SUMSQ]
                    stride //= 2
                totals[m] = part[:, 0]
        return totals, self.causes.astype(np.int64).sum(axis=1)

    def result(self) -> bytes:
        totals, causes = self.reduce()
        return totals.tobytes() + causes.tobytes()
