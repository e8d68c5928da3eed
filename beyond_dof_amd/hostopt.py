"""The optimisers that run on the host, in float64, on the few numbers a step refines beside the volume: one masked Adam
(0.9 / 0.999 / 1e-8) for the geometry (rotation.RigidGeometry) and the probe positions (positions.ProbePositions), the vector
their gradients cross the ranks in, and the probe with its complex Adam (the solvers' enable_probe_optimization)."""
import numpy as np

B1, B2, EPS = 0.9, 0.999, 1e-8


class MaskedAdam(object):
    """Adam on a real float64 array of any shape: m, v, a step counter t per entry, and the step `rate` (a scalar, or an
    array that broadcasts).  An entry advances only in a step whose `move` lists it."""

    def __init__(self, shape, rate):
        self.m, self.v, self.t, self.rate = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64), rate

    def step(self, value, g, move):
        """value after one step with gradient g: where move (bool, broadcasts against the entries) is set t, m, v and the value
        advance; elsewhere all four stay.  value may carry leading axes over the entries: every one of them takes the step."""
        self.t += move                           # (in place: whoever holds m, v, t sees them move)
        self.m[...] = np.where(move, B1 * self.m + (1 - B1) * g, self.m)
        self.v[...] = np.where(move, B2 * self.v + (1 - B2) * g * g, self.v)
        t = np.maximum(self.t, 1)
        step = self.rate * (self.m / (1 - B1 ** t)) / (np.sqrt(self.v / (1 - B2 ** t)) + EPS)
        return np.where(move, value - step, value)


def pack(listed_shape, at, grads, shapes):
    """One vector for the ranks to add: every gradient of `grads` scattered at the entries `at` (an index tuple; an entry listed
    twice adds) over zeros of its shape in `shapes` — a shape () takes its gradient as it is — then 0 / 1 over listed_shape, 1 at `at`."""
    parts = [np.zeros(shape) for shape in shapes] + [np.zeros(listed_shape)]
    for full, g in zip(parts, grads):
        np.add.at(full, at if full.ndim else (), np.asarray(g, dtype=np.float64))
    parts[-1][at] = 1.
    return np.concatenate([part.reshape(-1) for part in parts])


def unpack(dense, listed_shape, shapes):
    """pack's vector (summed over the ranks) -> [(gradient, move)] per shape, move being the listed entries with trailing axes of
    length 1 up to the gradient's rank (MaskedAdam.step broadcasts it); a shape () always moves."""
    *grads, listed = np.split(dense, np.cumsum([int(np.prod(shape, dtype=int)) for shape in shapes]))
    listed = listed.reshape(listed_shape) > 0
    return [(g.reshape(shape), listed.reshape(listed.shape + (1,) * (len(shape) - listed.ndim)) if shape else np.True_)
            for g, shape in zip(grads, shapes)]


class ProbeVariable(object):
    """The optimisable probe, (Y, X) complex128 — or (M, Y, X) probe modes, each with its own moments and one step counter: Adam on
    (real, imag) written in complex arithmetic, the pupil that multiplies every mode after a step, and the count of minibatches whose
    gradient the engine's device accumulator holds."""

    def __init__(self, probe, rate, pupil=None):
        self.rate = float(rate)
        self.pupil = None if pupil is None else np.asarray(pupil, dtype=np.float64)
        self.grad, self.n_acc = None, 0            # the engine's device accumulator of the gradient, minibatches in it
        self.restart(probe)

    def restart(self, probe):
        """a new probe; the moments and the step counter start again"""
        self.probe = probe
        self.probe_m, self.probe_v, self.probe_t = np.zeros_like(probe), np.zeros_like(probe), 0

    def get(self):
        return self.probe.real.copy(), self.probe.imag.copy()

    def to_engine(self, eng):
        (eng.set_probe_modes if self.probe.ndim == 3 else eng.set_probe)(self.probe.real, self.probe.imag)

    def collect(self, eng):
        """add the probe gradient of the engine's last loss + gradient to the device accumulator"""
        self.grad = eng.probe_grad(accumulate=self.n_acc > 0, to_host=False)
        self.n_acc += 1

    def apply(self, rank_mean, b1=B1, b2=B2, eps=EPS):
        """Adam with the accumulated gradient: its mean over the accumulated minibatches, then rank_mean's over the ranks"""
        g = np.ascontiguousarray(np.swapaxes(self.grad.download(), -2, -1)).astype(np.complex128) / self.n_acc
        self.n_acc = 0
        g = rank_mean(g)
        self.probe_t += 1
        self.probe_m = b1 * self.probe_m + (1 - b1) * g
        self.probe_v = b2 * self.probe_v + (1 - b2) * (g.real ** 2 + 1j * g.imag ** 2)
        mh = self.probe_m / (1 - b1 ** self.probe_t)
        vh = self.probe_v / (1 - b2 ** self.probe_t)
        self.probe = self.probe - self.rate * (mh.real / (np.sqrt(vh.real) + eps) + 1j * mh.imag / (np.sqrt(vh.imag) + eps))
        if self.pupil is not None:
            self.probe = self.probe * self.pupil
