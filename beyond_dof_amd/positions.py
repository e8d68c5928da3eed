"""Sub-pixel probe positions of ptychography and their refinement: the offsets a solver adds to probe_pos, the validation of the
keywords (host side, ValueError before anything is allocated) and a host Adam on them.

Offsets are in pixels in the order of probe_pos, (y, x), one pair per (angle, position).  refine_positions='per_angle' moves
every (angle, position) pair on its own; 'shared' moves one offset per position for all angles — the gradients of the angles that
list a position are added and every angle's offset of that position takes the same step.

Gauge: the mean offset is a translation of the object against the scan and is NOT removed; a volume that is reconstructed at the
same time absorbs it, and Adam's path decides the split."""
import numpy as np

from . import hostopt

MODES = (None, 'shared', 'per_angle')


def check_positions(position_offsets, refine_positions, n_pos, n_theta=None, propagator='fft', slice_binning=1, adjoint_precision=None,
                    n_batch_per_update=1):
    """The keywords position_offsets / refine_positions against what carries them: ValueError with the keyword's name, else
    the offsets as a float64 array (n_pos, 2) or (n_theta, n_pos, 2) (zeros when only refine_positions is set), or None when
    neither keyword is set (nothing of this runs).  n_theta=None: the first axis of a 3-D array is not checked."""
    if refine_positions not in MODES:
        raise ValueError("refine_positions must be None, 'shared' or 'per_angle', not {!r}".format(refine_positions))
    if position_offsets is None and refine_positions is None:
        return None
    name = 'position_offsets' if refine_positions is None else 'refine_positions'
    if propagator == 'conv':
        raise ValueError("{} runs with the transfer-function propagator: not together with propagator='conv'".format(name))
    if int(slice_binning) > 1:
        raise ValueError('{} reads the window stack slice by slice: not together with slice_binning > 1'.format(name))
    if adjoint_precision not in (None, 'float32'):
        raise ValueError("{} runs the float32 sweeps: not together with adjoint_precision={!r}".format(name, adjoint_precision))
    if refine_positions is not None and int(n_batch_per_update) > 1:
        raise ValueError('refine_positions moves the positions at every minibatch: not together with n_batch_per_update > 1')
    if position_offsets is None:
        return np.zeros((int(n_pos), 2))
    off = np.array(position_offsets, dtype=np.float64)
    ok = off.shape == (int(n_pos), 2) or (off.ndim == 3 and off.shape[1:] == (int(n_pos), 2) and (n_theta is None or off.shape[0] == int(n_theta)))
    if not ok:
        raise ValueError('position_offsets must be (n_pos, 2) or (n_theta, n_pos, 2) = ({}{}, 2) in the order of probe_pos (y, x), not {}'.format(
            '' if n_theta is None else '{}, '.format(int(n_theta)), int(n_pos), off.shape))
    if not np.all(np.isfinite(off)):
        raise ValueError('position_offsets must be finite')
    return off


def to_level(offsets, ds_level):
    """full-resolution offsets in the pixels of multiscale level ds_level (the levels are strided: pixel i of a level is pixel
    i * ds_level of the full resolution)"""
    return np.asarray(offsets, dtype=np.float64) / ds_level


def from_level(offsets, ds_level):
    return np.asarray(offsets, dtype=np.float64) * ds_level


class ProbePositions(object):
    """The offsets (n_theta, n_pos, 2) of a solver, the mode and, when refining, a host Adam (0.9 / 0.999 / 1e-8) whose step
    `rate` is in pixels.  An entry — a position under 'shared', an (angle, position) pair under 'per_angle' — keeps its own
    update counter and moves only in a step that lists it."""

    def __init__(self, n_theta, n_pos, offsets=None, mode=None, rate=0.05):
        if mode not in MODES:
            raise ValueError("refine_positions must be None, 'shared' or 'per_angle', not {!r}".format(mode))
        self.n_theta, self.n_pos, self.mode, self.rate = int(n_theta), int(n_pos), mode, float(rate)
        off = np.zeros((self.n_pos, 2)) if offsets is None else np.asarray(offsets, dtype=np.float64)
        self.offset = np.array(np.broadcast_to(off, (self.n_theta, self.n_pos, 2)), dtype=np.float64)
        self.shape = (self.n_pos, 2) if mode == 'shared' else (self.n_theta, self.n_pos, 2)
        self.opt = hostopt.MaskedAdam(self.shape, self.rate)
        self.m, self.v, self.t = self.opt.m, self.opt.v, self.opt.t           # (the optimiser's own arrays)

    @property
    def refine(self):
        return self.mode is not None

    def values(self):
        return self.offset.copy()

    def of(self, i_theta, pos_idx):
        """the (len(pos_idx), 2) offsets (y, x) of positions pos_idx at angle i_theta"""
        return self.offset[int(i_theta), np.asarray(pos_idx)]

    def dense(self, grad, i_theta, pos_idx):
        """one vector for the ranks to add: the gradient (len(pos_idx), 2) scattered over the entries (a position listed twice
        adds), then which entries it lists"""
        at = (np.asarray(pos_idx),) if self.mode == 'shared' else (np.full(len(pos_idx), int(i_theta)), np.asarray(pos_idx))
        return hostopt.pack(self.shape[:-1], at, [grad], [self.shape])

    def split(self, dense):
        """dense()'s vector -> (gradient, listed) in the entries' shape"""
        g, move = hostopt.unpack(dense, self.shape[:-1], [self.shape])[0]
        return g, move[..., 0]

    def update(self, dense):
        """Adam on the listed entries from dense()'s vector (already summed over the ranks and divided by their number)"""
        g, move = hostopt.unpack(dense, self.shape[:-1], [self.shape])[0]
        self.offset = self.opt.step(self.offset, g, move)      # ('shared': (n_pos, 2) against (n_theta, n_pos, 2) — every angle takes the step)


def summary_line(start, end):
    """the refined_positions line of summary.txt: rms and largest move of the offsets, in full-resolution pixels"""
    move = np.sqrt(np.sum((np.asarray(end) - np.asarray(start)) ** 2, axis=-1))
    return '{:<20}rms move {:.6g} px, largest move {:.6g} px over {} offsets\n'.format(
        'refined_positions', float(np.sqrt(np.mean(move ** 2))), float(move.max()), move.size)
