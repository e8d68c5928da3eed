"""How a solver's volume reaches the beam frame of an angle and how a rotated-frame gradient comes back: one class per way of
rotating, all with the same methods.  A solver picks one in its constructor (choose: host side, ValueError before anything is
allocated), hands it the device (allocate) and then calls it without asking which kind it is."""
import collections

import numpy as np

from . import hostopt, util
from ._lib import DeviceBuffer

# a materialised kind: the host builder of its float64 rows per angle, their width, and its three libbdof entry points
Kind = collections.namedtuple('Kind', 'prm columns rotate set_object adjoint')
KINDS = {'bilinear': Kind(util.bilinear_prm, 4, 'bdof_rotate_bilinear', 'bdof_set_object_bilinear', 'bdof_rotate_bilinear_adjoint'),
         'trilinear': Kind(util.rigid_prm, 12, 'bdof_rotate_rigid', 'bdof_set_object_rigid', 'bdof_rotate_rigid_adjoint')}


def choose(rotation, shape, n_theta, coord_ls, theta, geometry, materialised=None, refine=(), rate=0.05):
    """shape = (Y, X, Z); geometry = (axis_tilt, axis_roll, center, rotation_matrices); materialised: the class for a kind of KINDS.
    refine, rate: the solvers' refine_geometry and geometry_learning_rate (RigidGeometry; ValueError for what cannot be refined)."""
    refine = check_refine(refine, rotation, geometry[3])
    if rotation == 'nearest':
        return LookupRotation(shape, n_theta, coord_ls)
    rot = (materialised or MaterialisedRotation)(shape, n_theta, KINDS[rotation], KINDS[rotation].prm(n_theta, shape, theta, *geometry))
    if rotation == 'trilinear' and geometry[3] is None:
        rot.geometry = RigidGeometry(shape, theta, geometry[0], geometry[1], geometry[2], refine, rate)
    return rot


def check_refine(refine, rotation, rotation_matrices):
    """A solver's refine_geometry as a tuple of names of util.GEOMETRY_NAMES; ValueError for an unknown name, for a rotation
    other than 'trilinear' and for raw rotation_matrices (which refinement could not keep rigid)."""
    refine = (refine,) if isinstance(refine, str) else tuple(refine or ())
    unknown = [n for n in refine if n not in util.GEOMETRY_NAMES]
    if unknown:
        raise ValueError('refine_geometry takes names out of {}, not {}'.format(util.GEOMETRY_NAMES, unknown))
    if refine and rotation != 'trilinear':
        raise ValueError("refine_geometry runs with rotation='trilinear' only")
    if refine and rotation_matrices is not None:
        raise ValueError('refine_geometry moves center, axis_tilt, axis_roll, theta and shifts: not together with rotation_matrices')
    return refine


class RigidGeometry(object):
    """The numbers util.rigid_geometry builds rotation='trilinear' from, the chain rule from dL/d(M | t) back to them and, for
    the names in `refine`, a host Adam (0.9 / 0.999 / 1e-8) on them.  rate: Adam's step as a displacement in pixels at the
    volume's edge — center and shifts take it as it is, the three angles rate / (max(X, Z, Y) / 2).  A per-angle entry (theta,
    shifts) keeps its own update counter and moves only in a step that lists its angle.
    Gauge: the mean horizontal shift and center move the same rows, the mean vertical shift is a translation of the volume
    along y; refining both members of a pair leaves their split to Adam's path."""

    def __init__(self, shape, theta, axis_tilt, axis_roll, center, refine=(), rate=0.05):
        self.shape = tuple(int(a) for a in shape)
        n = len(np.atleast_1d(theta))
        self.value = dict(center=np.array((self.shape[1] - 1) / 2. if center is None else float(center)), axis_tilt=np.array(float(axis_tilt)),
                          axis_roll=np.array(float(axis_roll)), theta=np.array(np.atleast_1d(theta), dtype=np.float64), shifts=np.zeros((n, 2)))
        self.refine, self.n_theta = tuple(refine), n
        self.rate = {k: float(rate) / (1. if k in ('center', 'shifts') else max(self.shape) / 2.) for k in util.GEOMETRY_NAMES}
        self.opt = {k: hostopt.MaskedAdam(self.value[k].shape, self.rate[k]) for k in self.refine}
        self.shapes = [self.value[k].shape for k in self.refine]
        self.m, self.v, self.t = [{k: getattr(o, a) for k, o in self.opt.items()} for a in 'mvt']     # (the optimisers' own arrays)

    def values(self):
        return {k: v.copy() for k, v in self.value.items()}

    def set_values(self, **values):
        for k, v in values.items():
            self.value[k] = np.array(v, dtype=np.float64).reshape(self.value[k].shape)

    def prm(self):
        g = self.value
        return util.rigid_geometry(g['theta'], self.shape, float(g['axis_tilt']), float(g['axis_roll']), float(g['center']), g['shifts'])

    def gradient(self, dprm, index):
        """dL/d(M | t) rows (len(index), 3, 4) of the angles index -> util.rigid_geometry_gradient's dict"""
        g = self.value
        return util.rigid_geometry_gradient(g['theta'], self.shape, float(g['axis_tilt']), float(g['axis_roll']), float(g['center']), g['shifts'],
                                            np.reshape(dprm, (len(index), 12)), index)

    def dense(self, grad, index):
        """one vector for the ranks to add (hostopt.pack): per refined name its gradient scattered over all angles, then which angles it lists"""
        return hostopt.pack((self.n_theta,), (np.asarray(index),), [grad[k] for k in self.refine], self.shapes)

    def update(self, dense):
        """Adam on the refined names from dense()'s vector (already summed over the ranks and divided by their number)"""
        for k, (g, move) in zip(self.refine, hostopt.unpack(dense, (self.n_theta,), self.shapes)):
            self.value[k] = self.opt[k].step(self.value[k], g, move)


class LookupRotation(object):
    """rotation='nearest': the lookup tables (cnn_propagator/util.py:294-402), uploaded once and fused into the kernels."""
    one_pass_tail = float64_paths = True       # bdof_rotation_adjoint_adam and the models' float64 twins go through the tables
    geometry = None            # only rotation='trilinear' from theta and the axis keywords has one: its RigidGeometry (choose)

    def __init__(self, shape, n_theta, coord_ls):
        self.dim_y, self.dim_x, self.dim_z = [int(s) for s in shape]
        self.n_theta, self.coord_ls = int(n_theta), coord_ls

    def allocate(self, ctx, mb):
        self.ctx, self.mb = ctx, int(mb)
        coord_ls = self.coord_ls
        if coord_ls is None:
            coord_ls = util.rotation_lookup([self.dim_y, self.dim_x, self.dim_z], self.n_theta)
        tables = util.device_rotation_tables(coord_ls, self.dim_x, self.dim_z)
        self.tab, self.off, self.order = [DeviceBuffer.from_host(ctx, t) for t in tables]

    def bind_volume(self, eng, x):
        """the volume memory x is (again) what the engine's sweeps read"""
        eng.set_volume(x, self.dim_x * self.dim_z, self.dim_y, self.tab, self.dim_x, self.n_theta)

    def attach(self, eng):
        """once: the inverse tables of the rotation adjoint inside the library"""
        eng.set_rotation_adjoint(self.off, self.order, self.dim_x * self.dim_z)

    def stage_angles(self, idx):
        """the angles idx are the ones the next adjoint takes"""

    def stage(self, eng, x, idx, B, conv):
        """stage_angles, and the B rotated objects of the volume x are what the next sweep reads"""

    def angle_arg(self, a):
        """what loss_grad_device and forward take as their angle argument, given the indices a"""
        return a

    def adjoint(self, angles, g, x0, nx, accumulate):
        """full field: the rotated-frame gradient in the ctx into x-planes [x0, x0 + nx) of g"""
        lib, h = self.ctx.lib, self.ctx.handle
        self.ctx.check(lib.bdof_rotation_adjoint_rows(h, self.mb, angles.ptr, g.ptr, x0 * self.dim_z, nx * self.dim_z, int(accumulate), 1.0))

    def window_angle(self, i_theta):
        """ptychography: the angle index the window kernels see"""
        return i_theta

    def window_adjoint(self, i_theta, xo, yo, g):
        """ptychography: the window gradients in the ctx into the volume gradient g"""
        self.ctx.check(self.ctx.lib.bdof_window_rotation_adjoint(self.ctx.handle, self.mb, i_theta, xo, yo, g.ptr, 0, 1.0))

    def window_source(self, x, i_theta):
        """ptychography at fractional positions: (rows, table of the step's angle) bdof_window_stack gathers from — device addresses"""
        return x.ptr, self.tab.ptr + int(i_theta) * self.dim_z * self.dim_x * 4

    def window_stack_adjoint(self, i_theta, origin, g):
        """... and the window gradients in the ctx, cut at the origins `origin`, into the volume gradient g"""
        self.ctx.check(self.ctx.lib.bdof_window_stack_adjoint(self.ctx.handle, None, int(i_theta), origin.ptr, self.mb, g.ptr, 0, 1.0))


class MaterialisedRotation(LookupRotation):
    """rotation='bilinear' / 'trilinear' (KINDS), behind the same methods: the minibatch's rotated objects are written out at every
    step, straight into the ctx's modulation table, so no volume stays bound between steps; the adjoint is a gather with the same rows."""
    one_pass_tail = float64_paths = False

    def __init__(self, shape, n_theta, kind, prm):
        LookupRotation.__init__(self, shape, n_theta, None)
        self.kind, self.prm = kind, prm            # prm: (n_theta, kind.columns) float64
        self.dprm_buf = None

    def allocate(self, ctx, mb):
        self.ctx, self.mb = ctx, int(mb)
        self.prm_buf = DeviceBuffer(ctx, self.mb * self.kind.columns * 8, np.float64, (self.mb, self.kind.columns))

    def bind_volume(self, eng, x):
        pass

    def attach(self, eng):
        pass

    def stage_angles(self, idx):
        prm = np.zeros(self.prm_buf.shape)
        prm[:len(idx)] = self.prm[np.asarray(idx)]
        self.prm_buf.upload(prm)

    def _call(self, name, first, *last):
        self.ctx.check(getattr(self.ctx.lib, name)(self.ctx.handle, first, self.dim_x, self.dim_z, self.dim_y, self.prm_buf.ptr, *last))

    def stage(self, eng, x, idx, B, conv):
        self.stage_angles(idx)
        self._call(self.kind.set_object, x.ptr, B, int(conv))

    def angle_arg(self, a):
        return None

    def adjoint(self, angles, g, x0, nx, accumulate, grot=None):
        """grot: the rotated-frame gradient (None: the ctx's own, bdof_grot)"""
        grot = self.ctx.lib.bdof_grot(self.ctx.handle) if grot is None else grot.ptr
        self._call(self.kind.adjoint, grot, self.mb, g.ptr, x0 * self.dim_z, nx * self.dim_z, int(accumulate), 1.0)

    def param_gradient(self, x, grot=None):
        """dL/d(M | t) of the staged angles, (B, 3, 4) float64 on the host (bdof_rotate_rigid_param_grad): x the volume that was
        staged, grot the rotated-frame gradient (None: the ctx's own).  The download waits for the stream."""
        if self.kind is not KINDS['trilinear']:
            raise ValueError("param_gradient: rotation='trilinear' only")
        if self.dprm_buf is None:
            self.dprm_buf = DeviceBuffer(self.ctx, self.mb * 12 * 8, np.float64, (self.mb, 3, 4))
        lib, h = self.ctx.lib, self.ctx.handle
        self.ctx.check(lib.bdof_rotate_rigid_param_grad(h, x.ptr, None if grot is None else grot.ptr, self.dim_x, self.dim_z, self.dim_y,
                                                        self.prm_buf.ptr, self.mb, self.dprm_buf.ptr, 0))
        self.ctx.sync()
        return self.dprm_buf.download()


class RotatedCopy(MaterialisedRotation):
    """PtychoSolver's materialised rotation.  A minibatch has one angle, so per step the volume is rotated once into a plain
    (delta, beta) copy (B = 1) that is bound under a one-angle identity table: the windows run with angle 0 on whichever engine
    and precision was chosen, the window adjoint fills a rotated-frame gradient through the identity's inverse tables and the
    kind's adjoint takes it into the volume's."""

    def allocate(self, ctx, mb):
        MaterialisedRotation.allocate(self, ctx, 1)
        self.n_windows = int(mb)
        # the rotated copy [z][x][y] and its gradient, and the identity tables of one angle: rotated row (z, x) is row z X + x
        n_rows = self.dim_z * self.dim_x
        self.copy = DeviceBuffer.zeros(ctx, (self.dim_z, self.dim_x, self.dim_y, 2), np.float32)
        self.g_rot = DeviceBuffer.zeros(ctx, (self.dim_z, self.dim_x, self.dim_y, 2), np.float32)
        self.tab = DeviceBuffer.from_host(ctx, np.arange(n_rows, dtype=np.int32).reshape(1, self.dim_z, self.dim_x))
        self.off = DeviceBuffer.from_host(ctx, np.arange(n_rows + 1, dtype=np.int32).reshape(1, -1))
        self.order = DeviceBuffer.from_host(ctx, np.arange(n_rows, dtype=np.int32).reshape(1, -1))

    attach = LookupRotation.attach

    def stage(self, eng, x, idx, B, conv):
        self.stage_angles(idx)
        self._call(self.kind.rotate, x.ptr, 1, self.copy.ptr)
        eng.set_volume(self.copy, self.dim_z * self.dim_x, self.dim_y, self.tab, self.dim_x, 1)     # (again: that memory has changed)

    def window_angle(self, i_theta):
        return 0

    def window_adjoint(self, i_theta, xo, yo, g):
        """windows -> rotated frame (identity tables) -> volume frame (prm_buf still holds the step's angle)"""
        self.ctx.check(self.ctx.lib.bdof_window_rotation_adjoint(self.ctx.handle, self.n_windows, 0, xo, yo, self.g_rot.ptr, 0, 1.0))
        self.adjoint(None, g, 0, self.dim_x, 0, grot=self.g_rot)

    def param_gradient(self, x, grot=None):
        return MaterialisedRotation.param_gradient(self, x, self.g_rot if grot is None else grot)

    def window_source(self, x, i_theta):
        return self.copy.ptr, self.tab.ptr

    def window_stack_adjoint(self, i_theta, origin, g):
        self.ctx.check(self.ctx.lib.bdof_window_stack_adjoint(self.ctx.handle, None, 0, origin.ptr, self.n_windows, self.g_rot.ptr, 0, 1.0))
        self.adjoint(None, g, 0, self.dim_x, 0, grot=self.g_rot)
