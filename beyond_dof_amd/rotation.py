"""How a solver's volume reaches the beam frame of an angle and how a rotated-frame gradient comes back: one class per way of
rotating, all with the same methods.  A solver picks one in its constructor (choose: host side, ValueError before anything is
allocated), hands it the device (allocate) and then calls it without asking which kind it is."""
import collections

import numpy as np

from . import util
from ._lib import DeviceBuffer

# a materialised kind: the host builder of its float64 rows per angle, their width, and its three libbdof entry points
Kind = collections.namedtuple('Kind', 'prm columns rotate set_object adjoint')
KINDS = {'bilinear': Kind(util.bilinear_prm, 4, 'bdof_rotate_bilinear', 'bdof_set_object_bilinear', 'bdof_rotate_bilinear_adjoint'),
         'trilinear': Kind(util.rigid_prm, 12, 'bdof_rotate_rigid', 'bdof_set_object_rigid', 'bdof_rotate_rigid_adjoint')}


def choose(rotation, shape, n_theta, coord_ls, theta, geometry, materialised=None):
    """shape = (Y, X, Z); geometry = (axis_tilt, axis_roll, center, rotation_matrices); materialised: the class for a kind of KINDS."""
    if rotation == 'nearest':
        return LookupRotation(shape, n_theta, coord_ls)
    return (materialised or MaterialisedRotation)(shape, n_theta, KINDS[rotation], KINDS[rotation].prm(n_theta, shape, theta, *geometry))


class LookupRotation(object):
    """rotation='nearest': the lookup tables (cnn_propagator/util.py:294-402), uploaded once and fused into the kernels."""
    one_pass_tail = float64_paths = True       # bdof_rotation_adjoint_adam and the models' float64 twins go through the tables

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


class MaterialisedRotation(LookupRotation):
    """rotation='bilinear' / 'trilinear' (KINDS), behind the same methods: the minibatch's rotated objects are written out at every
    step, straight into the ctx's modulation table, so no volume stays bound between steps; the adjoint is a gather with the same rows."""
    one_pass_tail = float64_paths = False

    def __init__(self, shape, n_theta, kind, prm):
        LookupRotation.__init__(self, shape, n_theta, None)
        self.kind, self.prm = kind, prm            # prm: (n_theta, kind.columns) float64

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
