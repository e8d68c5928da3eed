"""Device-resident state of a reconstruction: the (delta, beta) volume, its Adam moments, the rotation tables and the
measured amplitudes, plus the Adam iteration built from libbdof calls.  This is the loop body of
cnn_propagator/fullfield.py:340-362 and ptychography.py:285-310 with every array kept in HBM.

One Adam iteration (`step`):
    forward + adjoint sweeps of this rank's wavefields                     bdof_loss_grad
    then, pipelined over x-slabs of the [X][Z][Y] volume (the "tail"):
      rotation adjoint of slab c                                          bdof_rotation_adjoint_rows
      gradient exchange of slab c across ranks                            bdof_reduce_scatter_grad | bdof_allreduce_grad
      regulariser + Adam + mask + clip on slab c (sharded: on this rank's 1/N of it)   bdof_adam_step_slab
      sharded: all-gather of the updated slab                             bdof_allgather_volume
    On one rank with the lookup-table rotation there is nothing between the rotation adjoint and Adam, and FullfieldSolver.step
    runs the tail as one pass over the volume that also leaves the new volume's modulation table   bdof_rotation_adjoint_adam
The collectives run on the communicator's stream; the ctx stream only waits for slab c two slabs later, so the producer
of the next slabs and the consumer of the previous ones run while a slab is on the wire.  The TV stencil reads the
pre-update volume (x_old), which no slab overwrites: slab-wise, sharded and whole-volume execution give identical results.
"""
import collections
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import DeviceBuffer
from . import analytic
from . import rotation as rotations
from . import positions as probe_positions
from . import modes as probe_modes
from . import util
from .comm import PseudoComm
from .engine import MultisliceEngine, RESIDENT_SIZES, check_model_options
from .hostopt import ProbeVariable

# one update of the volume as the tail takes it: bias-correction exponent, step, regulariser (_VolumeSolver.regularizer), clip to >= 0, mask
Update = collections.namedtuple('Update', 'i_update learning_rate alpha_d alpha_b gamma clip use_mask', defaults=(0.0, 0.0, 0.0, True, True))


def _check_options(propagator, adjoint64, *options, **path):
    """check_model_options with a solver's keywords: any adjoint64 that is on stands for the float64 path."""
    return check_model_options(*options, propagator=propagator, adjoint_precision='float64' if adjoint64 else None, **path)


class _VolumeSolver(object):
    """What the full-field and ptychography solvers share: volume double buffer, gradient, moments, the tail of the step."""

    lookahead = 2              # slabs in flight between a collective's start and the Adam pass that consumes it
    n_modes = 0                # probe modes (PtychoSolver with (M, py, px) probes)

    def _float64_paths(self, adjoint64, propagator):
        """adjoint64, propagator -> self.conv, self.f64 and (returned) the engine's adjoint64, its float64 adjoint sweep (transfer-function
        model).  f64 = 'first': the FIRST minibatch of every epoch runs through the model's float64 path on the same context (bdof_loss_grad_tf_f64
        / _conv_f64: whole sweeps in double) — Adam's first step after a restart is lr g / (|g| + 1e-8), the only one in which a 1e-8 error of
        the gradient moves a voxel by a fraction of a whole step; True: every minibatch (real-space model, which has no such sweep)."""
        if adjoint64 not in (None, False, True, 'first'):
            raise ValueError("adjoint64 must be None, False, True or 'first'")
        self.conv = propagator == 'conv'
        self.f64 = 'first' if adjoint64 == 'first' else (True if (adjoint64 is True and self.conv) else None)
        return adjoint64 is True and not self.conv

    def _set_up(self, energy_ev, psize_cm, kernel_size, loss, detector_weights, probe_real, probe_imag, **physics):
        """The constructors' common tail, once self.eng and self.rot exist: the engine's model (loss: set_loss's arguments, physics:
        set_physics' keywords), the float64 twin, then the buffers of the rotation, the volume and (_batch_buffers) the staged minibatch."""
        self.ctx = self.eng.ctx
        self.eng.set_loss(*loss)
        self.eng.set_physics(energy_ev, psize_cm, **physics)
        self.eng.set_detector_weights(detector_weights)
        if self.conv:
            self.eng.set_conv(energy_ev, psize_cm, kernel_size)
        (self.eng.set_probe_modes if np.ndim(probe_real) == 3 else self.eng.set_probe)(probe_real, probe_imag)
        if self.f64:
            self._enable_f64()
        self.rot.allocate(self.ctx, self.mb)
        self._init_volume()
        self._batch_buffers()
        self._bind_volume()
        self.rot.attach(self.eng)

    def _init_volume(self):
        shape = (self.dim_x, self.dim_z, self.dim_y, 2)
        self.x = [DeviceBuffer.zeros(self.ctx, shape, np.float32), DeviceBuffer.zeros(self.ctx, shape, np.float32)]
        self.cur = 0
        self.g, self.m, self.v = [DeviceBuffer.zeros(self.ctx, shape, np.float32) for _ in range(3)]
        self.mask = None
        self.nvox = self.dim_x * self.dim_z * self.dim_y
        self._plan = self.tuned = None
        self._acc = 0              # minibatches accumulated in self.g since the last update (n_batch_per_update)
        self._epoch_plan = None    # shard layout of the Adam moments since the last reset_moments (None: none taken yet)
        self._g_shards = None      # slabs whose gradient is reduced on this rank's 1/size only (after a sharded step)
        self._g_stale = False      # the last step ran the one-pass tail, which does not write self.g (_g_refresh)
        self.pvar = None           # enable_probe_optimization: the probe as a variable (hostopt.ProbeVariable)
        self.meas = None           # FullfieldSolver.set_measurements
        self.meas_all = None       # PtychoSolver.set_measurements
        # what a staged minibatch leaves behind, written by the staging functions only (_rot_loss_grad; _win_loss_grad, _stack_windows)
        self._angles = None        # its angles, int64 (ptychography: the one)
        self._last = None          # ptychography: (i_theta, xo, yo), xo / yo the device addresses of its window origins
        self._last_pos = None      # ... at fractional positions: (i_theta, pos_idx) of the windows the window gradient belongs to
        self._source = None        # ... and the (rows, table) they were cut from, device addresses (rotation's window_source)
        self.comm.attach(self.ctx)

    def _bind_volume(self):
        self.rot.bind_volume(self.eng, self.x[self.cur])

    # ---- the streaming engine's fused forward sweep (MultisliceEngine.set_sweep_fusion) ---------
    def set_sweep_fusion(self, mode):
        self.eng.set_sweep_fusion(mode)

    @property
    def sweep_fused(self):
        """The mode the last loss + gradient actually ran (0: the two-kernel sweep)."""
        return self.eng.sweep_fused

    def set_adjoint_fusion(self, on=True):
        self.eng.set_adjoint_fusion(on)

    @property
    def adjoint_fused(self):
        """1 if the last loss + gradient ran the fused adjoint sweep."""
        return self.eng.adjoint_fused

    # ---- state -------------------------------------------------------------------------------
    def set_volume(self, obj_delta, obj_beta):
        self.x[self.cur].upload(util.volume_to_rows(obj_delta, obj_beta))
        self._bind_volume()

    def get_volume(self):
        self.ctx.sync()
        return util.rows_to_volume(self.x[self.cur].download())

    def set_mask(self, mask):
        self.mask = None if mask is None else DeviceBuffer.from_host(
            self.ctx, np.ascontiguousarray(np.asarray(mask, dtype=np.float32).transpose(1, 2, 0)))

    def reset_moments(self):
        """m, v = (None, None) at the start of every epoch (fullfield.py:338, quirk Q10)."""
        lib, h = self.ctx.lib, self.ctx.handle
        self.ctx.check(lib.bdof_memset(h, self.m.ptr, 0, self.m.nbytes))
        self.ctx.check(lib.bdof_memset(h, self.v.ptr, 0, self.v.nbytes))
        self._acc = 0
        self._epoch_plan = None

    def bcast_volume(self, root=0):
        """Rank `root`'s volume to every rank (the init_*_temp.npy hand-over of ptychography.py:169-208)."""
        if self.comm.size > 1:
            self.comm.bcast_device(self.ctx, self.x[self.cur], root)
            self._bind_volume()

    def _get_loss(self):
        return self.eng.get_loss()

    def _enable_f64(self):
        """Bind the model's float64 twin in the constructor: it allocates the float64 wave + tape for the minibatch, so a run
        fails here, not mid-way; a probe the float64 path does not take is the caller's to decide about (BdofError)."""
        try:
            (self.eng.enable_conv_f64 if self.conv else self.eng.enable_tf_f64)()
        except ValueError as err:
            raise _lib.BdofError(str(err))

    def _g_is_local(self):
        """self.g is about to be rewritten whole with this rank's own, unreduced gradient: the shard layout a sharded step
        left behind no longer describes it (gradient_to_host would otherwise gather stale parts over it)."""
        self._g_shards = None
        self._g_stale = False

    def _g_refresh(self):
        """After a one-pass tail self.g was not written: the rotation adjoint of the rotated-frame gradient, which stays in the
        ctx until the next gradient sweep, with the scale the step used — the bits the separate kernels would have left."""
        if self._g_stale:
            self._produce()(0, self.dim_x)
            self._g_stale = False

    def gradient_to_host(self):
        """The gradient of the last step / loss_and_grad as (g_delta, g_beta), each (Y, X, Z).  After a sharded step every rank
        holds the reduced gradient of its own 1/size of each slab only: the parts are gathered first — the call is then a
        COLLECTIVE, every rank must make it.  After loss_and_grad (or a step in the all-reduce form) it is a local read-back."""
        if self._g_shards:
            per_x = self.dim_z * self.dim_y * 2
            for x0, nx in self._g_shards:
                self.comm.wait(self.ctx, self.comm.start_allgather(self.ctx, self.g, x0 * per_x, (nx // self.comm.size) * per_x))
            self._g_shards = None
        self._g_refresh()
        self.ctx.sync()
        return util.rows_to_volume(self.g.download())

    # ---- the geometry of rotation='trilinear' (rotation.RigidGeometry) --------------------------------------------------------
    def _rigid_geometry(self):
        if self.rot.geometry is None:
            raise ValueError("the geometry is that of rotation='trilinear' built from theta and the axis keywords (not rotation_matrices)")
        return self.rot.geometry

    def geometry(self):
        """The current center, axis_tilt, axis_roll, theta (n_theta) and shifts (n_theta, 2): what refine_geometry has made of them."""
        return self._rigid_geometry().values()

    def set_geometry(self, **values):
        """Replace values of geometry() (center, axis_tilt, axis_roll, theta, shifts): the next stage rotates with them."""
        geo = self._rigid_geometry()
        geo.set_values(**values)
        self.rot.prm = geo.prm()

    def geometry_gradient(self):
        """dL/d(center, axis_tilt, axis_roll, theta_i, shift_i) of the data term for the angles of the last loss_and_grad (or, inside
        step, of the step, before the tail flips the volume), not reduced over the ranks: the dict of util.rigid_geometry_gradient,
        its per-angle entries in the order of those angles.  One reduction on the device over the volume that was staged, the
        staged rows and the rotated-frame gradient (bdof_rotate_rigid_param_grad), then the chain rule on the host."""
        geo, index = self._rigid_geometry(), self._step_angles()
        if index is None:
            raise RuntimeError('geometry_gradient() follows loss_and_grad() or runs inside step(): no angles have been staged yet')
        return geo.gradient(self.rot.param_gradient(self.x[self.cur])[:len(index)], index)

    def _step_angles(self):
        return self._angles

    def _rank_mean(self, a):
        """a host array summed over the ranks and divided by their number (grads /= size, as the volume gradient)"""
        return self.comm.allreduce_sum_host(a) / self.comm.size if self.comm.size > 1 else a

    def _refine(self, variable, gradient, *where):
        """step, before the tail, for a variable with a host Adam (rotation.RigidGeometry, positions.ProbePositions) that is being
        refined: its gradient() at the entries `where` of the minibatch, the mean over the ranks, the variable's Adam.  True: it moved."""
        if variable is None or not variable.refine:
            return False
        variable.update(self._rank_mean(variable.dense(gradient(), *where)))
        return True

    def _refine_geometry(self):
        if self._refine(self.rot.geometry, self.geometry_gradient, self._angles):
            self.rot.prm = self.rot.geometry.prm()           # new rows for the next stage

    def regularizer(self, alpha_d=0.0, alpha_b=0.0, gamma=0.0):
        """alpha_d sum|delta| + alpha_b sum|beta| + gamma TV(delta) of the current volume (fullfield.py:109-118), on the device."""
        sums = (ctypes.c_double * 3)()
        self.ctx.check(self.ctx.lib.bdof_regularizer_value(self.ctx.handle, self.x[self.cur].ptr, self.dim_x, self.dim_z, self.dim_y, sums))
        return alpha_d * sums[0] + alpha_b * sums[1] + gamma * sums[2]

    def shell_correlation(self, other, psize_cm=None):
        """Fourier shell correlation (resolution.fourier_shell_correlation) of the resident volume with another solver's resident
        volume, or with a host (delta, beta) pair in (y, x, z) order: nothing comes back from the device but the shell sums."""
        from . import resolution
        mine = self.x[self.cur]
        if isinstance(other, _VolumeSolver):
            if other.ctx is not self.ctx and other.ctx.device != self.ctx.device:
                raise ValueError('the other solver lives on device {}, this one on {}'.format(other.ctx.device, self.ctx.device))
            other.ctx.sync()
            other = other.x[other.cur]
        return resolution.fourier_shell_correlation(mine, other, psize_cm, ctx=self.ctx)

    # ---- the tail of the step ----------------------------------------------------------------
    def _reduces(self):
        return self.comm.size > 1 or self.comm.always_reduce

    def slab_bounds(self, n_slabs):
        """x-plane ranges [(x0, nx)] of n_slabs nearly equal slabs of the [X][Z][Y] volume."""
        n_slabs = max(1, min(int(n_slabs), self.dim_x))
        edges = [(self.dim_x * i) // n_slabs for i in range(n_slabs + 1)]
        return [(edges[i], edges[i + 1] - edges[i]) for i in range(n_slabs)]

    def tail_plan(self, n_slabs=None, sharded=None):
        """(n_slabs, sharded) of the exchange.  sharded = reduce-scatter -> Adam on this rank's 1/size of each slab ->
        all-gather: needs every slab to split evenly over the ranks, else the all-reduce form is used.
        BDOF_ALLREDUCE_SLABS / BDOF_SHARDED_ADAM override; tune_tail() picks the slab count by measurement."""
        if not self._reduces():
            return 1, False
        if n_slabs is None and sharded is None and self._plan is not None:
            return self._plan
        if n_slabs is None:
            n_slabs = int(os.environ.get('BDOF_ALLREDUCE_SLABS', '8'))
        if sharded is None:
            sharded = self.comm.sharded and os.environ.get('BDOF_SHARDED_ADAM', '1') != '0'
        n_slabs = max(1, min(int(n_slabs), self.dim_x))
        if sharded:
            n = n_slabs
            while n > 1 and self.dim_x % (n * self.comm.size):
                n -= 1
            if self.dim_x % (n * self.comm.size) == 0:
                n_slabs = n
            else:
                sharded = False
        return n_slabs, bool(sharded)

    def _adam_slab(self, u, slab, g_scale):
        new = 1 - self.cur
        self.eng.adam_step(self.x[self.cur], self.x[new], self.g, self.m, self.v, self.mask if u.use_mask else None,
                           (self.dim_x, self.dim_z, self.dim_y), u.i_update, u.learning_rate, g_scale=g_scale,
                           alpha_d=u.alpha_d, alpha_b=u.alpha_b, gamma=u.gamma, clip=u.clip, slab=slab)

    def _flip(self):
        self.cur = 1 - self.cur
        self._bind_volume()

    def adam_update(self, i_batch, learning_rate, alpha_d=0.0, alpha_b=0.0, gamma=0.0, clip=True, use_mask=True):
        """Regulariser + Adam on the gradient in self.g (whole volume, no exchange) with this rank's moments: wrong, and refused,
        once a sharded step has left them valid on 1/size of every slab only."""
        if self._epoch_plan is not None and self._epoch_plan[1] is not None:
            raise RuntimeError('adam_update() after a sharded step(): the Adam moments of this epoch are sharded over the ranks '
                               '(call reset_moments() first, or keep using step())')
        self._epoch_plan = ('taken', None)
        self._g_refresh()
        u = Update(i_batch, learning_rate, alpha_d=alpha_d, alpha_b=alpha_b, gamma=gamma, clip=clip, use_mask=use_mask)
        self._adam_slab(u, None, 1.0 / self.comm.size)
        self._flip()

    time_tail = False          # True: every _tail is bracketed by stream-ordered time stamps (bdof_timer_mark slots 0 / 1)

    def tail_ms(self):
        """Duration of the last tail on the ctx stream (rotation adjoint + exchange + Adam + all-gather), with time_tail on."""
        ms = ctypes.c_double(0)
        self.ctx.check(self.ctx.lib.bdof_timer_elapsed(self.ctx.handle, 0, 1, ctypes.byref(ms)))
        return ms.value

    def _tail(self, produce, u, n_slabs=None, sharded=None, flip=True, n_acc=1, one_pass=None):
        """produce(x0, nx): enqueue the kernels that leave this rank's gradient of x-planes [x0, x0+nx) in self.g.
        Then exchange + regulariser + Adam (+ mask, clip) of the Update u, slab by slab.  g_scale = 1 / (size * n_acc)
        (grads /= size, fullfield.py:351; accumulated minibatches are averaged, tensorflow_recon/fullfield.py:424).
        one_pass(u, g_scale): what to run in place of produce + Adam when nothing is exchanged (FullfieldSolver._one_pass_tail)."""
        comm, ctx = self.comm, self.ctx
        if self.time_tail:
            ctx.check(ctx.lib.bdof_timer_mark(ctx.handle, 0))
        g_scale = 1.0 / (comm.size * n_acc)
        if not self._reduces():
            if one_pass is not None:
                one_pass(u, g_scale=g_scale)
            else:
                produce(0, self.dim_x)
                self._adam_slab(u, None, g_scale)
        else:
            n_slabs, sharded = self.tail_plan(n_slabs, sharded)
            # Sharded form: the Adam moments (and, after the reduce-scatter, the gradient) are valid on this rank's 1/size of every
            # slab only, so the shard layout must not move while the moments live — i.e. until the next reset_moments().  The
            # all-reduce form keeps them whole on every rank, whatever its slab count.
            layout = (n_slabs, True) if sharded else None
            if self._epoch_plan is None:
                self._epoch_plan = ('taken', layout)
            elif self._epoch_plan[1] != layout:
                raise RuntimeError('the exchange plan changed from {} to {} inside an epoch: the Adam moments are sharded by the first one '
                                   '(call reset_moments() first)'.format(self._epoch_plan[1], layout))
            slabs = self.slab_bounds(n_slabs)
            self._g_shards = list(slabs) if sharded else None
            per_x = self.dim_z * self.dim_y * 2                  # floats per x-plane of the gradient / volume
            size, rank = comm.size, comm.rank
            tickets, gathers = [None] * len(slabs), []
            x_new = self.x[1 - self.cur]

            def finish(c):
                x0, nx = slabs[c]
                comm.wait(ctx, tickets[c])
                if sharded:
                    w = nx // size
                    self._adam_slab(u, (x0 + rank * w, w), g_scale)
                    gathers.append(comm.start_allgather(ctx, x_new, x0 * per_x, w * per_x))
                else:
                    self._adam_slab(u, (x0, nx), g_scale)

            for c, (x0, nx) in enumerate(slabs):
                produce(x0, nx)
                if sharded:
                    tickets[c] = comm.start_reduce_scatter(ctx, self.g, x0 * per_x, (nx // size) * per_x)
                else:
                    tickets[c] = comm.start_allreduce(ctx, self.g, x0 * per_x, (x0 + nx) * per_x)
                if c >= self.lookahead:
                    finish(c - self.lookahead)
            for c in range(max(0, len(slabs) - self.lookahead), len(slabs)):
                finish(c)
            for t in gathers:
                comm.wait(ctx, t)
        if flip:
            self._flip()
        if self.time_tail:
            ctx.check(ctx.lib.bdof_timer_mark(ctx.handle, 1))

    def tune_tail(self, candidates=(1, 8, 16, 32), reps=2):
        """Pick the number of slabs of the pipelined tail by timing it on this machine and process layout (the collective,
        the streams it runs on and the kernels either side interact in ways that differ between runtimes).  Dry run with
        learning rate 0 on a zeroed rotated-frame gradient: the gradient buffer, the spare volume buffer and the Adam
        moments are scratch afterwards (the moments are zeroed again), the volume is not touched.  Every rank takes the
        same decision (max of the timings over ranks).  `step` uses the result."""
        import time
        if not self._reduces() or os.environ.get('BDOF_ALLREDUCE_SLABS'):
            self._plan = self.tail_plan()
            return self._plan
        self._zero_rotated_gradient()
        plans = []
        for n in candidates:
            p = self.tail_plan(n)
            if p not in plans:
                plans.append(p)
        times = []
        for p in plans:
            self._epoch_plan = None                           # dry runs: the moments are scratch (zeroed again below)
            self._dry_tail(*p)                                # first use: communicator / stream set-up
            self.ctx.sync()
            self.comm.Barrier()
            t0 = time.perf_counter()
            for _ in range(reps):
                self._dry_tail(*p)
            self.ctx.sync()
            times.append(time.perf_counter() - t0)
        self._g_shards = None
        worst = self.comm.allreduce_max_host(np.array(times))
        self._plan = plans[int(np.argmin(worst))]
        self.tuned = {'{}slab{}'.format(p[0], '_sharded' if p[1] else ''): float(t) / reps for p, t in zip(plans, worst)}
        self.reset_moments()
        return self._plan

    def _zero_rotated_gradient(self):
        lib, h = self.ctx.lib, self.ctx.handle
        n = self.mb * self.dim_z * self.eng.nx * self.eng.ny * 8
        self.ctx.check(lib.bdof_memset(h, lib.bdof_grot(h), 0, n))

    # ---- optimisable probe (probe_type='optimizable', tensorflow_recon/fullfield.py:311-327,442-455) ---------------------
    def enable_probe_optimization(self, probe_real, probe_imag, probe_learning_rate=1e-3, pupil_function=None):
        """probe_real / probe_imag become optimisation variables with their own Adam (learning rate probe_learning_rate; its
        step counter runs over the whole level, as a tf.train.AdamOptimizer's does).  Every step() then also takes the
        gradient w.r.t. the probe (bdof_probe_grad: G(psi_0) summed over the minibatch), averages it over the ranks,
        updates the probe on the host in float64 — it is one (Y, X) field — multiplies by the pupil function
        (tensorflow_recon/fullfield.py:546-548) and hands it back to the engine, which re-derives its carrier (scalar, or
        the carrier field propagated on the device in float64).
        Probe modes (PtychoSolver with (M, py, px) probes): the arrays are (M, py, px), every mode has its own Adam moments
        (one step counter), the gradient is bdof_probe_grad_modes' and the pupil multiplies every mode."""
        probe = (np.asarray(probe_real, dtype=np.float64) + 1j * np.asarray(probe_imag, dtype=np.float64)) * np.ones((self.eng.ny, self.eng.nx))
        self.pvar = None
        if probe.ndim != (3 if self.n_modes else 2) or (self.n_modes and probe.shape[0] != self.n_modes):
            raise ValueError('enable_probe_optimization: the probe must have the shape the solver was built with ({})'.format(
                '{} probe modes'.format(self.n_modes) if self.n_modes else 'one (Y, X) probe'))
        self.pvar = ProbeVariable(probe, probe_learning_rate, pupil_function)
        self.eng.enable_probe_grad(True)
        # The resident amplitudes were laid out as m - |a0| for the probe in force at set_measurements (residual splitting,
        # MultisliceEngine.meas_layout).  A probe that moves every step would leave that reference behind — every residual biased by
        # |a0_new| - |a0_old|, or by |a0| itself once the carrier changes kind — so the splitting is switched off here and
        # amplitudes that are already resident are put back to plain m.
        old_ref = self.eng.meas_ref
        self.eng.residual_split = False
        self.pvar.to_engine(self.eng)
        if old_ref and self.meas is not None:
            self.ctx.sync()
            self.meas.upload((self.meas.download().astype(np.float64) + old_ref).astype(np.float32))

    def _of_probe(name):
        return property(lambda self: None if self.pvar is None else getattr(self.pvar, name))
    probe, probe_m, probe_v, probe_t = _of_probe('probe'), _of_probe('probe_m'), _of_probe('probe_v'), _of_probe('probe_t')

    def _probe_collect(self):
        """Add this minibatch's probe gradient to the device accumulator (call after every loss_grad)."""
        if self.pvar is not None:
            self.pvar.collect(self.eng)

    def _probe_apply(self):
        """Adam on (probe_real, probe_imag) with the accumulated gradient (mean over accumulated minibatches and ranks)."""
        if self.pvar is None or self.pvar.n_acc == 0:
            return
        self.ctx.sync()
        self.pvar.apply(self._rank_mean)
        self.pvar.to_engine(self.eng)

    def get_probe(self):
        return self.pvar.get()

    def shrink_wrap(self, thresh=1e-15):
        """mask = mask * (obj_delta > 1e-15)   (cnn_propagator/fullfield.py:365-368, intended behaviour, quirk Q8)."""
        if self.mask is not None:
            self.ctx.check(self.ctx.lib.bdof_mask_shrink(self.ctx.handle, self.x[self.cur].ptr, self.mask.ptr, self.nvox, thresh))


class FullfieldSolver(_VolumeSolver):
    def __init__(self, dim_y, dim_x, dim_z, n_theta, minibatch_size, energy_ev, psize_cm, free_prop_cm=None,
                 probe_real=None, probe_imag=None, variant='numpy_skip_last', comm=None, device=0, stream=None,
                 coord_ls=None, propagator='fft', kernel_size=17, recompute=False, rotation='nearest', theta=None, adjoint64=None,
                 detector_kernel='TF', loss_type='lsq', poisson_multiplier=2e6, slice_binning=1, detector_weights=None,
                 axis_tilt=0., axis_roll=0., center=None, rotation_matrices=None, refine_geometry=(), geometry_learning_rate=0.05):
        """loss_type / poisson_multiplier: the data term (MultisliceEngine.set_loss; 'poisson' with propagator='fft' only).
        detector_weights: one (Y, X) plane of weights >= 0 for every projection (MultisliceEngine.set_detector_weights; 0: the
        pixel takes no part), set before any measurement is bound; propagator='fft' only.
        slice_binning: voxel slices per propagation step (MultisliceEngine); > 1 with propagator='fft', rotation='nearest' and
        no adjoint64 only.
        free_prop_cm as a sequence of D distances: D detector planes per angle (MultisliceEngine.set_physics) — measurements and
        forward_angles are then (n, D, Y, X); with propagator='fft', rotation='nearest', the tape and no adjoint64 only.
        propagator='fft': the transfer-function step of np_funcs.py (north-star path); 'conv': the truncated real-space
        kernel of propagation.py, what cnn_propagator/fullfield.py:87,102 calls (kernel_size taps per axis).
        rotation='nearest': the cnn variant's lookup tables, fused into the kernels (cnn_propagator/util.py:294-402);
        'bilinear': the TF twin's tf_rotate(obj, theta[i], 'BILINEAR') (tensorflow_recon/fullfield.py:96) with the true angles
        `theta` (radians, one per projection): the minibatch's rotated objects are materialised per step
        (bdof_rotate_bilinear), its adjoint is a gather (bdof_rotate_bilinear_adjoint);
        'trilinear': a rigid map per angle, sampled trilinearly (bdof_set_object_rigid / bdof_rotate_rigid_adjoint), on the same
        path as 'bilinear' — util.rigid_geometry(theta, (Y, X, Z), axis_tilt, axis_roll, center): the axis tilted towards the
        beam by axis_tilt (laminography), rolled about the beam by axis_roll (radians), projecting onto detector column `center`
        (a pixel index, fractional if need be; None: the middle) — or rotation_matrices (n_theta, 3, 4), any rigid (M | t) per
        angle (util.check_rigid), which then stands in place of theta and the three geometry keywords.  With any other rotation
        these four keywords are ignored.
        refine_geometry: names out of 'center', 'axis_tilt', 'axis_roll', 'theta', 'shifts' (a per-angle detector offset, util.rigid_geometry)
        that every step() moves with the volume — geometry_gradient(), summed over the ranks, a host Adam whose step
        geometry_learning_rate is a displacement in pixels at the volume's edge (rotation.RigidGeometry), new rows for the next
        step; geometry() returns the current values.  rotation='trilinear' without rotation_matrices and without
        n_batch_per_update > 1 only.  Empty: nothing of this runs."""
        self.n_planes = _check_options(propagator, adjoint64, loss_type, poisson_multiplier, detector_weights, slice_binning, free_prop_cm,
                                       rotation=rotation if rotation in ('bilinear', 'trilinear') else 'nearest', recompute=recompute, detector_kernel=detector_kernel)
        engine64 = self._float64_paths(adjoint64, propagator)
        if adjoint64 and rotation in rotations.KINDS and (self.conv or adjoint64 == 'first'):
            raise ValueError("the float64 paths (adjoint64='first'; propagator='conv') run with the lookup-table rotation")
        if probe_real is not None and np.ndim(probe_real) == 3:
            raise ValueError("probe modes ((M, Y, X) probes) are ptychography's: FullfieldSolver takes one (Y, X) probe")
        if rotation not in ('nearest', 'bilinear', 'trilinear'):
            raise ValueError("rotation must be 'nearest', 'bilinear' or 'trilinear'")
        # the rotation's host side (for a materialised kind its float64 rows per angle): checked here, before anything is allocated
        self.rot = rotations.choose(rotation, (dim_y, dim_x, dim_z), n_theta, coord_ls, theta, (axis_tilt, axis_roll, center, rotation_matrices),
                                    refine=refine_geometry, rate=geometry_learning_rate)
        self.dim_y, self.dim_x, self.dim_z = int(dim_y), int(dim_x), int(dim_z)
        self.n_theta, self.mb = int(n_theta), int(minibatch_size)
        # what analytic_volume builds its maps and filters from
        self._rotation = (rotation, theta, axis_tilt, axis_roll, center, rotation_matrices)
        self._analytic = dict(propagator=propagator, free_prop_cm=free_prop_cm, energy_ev=energy_ev, psize_cm=psize_cm)
        self.comm = comm or PseudoComm()
        self.eng = MultisliceEngine(self.dim_y, self.dim_x, self.dim_z, self.mb, with_grad=True, device=device, stream=stream,
                                    recompute=recompute, adjoint64=engine64, slice_binning=slice_binning)
        self.eng.set_sweep_fusion(1)        # the fused forward sweep (a ctx of its own starts at 0)
        self.eng.set_adjoint_fusion(True)   # ... and the fused adjoint sweep behind it (MEASUREMENTS.md: the step-time criterion)
        if probe_real is None:
            probe_real, probe_imag = np.ones((dim_y, dim_x)), np.zeros((dim_y, dim_x))   # 'plane', fullfield.py:276-278
        self._set_up(energy_ev, psize_cm, kernel_size, (loss_type, poisson_multiplier), detector_weights, probe_real, probe_imag,
                     free_prop_cm=free_prop_cm, variant=variant, detector_kernel=detector_kernel)

    def _batch_buffers(self):
        self.meas_stage = DeviceBuffer(self.ctx, self.mb * self.n_planes * self.dim_x * self.dim_y * 4, np.float32,
                                       (self.mb, self.dim_x, self.dim_y) if self.n_planes == 1 else (self.mb, self.n_planes, self.dim_x, self.dim_y))
        self.angle_buf = DeviceBuffer(self.ctx, self.mb * 4, np.int32, (self.mb,))

    def set_measurements(self, prj_abs):
        """|prj| for every angle, (n_theta, Y, X) — with D detector planes (n_theta, D, Y, X) — (loss uses np.abs(this_prj_batch),
        fullfield.py:106).  The residual stays split
        or not by what these amplitudes are (MultisliceEngine.choose_residual_split)."""
        self.eng.choose_residual_split(prj_abs)
        self.meas = DeviceBuffer.from_host(self.ctx, self.eng.meas_layout(prj_abs))

    # ---- analytic starting volume (analytic.py; csrc/bdof_fbp.h) --------------------------------
    def analytic_rows(self):
        """(rows, angles) of analytic.rotation_rows for the rotation this solver runs with: for rotation='trilinear' built from theta
        and the axis keywords the CURRENT geometry (set_geometry, refine_geometry), else what the constructor was given."""
        rotation, theta, axis_tilt, axis_roll, center, rotation_matrices = self._rotation
        shape = (self.dim_y, self.dim_x, self.dim_z)
        if self.rot.geometry is not None:
            g = self.rot.geometry.values()
            return analytic.rotation_rows('trilinear', self.n_theta, shape, g['theta'], float(g['axis_tilt']), float(g['axis_roll']),
                                          float(g['center']), None, g['shifts'])
        return analytic.rotation_rows(rotation, self.n_theta, shape, theta, axis_tilt, axis_roll, center, rotation_matrices)

    def analytic_volume(self, prj_abs, delta_beta_ratio=10., ctf_regularization=1e-2, object_type='normal'):
        """Form the resident volume analytically from the measured amplitudes prj_abs (n_theta, Y, X) — with D detector planes
        (n_theta, D, Y, X), all of which enter — and bind it: contrast-transfer-function retrieval of the projected absorption for
        a homogeneous object delta = delta_beta_ratio * beta (regularised by ctf_regularization), a Ram-Lak filter and a
        back-projection through the maps of this solver's rotation (bdof_ctf_retrieve, bdof_backproject; analytic.py has the
        model), clipped at 0 and multiplied by the solver's mask.  No optimiser step; get_volume() returns the result.
        object_type 'phase_only' / 'absorption_only': that channel alone is retrieved, the other is 0.  Detector weights of 0 take
        their pixels out.  Every rank computes the whole volume from all angles, in batches of the minibatch size: identical bits
        on every rank, nothing communicated.  ValueError: analytic.check_analytic's refusals (propagator='conv', a probe that is
        not a plane wave, the far field, a negative ratio, a regularisation <= 0)."""
        a = self._analytic
        probe = self.pvar.get() if self.pvar is not None else self.eng.probe_arrays()
        a0_sq = analytic.check_analytic(a['propagator'], probe[0], probe[1], delta_beta_ratio, ctf_regularization, object_type, a['free_prop_cm'])
        D, nx, ny = self.n_planes, self.dim_x, self.dim_y
        self.eng._check_frames(prj_abs)
        prj_abs = np.asarray(prj_abs)
        if len(prj_abs) != self.n_theta:
            raise ValueError('analytic_volume takes the amplitudes of all {} angles'.format(self.n_theta))
        rows, angles = self.analytic_rows()
        weights = analytic.angle_weights(angles).astype(np.float32)
        filters = DeviceBuffer.from_host(self.ctx, analytic.ctf_filters(nx, ny, a['energy_ev'], a['psize_cm'], a['free_prop_cm'], self.dim_z,
                                                                        delta_beta_ratio, ctf_regularization, object_type))
        wgt = None if self.eng.detector_weights is None else DeviceBuffer.from_host(
            self.ctx, np.ascontiguousarray(np.asarray(self.eng.detector_weights, dtype=np.float32).T))
        q = DeviceBuffer(self.ctx, self.mb * nx * ny * 4, np.float32, (self.mb, nx, ny))
        prm = DeviceBuffer(self.ctx, self.mb * 12 * 8, np.float64, (self.mb, 12))
        w = DeviceBuffer(self.ctx, self.mb * 4, np.float32, (self.mb,))
        per_voxel = 1.0 / (float(a['psize_cm']) * 1e7)                # the projected quantity is in nm
        scale = {'normal': (delta_beta_ratio * per_voxel, per_voxel), 'phase_only': (per_voxel, 0.), 'absorption_only': (0., per_voxel)}[object_type]
        lib, h, vol = self.ctx.lib, self.ctx.handle, self.x[self.cur]
        for i in range(0, self.n_theta, self.mb):
            B = min(self.mb, self.n_theta - i)
            frames = np.zeros((self.mb,) + (() if D == 1 else (D,)) + (nx, ny), dtype=np.float32)
            frames[:B] = np.swapaxes(prj_abs[i:i + B], -2, -1)
            r64, w32 = np.zeros((self.mb, 12)), np.zeros(self.mb, dtype=np.float32)
            r64[:B], w32[:B] = rows[i:i + B], weights[i:i + B]
            self.meas_stage.upload(frames)
            prm.upload(r64)
            w.upload(w32)
            self.ctx.check(lib.bdof_ctf_retrieve(h, self.meas_stage.ptr, _lib._ptr(wgt), a0_sq, filters.ptr, B, D, nx, ny, q.ptr))
            self.ctx.check(lib.bdof_backproject(h, q.ptr, nx, ny, prm.ptr, w.ptr, B, vol.ptr, self.dim_x, self.dim_z, self.dim_y,
                                                0, self.dim_x * self.dim_z, int(i > 0), scale[0], scale[1]))
        self.ctx.check(lib.bdof_volume_clip_mask(h, vol.ptr, _lib._ptr(self.mask), self.nvox))
        self.ctx.sync()                                               # (the temporaries below go with this call)
        for buf in (filters, wgt, q, prm, w):
            if buf is not None:
                buf.free()
        self._bind_volume()

    # ---- one Adam iteration ------------------------------------------------------------------
    def _rot_loss_grad(self, angle_idx, f64=False):
        """Forward + adjoint sweeps of this rank's angles: the gradient w.r.t. the rotated objects stays in the ctx.
        f64: through the transfer-function model's float64 path on the same context (bdof_loss_grad_tf_f64)."""
        idx = np.asarray(angle_idx, dtype=np.int32)
        assert len(idx) == self.mb
        self.angle_buf.upload(idx)
        # this_prj_batch = prj[this_ind_batch] (fullfield.py:344): one gather launch on the resident stack (an angle's planes are one item)
        self.ctx.check(self.ctx.lib.bdof_gather_fields(self.ctx.handle, self.meas_stage.ptr, self.meas.ptr, self.angle_buf.ptr, self.mb,
                                                       self.n_planes * self.dim_x * self.dim_y * 4))
        self._angles = np.asarray(angle_idx, dtype=np.int64)
        if f64:
            if not self.rot.float64_paths:
                raise ValueError("f64: the float64 paths run with the lookup-table rotation")
            if self.conv and not self.eng.conv_f64:      # (a probe or physics set since the last call unbound the twin)
                self.eng.enable_conv_f64()
            if not self.conv and not self.eng.tf_f64:
                self.eng.enable_tf_f64()
        else:
            self.rot.stage(self.eng, self.x[self.cur], angle_idx, self.mb, self.conv)
        self.eng.loss_grad_device(self.mb, self.rot.angle_arg(self.angle_buf.ptr), None, None, self.meas_stage.ptr,
                                  conv=self.conv, f64=f64)

    def _produce(self, accumulate=False):
        return lambda x0, nx: self.rot.adjoint(self.angle_buf, self.g, x0, nx, accumulate)

    def loss_and_grad(self, angle_idx, want_loss=True, f64=False):
        """Data-term loss and its gradient w.r.t. the volume for this rank's angles (left in self.g, not reduced).  f64: both
        sweeps through the model's float64 path (a float64 twin of the fused kernels on the same context; the tests hold it to 3e-15 /
        2.5e-8 of the host's float64 restatement at the sizes that reaches: tests/test_gpu_parity.py)."""
        self._rot_loss_grad(angle_idx, f64=f64 or self.f64 is True)
        self._g_is_local()
        self._produce()(0, self.dim_x)
        return self._get_loss() if want_loss else None

    def _one_pass_tail(self, u, g_scale):
        """The tail of a step that exchanges nothing, in one pass (bdof_rotation_adjoint_adam): the volume gradient is not written
        (self.g is stale until _g_refresh), and the new volume's modulation table is in the ctx when _flip binds it."""
        lib, h = self.ctx.lib, self.ctx.handle
        new = 1 - self.cur
        mask = self.mask if u.use_mask else None
        self.ctx.check(lib.bdof_rotation_adjoint_adam(h, self.mb, self.angle_buf.ptr, None, 0, self.dim_x * self.dim_z, 0, 1.0,
                                                      self.x[self.cur].ptr, self.x[new].ptr, self.m.ptr, self.v.ptr, _lib._ptr(mask),
                                                      self.dim_x, self.dim_z, self.dim_y, g_scale, u.alpha_d, u.alpha_b, u.gamma,
                                                      u.learning_rate, 0.9, 0.999, 1e-8, int(u.i_update), int(u.clip)))
        self._g_shards = None
        self._g_stale = True

    def _dry_tail(self, n_slabs, sharded):
        idx = np.arange(self.mb, dtype=np.int32) % self.n_theta
        self.angle_buf.upload(idx)
        self.rot.stage_angles(idx)
        self._tail(self._produce(), Update(0, 0.0), n_slabs=n_slabs, sharded=sharded, flip=False)

    def step(self, i_batch, angle_idx, learning_rate, alpha_d=0.0, alpha_b=0.0, gamma=0.0, want_loss=False, n_slabs=None,
             sharded=None, use_mask=True, clip=True, n_batch_per_update=1, last_of_epoch=False):
        """grads = loss_grad(...); Allreduce; /size; Adam; mask; clip   (fullfield.py:345-362).

        n_batch_per_update > 1 (tensorflow_recon/fullfield.py:413-425,512-530): the volume gradient of consecutive
        minibatches is accumulated and applied (averaged) every n-th minibatch or at the last one of the epoch; the Adam
        bias-correction exponent then counts updates, not minibatches."""
        if self.rot.geometry is not None and self.rot.geometry.refine and int(n_batch_per_update) > 1:
            raise ValueError('refine_geometry moves the geometry at every minibatch: not together with n_batch_per_update > 1')
        self._rot_loss_grad(angle_idx, f64=self.f64 is True or (self.f64 == 'first' and i_batch == 0 and self.probe is None))
        self._probe_collect()
        self._refine_geometry()
        nb = max(1, int(n_batch_per_update))
        u = Update(i_batch // nb, learning_rate, alpha_d=alpha_d, alpha_b=alpha_b, gamma=gamma, clip=clip, use_mask=use_mask)
        if nb > 1:
            self._g_is_local()
            self._produce(accumulate=self._acc > 0)(0, self.dim_x)
            self._acc += 1
            if self._acc == nb or last_of_epoch:
                n_acc, self._acc = self._acc, 0
                self._tail(lambda x0, nx: None, u, n_slabs, sharded, n_acc=n_acc)
                self._probe_apply()
        else:
            # one rank, a rotation that carries it (the lookup tables): nothing happens between the rotation adjoint and Adam
            one_pass = self._one_pass_tail if not self._reduces() and self.rot.one_pass_tail else None
            self._tail(self._produce(), u, n_slabs, sharded, one_pass=one_pass)
            self._probe_apply()
        return self._get_loss() if want_loss else None          # the loss of THIS minibatch stays on the device until the next one

    def forward_angles(self, angle_idx):
        """Detector waves (len(idx), Y, X) of the current volume — the forward_pass of fullfield.py:79-91; with D detector planes
        (len(idx), D, Y, X)."""
        idx = np.asarray(angle_idx, dtype=np.int32)
        out = []
        for i in range(0, len(idx), self.mb):
            chunk = idx[i:i + self.mb]
            self.rot.stage(self.eng, self.x[self.cur], chunk, len(chunk), self.conv)
            out.append(self.eng.forward(len(chunk), angle_idx=self.rot.angle_arg(chunk), conv=self.conv))
        return np.concatenate(out, axis=0)


class PtychoSolver(_VolumeSolver):
    """Device-resident state of a ptychographic reconstruction (cnn_propagator/ptychography.py:285-310): volume,
    Adam moments, rotation tables, all diffraction amplitudes; windows are cut by index math inside the kernels."""

    def __init__(self, obj_size, probe_size, probe_pos, n_theta, minibatch_size, energy_ev, psize_cm, probe_real, probe_imag,
                 variant='numpy_skip_last', comm=None, device=0, stream=None, coord_ls=None, propagator='fft', kernel_size=17,
                 adjoint64=None, engine=None, loss_type='lsq', poisson_multiplier=2e6, slice_binning=1, detector_weights=None,
                 rotation='nearest', theta=None, axis_tilt=0., axis_roll=0., center=None, rotation_matrices=None, refine_geometry=(),
                 geometry_learning_rate=0.05, position_offsets=None, refine_positions=None, position_learning_rate=0.05):
        """position_offsets: (n_pos, 2) or (n_theta, n_pos, 2) pixels in the order of probe_pos (y, x), added to probe_pos: the windows
        are then cut at fractional origins.  refine_positions: None, 'shared' (one offset per position for all angles) or 'per_angle':
        every step() also takes position_gradient() (bdof_window_position_grad), sums it over the ranks and moves the listed offsets
        by a host Adam whose step position_learning_rate is in pixels (positions.ProbePositions); positions() returns them.  With
        either keyword set a step cuts the minibatch's windows into a stack [mb][S][px][py] of (delta, beta) pairs
        (bdof_window_stack), binds it as a batch of already rotated objects and sweeps without angle and window offsets; the window
        adjoint is bdof_window_stack_adjoint.  MEMORY: the stack and the modulation table built from it take mb * S * px * py * 8
        bytes EACH — 4.25 GB each for 400 windows of 72 x 72 over 256 slices.  Transfer-function propagator, float32 sweeps (no
        adjoint64), slice_binning 1, every engine, both rotations; with neither keyword set nothing of this runs and a step has the
        bits it had.  Gauge: the mean offset is a translation of the object against the scan and is not removed.
        refine_geometry / geometry_learning_rate: as for FullfieldSolver (the step's one angle moves).
        rotation='nearest': the lookup tables.  'trilinear': the rigid map of FullfieldSolver(rotation='trilinear'), with the same
        theta / axis_tilt / axis_roll / center / rotation_matrices (tilt 0: ptychography's interpolating rotation), through a rotated
        copy per step (rotation.RotatedCopy).  slice_binning > 1 keeps to rotation='nearest'.
        loss_type / poisson_multiplier: the data term (MultisliceEngine.set_loss; 'poisson' with propagator='fft' only).
        detector_weights: one (py, px) plane of weights >= 0 for every diffraction pattern, fftshifted as the patterns are
        (MultisliceEngine.set_detector_weights; 0: dead pixel, beamstop), set before any measurement is bound; propagator='fft' only.
        slice_binning: voxel slices per propagation step (MultisliceEngine); > 1 with propagator='fft' and no adjoint64 only, and
        engine=None then takes 'auto' (the resident engine does not carry it).
        engine: None picks the LDS-resident engine for small square probes (below) and the automatic choice otherwise; 'auto',
        'generic', 'streaming' or 'resident' go to MultisliceEngine(engine=...) as they are.
        probe_real / probe_imag of shape (M, py, px): M probe modes whose intensities add (partial coherence; modes.py,
        bdof_set_probe_modes) — a 2-D probe takes the single-probe path and gives the bits it gave.  With modes engine=None picks
        'resident' for the sizes with a resident plan and 'generic' otherwise ('streaming' raises), every minibatch sweeps mb * M
        wavefields (the tape and the engine's batch are M times those of one probe), and propagator='conv', slice_binning > 1 and
        adjoint64 raise (modes.check_probe_modes).  position_offsets / refine_positions, rotation='trilinear' and refine_geometry
        work as they do with one probe: they read the window gradient, in which the modes are already summed."""
        if rotation not in ('nearest', 'trilinear'):
            raise ValueError("rotation must be 'nearest' or 'trilinear'")
        _check_options(propagator, adjoint64, loss_type, poisson_multiplier, detector_weights, slice_binning, rotation=rotation)
        offsets = probe_positions.check_positions(position_offsets, refine_positions, len(probe_pos), n_theta, propagator=propagator,
                                                  slice_binning=slice_binning, adjoint_precision='float64' if adjoint64 else None)
        self.pos = None if offsets is None else probe_positions.ProbePositions(n_theta, len(probe_pos), offsets, refine_positions, position_learning_rate)
        if np.ndim(probe_real) == 3:
            precision = None if not adjoint64 else 'first-step' if adjoint64 == 'first' else 'float64'
            self.n_modes = probe_modes.check_probe_modes(int(np.shape(probe_real)[0]), propagator=propagator, slice_binning=slice_binning,
                                                         adjoint_precision=precision, engine=engine)
        engine64 = self._float64_paths(adjoint64, propagator)
        self.dim_y, self.dim_x, self.dim_z = [int(s) for s in obj_size]
        self.rot = rotations.choose(rotation, obj_size, n_theta, coord_ls, theta, (axis_tilt, axis_roll, center, rotation_matrices),
                                    materialised=rotations.RotatedCopy, refine=refine_geometry, rate=geometry_learning_rate)
        self.py, self.px = int(probe_size[0]), int(probe_size[1])
        self.n_theta, self.mb = int(n_theta), int(minibatch_size)
        self.comm = comm or PseudoComm()
        self.probe_pos = np.asarray(probe_pos).astype(int)
        self.half = (np.array(probe_size) / 2).astype('int')            # ptychography.py:138
        # small square probes: the LDS-resident engine (one launch per minibatch) also for the minibatches of ~20 positions the
        # drivers use, where the automatic choice would take the launch-bound streaming kernels for 64^2 / 128^2
        if engine is None:
            engine = 'resident' if self.py == self.px and self.py in RESIDENT_SIZES and not self.conv and slice_binning == 1 else \
                'generic' if self.n_modes else 'auto'
        self.eng = MultisliceEngine(self.py, self.px, self.dim_z, self.mb * max(self.n_modes, 1), with_grad=True, device=device, stream=stream,
                                    engine=engine, adjoint64=engine64, slice_binning=slice_binning)
        self._set_up(energy_ev, psize_cm, kernel_size, (loss_type, poisson_multiplier), detector_weights, probe_real, probe_imag,
                     free_prop_cm='inf', variant=variant)                        # ('inf': ptychography.py:76)

    def _batch_buffers(self):
        self.meas_stage = DeviceBuffer(self.ctx, self.mb * self.py * self.px * 4, np.float32, (self.mb, self.py, self.px))
        self.idx_buf = DeviceBuffer(self.ctx, 4 * self.mb * 4, np.int32, (4, self.mb))
        if self.pos is not None:
            # the window stack [mb][S][px][py] of pairs, the origins (u, v) it is cut at and their derivative
            self.stack = DeviceBuffer(self.ctx, self.mb * self.dim_z * self.px * self.py * 8, np.float32, (self.mb, self.dim_z, self.px, self.py, 2))
            self.origin_buf = DeviceBuffer(self.ctx, self.mb * 16, np.float64, (self.mb, 2))
            self.dpos_buf = DeviceBuffer(self.ctx, self.mb * 16, np.float64, (self.mb, 2))

    def set_measurements(self, prj_abs_all):
        """All diffraction amplitudes |prj| (n_theta, n_pos, py, px) resident on the device (a cfg5-sized dataset is 0.75 GB):
        the minibatch is then picked out by one gather launch instead of an HDF5 read + upload per step
        (this_prj_batch = prj[this_i_theta, this_ind_batch], ptychography.py:295)."""
        a = np.asarray(prj_abs_all)
        self.n_pos_all = a.shape[1]
        self.meas_all = DeviceBuffer.from_host(self.ctx, self.eng.meas_layout(a.reshape((-1,) + a.shape[2:])))

    def _stage(self, i_theta, pos_idx, prj_abs_batch):
        pos = self.probe_pos[np.asarray(pos_idx)]
        idx = np.empty((4, self.mb), dtype=np.int32)
        idx[0] = self.rot.window_angle(i_theta)
        idx[1] = pos[:, 1] - self.half[1]            # window origin in x (axis 1), ptychography.py:68-70
        idx[2] = pos[:, 0] - self.half[0]            # window origin in y (axis 0)
        idx[3] = 0
        p = self.idx_buf.ptr
        if prj_abs_batch is None:
            if self.meas_all is None:
                raise ValueError('no measurements: pass prj_abs_batch or call set_measurements first')
            idx[3] = int(i_theta) * self.n_pos_all + np.asarray(pos_idx)
            self.idx_buf.upload(idx)
            self.ctx.check(self.ctx.lib.bdof_gather_fields(self.ctx.handle, self.meas_stage.ptr, self.meas_all.ptr, p + 12 * self.mb, self.mb,
                                                           self.py * self.px * 4))
        else:
            self.idx_buf.upload(idx)
            self.meas_stage.upload(self.eng.meas_layout(prj_abs_batch))
        return p, p + 4 * self.mb, p + 8 * self.mb

    def _stack_windows(self, i_theta, pos_idx, for_gradient=True):
        """The windows of positions pos_idx (at most mb) at their fractional origins, cut from the volume under angle i_theta
        into self.stack and bound as that many already rotated objects.  for_gradient: a window gradient will belong to them."""
        pos_idx = np.asarray(pos_idx)
        n = len(pos_idx)
        at = self.probe_pos[pos_idx] + self.pos.of(i_theta, pos_idx)
        origin = np.zeros((self.mb, 2))
        origin[:n, 0] = at[:, 1] - self.half[1]          # u: along x (axis 1), as _stage's integer origins
        origin[:n, 1] = at[:, 0] - self.half[0]          # v: along y (axis 0)
        self.origin_buf.upload(origin)
        self.rot.stage(self.eng, self.x[self.cur], [int(i_theta)], 1, self.conv)
        self._source = self.rot.window_source(self.x[self.cur], i_theta)
        self.ctx.check(self.ctx.lib.bdof_window_stack(self.ctx.handle, self._source[0], self.dim_x, self.dim_y, self._source[1], self.origin_buf.ptr,
                                                      n, self.stack.ptr))
        self.eng.set_volume(self.stack, n * self.dim_z * self.px, self.py, None, 0, 0)
        self._last_pos = (int(i_theta), pos_idx.copy()) if for_gradient else None

    def _win_loss_grad(self, i_theta, pos_idx, prj_abs_batch, use64=False):
        a, xo, yo = self._stage(i_theta, pos_idx, prj_abs_batch)
        f64 = self.f64 is True or (use64 and self.f64 == 'first')
        if self.pos is not None:
            self._stack_windows(i_theta, pos_idx)
            self.eng.loss_grad_device(self.mb, None, None, None, self.meas_stage.ptr)
        else:
            self.rot.stage(self.eng, self.x[self.cur], [int(i_theta)], 1, self.conv)
            self.eng.loss_grad_device(self.mb, a, xo, yo, self.meas_stage.ptr, conv=self.conv, f64=f64)
        self._last = (int(i_theta), xo, yo)
        self._angles = np.array([int(i_theta)], dtype=np.int64)

    def _produce_all(self):
        i_theta, xo, yo = self._last
        self._g_is_local()
        if self.pos is not None:
            self.rot.window_stack_adjoint(i_theta, self.origin_buf, self.g)
        else:
            self.rot.window_adjoint(i_theta, xo, yo, self.g)

    # ---- probe positions (positions.ProbePositions) ---------------------------------------------------------------------------
    def positions(self):
        """The current offsets (n_theta, n_pos, 2), pixels in the order of probe_pos (y, x): what refine_positions has made of them."""
        if self.pos is None:
            raise ValueError('positions(): the solver was built without position_offsets and refine_positions')
        return self.pos.values()

    def position_gradient(self):
        """dL/d(offset) of the data term for the positions of the last loss_and_grad (or, inside step, of the step, before the tail
        flips the volume), (mb, 2) in the order of probe_pos (y, x), not reduced over the ranks: one reduction on the device over the
        volume that was cut, the origins and the window-frame gradient (bdof_window_position_grad).  The download waits for the stream."""
        if self.pos is None or self._last_pos is None:
            raise RuntimeError('position_gradient() follows loss_and_grad() or runs inside step() of a solver built with position_offsets or refine_positions')
        self.ctx.check(self.ctx.lib.bdof_window_position_grad(self.ctx.handle, self._source[0], self.dim_x, self.dim_y, self._source[1], None,
                                                              self.origin_buf.ptr, self.mb, self.dpos_buf.ptr, 0))
        self.ctx.sync()
        return self.dpos_buf.download()[:, ::-1].copy()           # (dL/du, dL/dv) = (x, y) -> (y, x)

    def orthogonalize_probe_modes(self):
        """The optimised probe modes mixed into their orthogonal form, descending in power (modes.orthogonalize: a unitary mix, the
        model's intensities do not change).  The probe's Adam moments and step counter start again: they belong to the basis
        that went.  Returns the modes' relative powers."""
        if self.probe is None or self.probe.ndim != 3:
            raise ValueError('orthogonalize_probe_modes(): the solver optimises no probe modes (enable_probe_optimization with (M, py, px) probes)')
        self.pvar.restart(probe_modes.orthogonalize(self.probe))
        self.pvar.to_engine(self.eng)
        return probe_modes.relative_power(self.probe)

    def loss_and_grad(self, i_theta, pos_idx, prj_abs_batch=None, want_loss=True, f64=False):
        """prj_abs_batch: |this_prj_batch| (mb, py, px) for probe positions pos_idx at angle i_theta (None: from the resident
        stack of set_measurements).  f64: through the model's float64 path (solver built with adjoint64='first')."""
        if f64 and self.f64 is None:
            raise ValueError("f64: build the solver with adjoint64='first' (the float64 path's buffers are allocated there)")
        self._win_loss_grad(i_theta, pos_idx, prj_abs_batch, use64=bool(f64))
        self._produce_all()
        return self._get_loss() if want_loss else None

    def _dry_tail(self, n_slabs, sharded):
        self._tail(lambda x0, nx: None, Update(0, 0.0, use_mask=False), n_slabs=n_slabs, sharded=sharded, flip=False)

    def step(self, i_batch, i_theta, pos_idx, prj_abs_batch=None, learning_rate=1.0, want_loss=False, n_slabs=None, sharded=None, clip=True):
        """One Adam iteration of ptychography.py:301-310: loss_grad, Allreduce, /size, Adam, clip (no regulariser, no mask).
        The window/rotation adjoint produces the whole volume gradient in one pass; exchange and Adam are still slab-wise."""
        self._win_loss_grad(i_theta, pos_idx, prj_abs_batch,
                            use64=self.f64 == 'first' and i_batch == 0 and self.probe is None)
        self._probe_collect()
        self._produce_all()
        self._refine_geometry()          # (after the window adjoint: the rotated-frame gradient is the rotated copy's)
        if self.pos is not None:
            self._refine(self.pos, self.position_gradient, *self._last_pos)
        self._tail(lambda x0, nx: None, Update(i_batch, learning_rate, clip=clip, use_mask=False), n_slabs=n_slabs, sharded=sharded)
        self._probe_apply()
        return self._get_loss() if want_loss else None

    def forward(self, i_theta, pos_idx):
        pos = self.probe_pos[np.asarray(pos_idx)]
        if self.pos is not None:
            self._stack_windows(i_theta, pos_idx, for_gradient=False)
            return self.eng.forward(len(pos))
        self.rot.stage(self.eng, self.x[self.cur], [int(i_theta)], 1, self.conv)
        return self.eng.forward(len(pos), angle_idx=[self.rot.window_angle(i_theta)] * len(pos), xoff=pos[:, 1] - self.half[1],
                                yoff=pos[:, 0] - self.half[0], conv=self.conv)
