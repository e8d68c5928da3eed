"""Python host of the multislice engine: owns a libbdof context and converts between the reference's
array conventions ((B, Y, X, S) objects, (B, Y, X) waves, (Y, X, Z) volumes) and the device layout.
All arithmetic of the hot path runs in libbdof.so; there is no CPU fallback."""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import DeviceBuffer
from . import util
from . import modes as probe_modes_mod

_VARIANT = {'numpy_skip_last': _lib.VARIANT_NUMPY_SKIP_LAST, 'tf_all': _lib.VARIANT_TF_ALL}
_LOSS = {'lsq': _lib.LOSS_LSQ, 'poisson': _lib.LOSS_POISSON}


def check_loss(loss_type, poisson_multiplier):
    """The data term's two keywords as every layer takes them (raises ValueError)."""
    if loss_type not in _LOSS:
        raise ValueError("loss_type must be 'lsq' or 'poisson'")
    if not float(poisson_multiplier) > 0:
        raise ValueError('poisson_multiplier must be > 0')


def check_detector_weights(w, ny, nx):
    """One (ny, nx) plane of finite weights >= 0, not all of them 0, as float32 (raises ValueError('detector_weights ...'))."""
    w = np.asarray(w)
    if w.shape != (ny, nx):
        raise ValueError('detector_weights must have the shape of one measured frame, {}, not {}'.format((ny, nx), w.shape))
    if w.dtype.kind not in 'fiub':
        raise ValueError('detector_weights must be real numbers')
    w = np.ascontiguousarray(w, dtype=np.float32)
    if not np.isfinite(w).all():
        raise ValueError('detector_weights must be finite')
    if (w < 0).any():
        raise ValueError('detector_weights must be >= 0')
    if not (w > 0).any():
        raise ValueError('detector_weights must leave at least one pixel with a weight > 0')
    return w


def read_detector_weights(detector_weights, data_path, frame_shape):
    """The detector_weights keyword of the entry points as a checked (Y, X) float32 plane, or None: an array, or the name of a
    dataset of the data file (for instance 'exchange/weights')."""
    if detector_weights is None:
        return None
    if isinstance(detector_weights, str):
        from . import h5io
        try:
            detector_weights = h5io.read_dataset(data_path, detector_weights)
        except KeyError as e:
            raise ValueError('detector_weights: {}'.format(e))
    return check_detector_weights(detector_weights, int(frame_shape[0]), int(frame_shape[1]))


def check_slice_binning(slice_binning):
    """The slice_binning keyword as every layer takes it: an integer >= 1 (raises ValueError)."""
    if isinstance(slice_binning, bool) or not isinstance(slice_binning, (int, np.integer)) or slice_binning < 1:
        raise ValueError('slice_binning must be an integer >= 1')


# ---- the model's options against the path of a call ------------------------------------------------------------------------------
# The path: what a call runs on, by the keyword that chooses it, with the value that carries every option.  `method` is an
# engine method that steps off the main path, by the words its refusal begins with.
PATH = dict(propagator='fft', adjoint_precision=None, rotation='nearest', engine='auto', recompute=False, adjoint64=False,
            no_grot=False, detector_kernel='TF', method=None)
_SET_CONV = 'the real-space propagator (set_conv)'
_TF_F64 = 'the float64 twin (enable_tf_f64)'
_CONV_F64 = 'the float64 twin (enable_conv_f64)'
_FORWARD_CONV = 'the real-space propagator (forward(conv=True))'
_LOSS_GRAD_OFF = 'the real-space propagator / the float64 twin (loss_grad(conv=True / f64=True))'
_BINNING_ENGINES = "slice_binning > 1 runs on the streaming and generic engines with the tape: not engine='resident', recompute, adjoint64 or no_grot"
_PLANES_F32 = "several detector planes have no float64 twin: adjoint_precision must be 'float32' (no adjoint64)"
_F32 = (None, 'float32')

# option -> what it needs of the path: (keyword of the path, test of its value, text of the ValueError; {} is the value), in the
# order in which they are reported.  An explicit adjoint_precision other than 'float32' is refused; None: not given.
OPTION_NEEDS = {
    'poisson': (('propagator', lambda v: v == 'fft', "loss_type='poisson' runs on the transfer-function propagator (propagator='fft') only"),),
    'weights': (('propagator', lambda v: v == 'fft', "detector_weights run on the transfer-function propagator (propagator='fft') only"),),
    'binning': (
        ('propagator', lambda v: v == 'fft', "slice_binning > 1 runs on the transfer-function propagator (propagator='fft') only"),
        ('adjoint_precision', lambda v: v in _F32, "slice_binning > 1 has no float64 twin: adjoint_precision must be 'float32'"),
        ('rotation', lambda v: v == 'nearest', "slice_binning > 1 runs on the rotation tables (rotation='nearest') only"),
        ('engine', lambda v: v != 'resident', _BINNING_ENGINES),
        ('recompute', lambda v: not v, _BINNING_ENGINES),
        ('adjoint64', lambda v: not v, _BINNING_ENGINES),
        ('no_grot', lambda v: not v, _BINNING_ENGINES),
        ('method', lambda v: v not in (_SET_CONV, _TF_F64, _CONV_F64), '{} does not carry slice_binning > 1'),
    ),
    'planes': (
        ('propagator', lambda v: v == 'fft', "several detector planes (free_prop_cm as a sequence) run on the transfer-function propagator (propagator='fft') only"),
        ('adjoint_precision', lambda v: v in _F32, _PLANES_F32),
        ('adjoint64', lambda v: not v, _PLANES_F32),
        ('recompute', lambda v: not v, 'several detector planes run with the tape: not recompute'),
        ('rotation', lambda v: v == 'nearest', "several detector planes run on the rotation tables (rotation='nearest') only"),
        ('detector_kernel', lambda v: v in ('TF', 'IR'), "several detector planes share one detector_kernel, 'TF' or 'IR': not {!r}"),
        ('method', lambda v: v not in (_SET_CONV, _TF_F64, _FORWARD_CONV, _LOSS_GRAD_OFF), '{} does not carry several detector planes'),
    ),
}


def check_option_path(option, path):
    """Raise the ValueError of the first thing `option` needs that `path` (PATH with some keywords replaced) does not give."""
    for key, carries, text in OPTION_NEEDS[option]:
        if not carries(path[key]):
            raise ValueError(text.format(path[key]))


def check_model_options(loss_type='lsq', poisson_multiplier=2e6, detector_weights=None, slice_binning=1, free_prop_cm=None, **path):
    """The option keywords as every layer takes them (check_loss, check_slice_binning and util.detector_distances raise ValueError
    for a bad one), and for every option that is on that the call stays on what carries it (OPTION_NEEDS); **path: the
    keywords of PATH the caller has.  Returns the number of frames per angle (1 without detector planes)."""
    path = dict(PATH, **path)
    if len(path) != len(PATH):
        raise TypeError('not of the path: {}'.format(sorted(set(path) - set(PATH))))
    check_loss(loss_type, poisson_multiplier)
    if loss_type == 'poisson':
        check_option_path('poisson', path)
    if detector_weights is not None:
        check_option_path('weights', path)
    check_slice_binning(slice_binning)
    if slice_binning > 1:
        check_option_path('binning', path)
    planes = util.detector_distances(free_prop_cm)[1]
    if planes is None:
        return 1
    check_option_path('planes', path)
    return len(planes)


def _hp(arr):
    """Host pointer of a numpy array for a library call (None stays None)."""
    return None if arr is None else arr.ctypes.data


RESIDENT_SIZES = (32, 36, 48, 64, 72, 80, 96, 128)      # square fields with an LDS-resident plan (csrc/bdof_resident.h)


class MultisliceEngine(object):
    """One wavefield geometry (NY x NX x S) on one GPU."""

    def __init__(self, ny, nx, n_slice, batch_max, with_grad=True, device=0, stream=None, force_generic=False, engine='auto',
                 recompute=False, no_grot=False, adjoint64=False, slice_binning=1):
        """Engines (include/bdof.h, bdof_configure): powers of two in 64..1024 run on the fused streaming kernels; small
        square fields (32..128, e.g. the 72 x 72 ptychography probe) on the LDS-resident kernel when there is no fused plan
        or the batch is large; every other size on the generic engine (rocFFT).  engine='generic' (= force_generic=True),
        'streaming' (never resident) or 'resident' (resident for every batch size) pin the choice for cross-checks.
        adjoint64=True: the adjoint sweep in float64 (bdof_configure flag 64; generic engine) — the
        accuracy option for reconstructions that must follow the reference's float64 loop voxel by voxel.
        slice_binning=b: one propagation step per b voxel slices (bdof_set_slice_binning, include/bdof.h) — the modulation
        factors of a bin are multiplied, one transfer-function step of b * delta_nm follows, n_steps = n_slice / b steps in
        all; streaming and generic engines, float32 sweeps with the tape."""
        check_slice_binning(slice_binning)
        b = int(slice_binning)
        if int(n_slice) % b:
            raise ValueError('slice_binning must divide n_slice ({} % {} != 0)'.format(int(n_slice), b))
        check_model_options(slice_binning=b, engine=engine, recompute=recompute, adjoint64=adjoint64, no_grot=no_grot)
        if engine not in ('auto', 'generic', 'streaming', 'resident'):
            raise ValueError('engine must be auto, generic, streaming or resident')
        force_generic = force_generic or engine == 'generic'
        self.recompute = bool(recompute)
        self.adjoint64 = bool(adjoint64) and bool(with_grad)
        self.ctx = _lib.Context(device, stream)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.ny, self.nx, self.n_slice, self.batch_max = int(ny), int(nx), int(n_slice), int(batch_max)
        self.with_grad = bool(with_grad)
        self.slice_binning, self.n_steps = b, self.n_slice // b
        flags = (_lib.CFG_GRAD if with_grad else 0) | (_lib.CFG_GENERIC if force_generic else 0) \
            | (_lib.CFG_NO_RESIDENT if engine == 'streaming' else 0) | (_lib.CFG_ALWAYS_RESIDENT if engine == 'resident' else 0) \
            | (_lib.CFG_RECOMPUTE if self.recompute else 0) | (_lib.CFG_NO_GROT if no_grot else 0) | (_lib.CFG_ADJOINT64 if self.adjoint64 else 0)
        self.ctx.check(self.lib.bdof_configure(self.h, self.ny, self.nx, self.n_slice, self.batch_max, flags))
        if b > 1:           # (1 is what bdof_configure leaves)
            self.ctx.check(self.lib.bdof_set_slice_binning(self.h, b))
        self._reset_host_state()        # after bdof_configure, never before: it puts the ctx's data term back through the library (set_loss)

    # Host state: what the setters below record on the instance; before that, and after _reset_host_state(), as declared here.
    optics = None               # util.Optics of set_physics
    variant = k = None
    det_mode, det_kernel = _lib.DET_NONE, 'TF'
    _far_phase = None
    _conv_kernel = None         # (ky, kx, e) of set_conv; None: the transfer-function propagator only
    _conv_k64 = None
    _probe_args = None          # (real, imag) of set_probe: re-issued when the physics or the propagator change
    probe_stack, probe_gain = False, 1.0
    meas_ref = 0.0
    tf_f64 = conv_f64 = False
    _gprobe = None              # enable_probe_grad
    probe_modes = None          # set_probe_modes: the complex64 (M, Y, X) modes in force; None: the one probe of set_probe
    residual_split = True       # False: amplitudes go to the device as they are (a probe that changes between steps)
    loss_type, poisson_multiplier = 'lsq', 2e6      # set_loss
    detector_weights = None     # set_detector_weights: the (Y, X) float32 plane; None: every pixel counts alike
    n_planes = 1                # detector planes per wavefield (set_physics with a sequence of distances)

    def _reset_host_state(self):
        for name in set(vars(self)) & set(vars(MultisliceEngine)):
            delattr(self, name)
        self._keep = {}         # device buffers that must outlive the calls that registered them
        self.set_loss()         # the one setting that is sticky on the ctx itself (it survives bdof_configure): as declared, too

    # ---- data term -----------------------------------------------------------------------------
    def set_loss(self, kind='lsq', multiplier=2e6):
        """The data term loss_grad minimises (bdof_set_loss, include/bdof.h): 'lsq', mean((|d| - m)^2), or 'poisson', the
        photon-counting likelihood's deviance mean(mu (|d|^2 - m^2 - 2 m^2 ln(|d| / m))) with mu = multiplier photons per unit
        intensity (tensorflow_recon/ptychography.py's poisson_multiplier).  Transfer-function propagator only: under 'poisson'
        loss_grad(conv=True) and the tiled propagator's field loss raise."""
        check_loss(kind, multiplier)
        self.ctx.check(self.lib.bdof_set_loss(self.h, _LOSS[kind], float(multiplier)))
        self.loss_type, self.poisson_multiplier = kind, float(multiplier)

    def set_detector_weights(self, w):
        """Detector weights (bdof_set_detector_weights, include/bdof.h): one plane w >= 0 for every measurement of the run, in
        L = sum(w l) / (number of pixels) and G(d) = w (the seed) — 0 for dead and hot pixels, a beamstop, module gaps.  w is
        (Y, X) in the orientation of one measured frame (the far field fftshifted, as the data are) and is laid out as
        meas_layout lays out a frame; None clears the weights, and w == 1 everywhere gives the bits of no weights.  Where
        w == 0 meas_layout puts the amplitude to 0, whatever the data hold there (NaN, inf, a saturated count), and
        choose_residual_split looks at the other pixels only: amplitudes laid out BEFORE this call must be laid out again
        (meas_layout) after it.  Call it after set_physics (the detector decides the layout).  Transfer-function propagator
        only: with weights set loss_grad(conv=True) and the tiled propagator's field loss raise."""
        if w is None:
            self.ctx.check(self.lib.bdof_set_detector_weights(self.h, None))
            self.detector_weights = None
            return
        w = check_detector_weights(w, self.ny, self.nx)
        laid_out = self._plane_layout(w)            # (named: it has to outlive the call that reads its address)
        self.ctx.check(self.lib.bdof_set_detector_weights(self.h, _hp(laid_out)))
        self.detector_weights = w

    def _plane_layout(self, p):
        """(..., Y, X) planes in the index order of the loss kernels: transposed, or un-shifted in the far field."""
        if self.det_mode == _lib.DET_FAR:
            return np.ascontiguousarray(np.fft.ifftshift(p, axes=(-2, -1)))
        return np.ascontiguousarray(np.swapaxes(p, -2, -1))

    # ---- physics -------------------------------------------------------------------------------
    def set_physics(self, energy_ev, psize_cm, free_prop_cm=None, variant='numpy_skip_last', pi=util.PI, field_shape=None,
                    detector_kernel='TF'):
        """k and H exactly as cnn_propagator/np_funcs.py:19-32,45-57 derive them from energy / pixel size.  field_shape: this
        engine's wavefields are tiles of a (FY, FX) field and apply that field's propagator (util.get_kernel_tile).
        detector_kernel: 'TF' (what np_funcs.py:55 forces), 'IR' (get_kernel_ir, np_funcs.py:59-61) or 'auto' (the sampling
        criterion of np_funcs.py:51-53) for the step to a detector at a finite distance.
        free_prop_cm as a sequence of D distances: D detector planes per wavefield (bdof_set_detector_planes, include/bdof.h),
        each with the table of its own distance and the one detector_kernel, 'TF' or 'IR'.  forward then returns (B, D, Y, X)
        and loss_grad takes amplitudes of that shape; n_planes = D.  A sequence of one is its scalar.  Streaming and generic
        engines with the tape, scalar-carrier probes."""
        n_planes = check_model_options(free_prop_cm=free_prop_cm, propagator='fft' if self._conv_kernel is None else 'conv',
                                       recompute=self.recompute, adjoint64=self.adjoint64, detector_kernel=detector_kernel)
        o = util.Optics(energy_ev, psize_cm, free_prop_cm, pi, self.ny, self.nx, field_shape)
        if n_planes > 1:
            if field_shape is not None:
                raise ValueError('several detector planes: not for the tiles of a larger field (field_shape)')
            if self._probe_args is not None and self._wants_probe_stack(self._scalar_carrier(self._probe_field(), n_planes), o):
                raise ValueError('several detector planes run with a scalar carrier: this probe rides on a carrier field (set_probe)')
        det_mode = _lib.DET_NONE if free_prop_cm is None else _lib.DET_FAR if o.det_nm is None else _lib.DET_NEAR
        det_kernel = 'TF'
        if det_mode == _lib.DET_NEAR:
            det_kernel = util.detector_kernel_kind(detector_kernel, o.det_nm, o.lmbda_nm, o.voxel_nm, (self.ny, self.nx))
        self.optics, self.variant, self.k = o, variant, o.k       # (a refused argument has raised by now: the old physics stay whole)
        self.det_mode, self.det_kernel, self.n_planes = det_mode, det_kernel, n_planes
        hs64 = o.table(self._step_nm(), tiled=True, dtype=np.complex128)  # the slice step (of slice_binning voxels) honours field_shape ...
        hs = hs64.astype(np.complex64)
        h00 = o.dc(self._step_nm(), tiled=True)
        hdet00 = o.dc(o.det_nm, det_kernel) if det_mode == _lib.DET_NEAR else None
        hdet = self._detector_table(np.complex64)                          # ... the detector step does not
        self.tf_f64 = self.conv_f64 = False     # a float64 twin bound before this call held the previous tables
        # tf_all + far field: the last transfer-function step only multiplies the far field by the
        # unit-modulus H (F P phi = H . F phi); libbdof skips it and the host applies it to returned waves
        self._far_phase = None
        if self.det_mode == _lib.DET_FAR and variant == 'tf_all':
            self._far_phase = (hs.astype(np.complex128) * (self.nx * self.ny)).astype(np.complex64)
        self.ctx.check(self.lib.bdof_set_physics(self.h, o.k, hs.ctypes.data, _hp(hdet), h00.ctypes.data, _hp(hdet00),
                                                 self.det_mode, _VARIANT[variant]))
        # the same table in float64: the streaming kernels multiply by dithered float32 copies of it (bdof_set_transfer_f64)
        self.ctx.check(self.lib.bdof_set_transfer_f64(self.h, hs64.ctypes.data))
        if n_planes > 1:        # (bdof_set_physics has put the ctx back to one plane)
            tables = np.ascontiguousarray(np.stack([o.table(d, det_kernel) for d in o.det_planes_nm]))
            dcs = np.ascontiguousarray(np.stack([o.dc(d, det_kernel) for d in o.det_planes_nm]))
            if self.lib.bdof_probe_stack_supported(self.h) == 1:
                self.ctx.check(self.lib.bdof_set_probe_stack(self.h, None, None))      # the re-issued probe below rides on a scalar
            self.ctx.check(self.lib.bdof_set_detector_planes(self.h, n_planes, tables.ctypes.data, dcs.ctypes.data))
        if self.adjoint64:
            hd64 = self._detector_table(np.complex128)
            self.ctx.check(self.lib.bdof_set_physics_f64(self.h, hs64.ctypes.data, _hp(hd64)))
        if self._probe_args is not None:
            self.set_probe(*self._probe_args)      # the carrier (field, calibration) of the probe depends on the physics
        if self.probe_modes is not None:           # (bdof_set_physics has dropped the modes: their carriers were the old physics')
            self.set_probe_modes(self.probe_modes.real, self.probe_modes.imag)
        if self.detector_weights is not None:
            self.set_detector_weights(self.detector_weights)      # the detector decides the plane's index order

    def _step_nm(self):
        """Length of one propagation step: slice_binning voxel slices."""
        return self.optics.delta_nm * self.slice_binning

    def _admit(self, method):
        """A method that steps off the main path, under the options this engine runs with (OPTION_NEEDS, 'method')."""
        if self.slice_binning > 1:
            check_option_path('binning', dict(PATH, method=method))
        if self.n_planes > 1:
            check_option_path('planes', dict(PATH, method=method))

    def _detector_table(self, dtype, fold=True, transpose=False, tiled=False):
        """The un-shifted multiplier of the step to a near-field detector (None without one): the one place it is built.
        fold: 1/(nx*ny) folded in (the sweeps' tables) or not (the carrier fields').  tiled: honour field_shape, which only
        bdof_set_probe_field's table does, and only as 'TF'; every other caller takes the (ny, nx) mesh's own."""
        if self.det_mode != _lib.DET_NEAR:
            return None
        o = self.optics
        return o.table(o.det_nm, self.det_kernel, tiled and self.det_kernel == 'TF', fold, transpose, dtype)

    def _probe_field(self, round_c64=True):
        """The (ny, nx) probe of set_probe.  round_c64: rounded to complex64 as the reference's wavefront is (np_funcs.py:20-21)
        — set_probe and enable_tf_f64; enable_conv_f64 hands the float64 values over as they are."""
        pr, pi = self._probe_args
        probe = (np.asarray(pr) + 1j * np.asarray(pi)) * np.ones((self.ny, self.nx))
        return probe.astype(np.complex64) if round_c64 else probe

    def probe_arrays(self):
        """(real, imag) of the probe in force, as set_probe was given them; None before any set_probe"""
        return None if self._probe_args is None else tuple(np.array(a, copy=True) for a in self._probe_args)

    def _probe_stack(self, probe_c64):
        """The probe propagated through free space to the entrance of every slice and to the detector, in float64 on the
        host (np_funcs.py:42-61 without an object) — the carrier field of bdof_set_probe_stack (include/bdof.h)."""
        o = self.optics
        h = o.table(self._step_nm(), tiled=False, fold=False, dtype=np.complex128)      # this cross-check: the (ny, nx) mesh's own get_kernel
        p = probe_c64.astype(np.complex128)
        stack = np.empty((self.n_steps, self.nx, self.ny), dtype=np.complex64)
        for z in range(self.n_steps):
            stack[z] = p.T
            if z < self.n_steps - 1:
                p = np.fft.ifft2(np.fft.fft2(p) * h)
        if self.det_mode == _lib.DET_FAR:
            det = np.fft.fft2(p)                      # un-shifted, un-normalised; a tf_all step before it is applied on the host
        else:
            if self.variant == 'tf_all':
                p = np.fft.ifft2(np.fft.fft2(p) * h)
            if self.det_mode == _lib.DET_NEAR:
                p = np.fft.ifft2(np.fft.fft2(p) * self._detector_table(np.complex128, fold=False))
            det = p
        return np.ascontiguousarray(stack), np.ascontiguousarray(det.T.astype(np.complex64))

    def _probe_field_device(self, probe_c64):
        """The same carrier field computed by the library on the device in float64 (bdof_set_probe_field): the host only forms
        the two transfer functions (float64, transposed to [kx][ky]); both honour field_shape."""
        o = self.optics
        hT = o.table(self._step_nm(), tiled=True, fold=False, transpose=True, dtype=np.complex128)
        hdT = self._detector_table(np.complex128, fold=False, transpose=True, tiled=True)
        p = np.ascontiguousarray(probe_c64.T.astype(np.complex128))
        self.ctx.check(self.lib.bdof_set_probe_field(self.h, p.ctypes.data, hT.ctypes.data, _hp(hdT)))

    def set_probe(self, probe_real, probe_imag):
        previous, self._probe_args = self._probe_args, (np.array(probe_real, copy=True), np.array(probe_imag, copy=True))
        probe = self._probe_field()
        # Carrier splitting: the wave is held as carrier + eps and only eps runs through the float32 transforms.
        #  - a (nearly) uniform probe rides on its mean a0, propagated exactly as a scalar inside the library;
        #  - a localised probe rides on its own free-space propagation, a carrier FIELD per slice, which the library computes
        #    on the device in float64 (bdof_set_probe_field): eps is the scattered wave alone;
        #  - otherwise (BDOF_NO_PROBE_STACK, the real-space propagator) a0 = 0 and the whole wave is float32.
        a0 = self._scalar_carrier(probe, self.n_planes)
        use_stack = self._wants_probe_stack(a0, self.optics)
        if use_stack and self.n_planes > 1:        # (nothing has changed: the engine keeps the probe it had)
            self._probe_args = previous
            raise ValueError('several detector planes run with a scalar carrier: this probe rides on a carrier field')
        self.tf_f64 = self.conv_f64 = False     # the float64 twins (enable_tf_f64 / enable_conv_f64) hold the previous probe
        self.probe_stack = False
        if self._conv_kernel is not None and self.optics is not None:
            if self._set_conv_probe_stack(probe, a0):
                return
        if use_stack:
            if os.environ.get('BDOF_HOST_PROBE_STACK'):                     # cross-check: the float64 propagation on the host
                stack, det = self._probe_stack(probe)
                self._set_zero_probe()
                self.ctx.check(self.lib.bdof_set_probe_stack(self.h, stack.ctypes.data, det.ctypes.data))
            else:
                self._probe_field_device(probe)
            self.probe_stack, self.probe_gain = True, 1.0
            self._set_meas_mode(0j)
            return
        if self.lib.bdof_probe_stack_supported(self.h) == 1:
            self.ctx.check(self.lib.bdof_set_probe_stack(self.h, None, None))
        self.probe_gain = 1.0
        eps = np.ascontiguousarray((probe.astype(np.complex128) - a0).T.astype(np.complex64))
        self.ctx.check(self.lib.bdof_set_probe(self.h, eps.ctypes.data, a0.real, a0.imag))
        self._set_meas_mode(a0)

    @staticmethod
    def _scalar_carrier(probe, n_planes=1):
        """The scalar a (nearly) uniform probe rides on, its mean; 0 for any other probe.  Nearly uniform: no pixel further from
        the mean than a quarter of it.  With several detector planes, which have no carrier field to fall back on, the deviation
        is taken in RMS: a structured probe around a dominant mean (noise of 10 % on a plane wave, whose extreme pixels pass
        the quarter) still rides on its mean — exact algebra for any scalar, and the part left to the float32 transforms is
        small against the wave — and only a probe without a dominant mean (a localised one, a Gaussian) comes back as 0."""
        mean = complex(probe.astype(np.complex128).mean())
        dev = np.abs(probe - mean)
        spread = dev.max() if n_planes == 1 else float(np.sqrt(np.mean(dev.astype(np.float64) ** 2)))
        return mean if spread <= 0.25 * abs(mean) else 0j

    def _wants_probe_stack(self, a0, optics):
        """Whether set_probe puts a probe of scalar carrier a0 on a carrier FIELD under these optics."""
        return (a0 == 0 and optics is not None and not os.environ.get('BDOF_NO_PROBE_STACK')
                and self._conv_kernel is None                          # the real-space propagator has its own carrier
                and self.n_steps * self.nx * self.ny <= (1 << 32)      # 32 GiB of stack at most
                and self.lib.bdof_probe_stack_supported(self.h) == 1)

    def _set_zero_probe(self):
        """bdof_set_probe with nothing in it: the wave is a carrier field's, or a caller's."""
        zero = np.zeros((self.nx, self.ny), dtype=np.complex64)
        self.ctx.check(self.lib.bdof_set_probe(self.h, zero.ctypes.data, 0.0, 0.0))

    def _set_conv_probe_stack(self, probe, a0):
        """Real-space propagator with a probe that has no dominant constant part (a0 == 0, e.g. a ptychography probe): the
        carrier FIELD of bdof_set_conv_probe_stack — the probe carried through empty space by the padded convolution itself,
        in float64 on the host — so that only the scattered wave runs through the float32 convolutions and the residual
        |d| - m is taken in float64.  Returns True if the stack was set (False: scalar carrier, stack removed)."""
        lib, h = self.lib, self.h
        small = (self.n_slice + 1) * self.nx * self.ny <= (1 << 28)
        if a0 != 0 or not small or os.environ.get('BDOF_NO_PROBE_STACK'):
            self.ctx.check(lib.bdof_set_conv_probe_stack(h, None, None, 0., 0., 0., 0.))
            return False
        planes = util.conv_probe_stack(probe.astype(np.complex128), *self._conv_kernel, self.n_slice)     # (S + 1, Y, X)
        p_end = planes[-1]
        if self.det_mode == _lib.DET_FAR:
            det = np.fft.fft2(p_end)                                                                   # [ky][kx], un-shifted
        elif self.det_mode == _lib.DET_NEAR:
            det = np.fft.ifft2(np.fft.fft2(p_end) * self._detector_table(np.complex128, fold=False)).T    # [x][y]
        else:
            det = p_end.T
        stack = np.ascontiguousarray(planes.transpose(0, 2, 1).astype(np.complex64))                   # [S + 1][x][y]
        det = np.ascontiguousarray(det.astype(np.complex128))
        if lib.bdof_probe_stack_supported(h) == 1:
            self.ctx.check(lib.bdof_set_probe_stack(h, None, None))
        self._set_zero_probe()
        p0, ps = complex(planes[0][0, 0]), complex(p_end[0, 0])
        self.ctx.check(lib.bdof_set_conv_probe_stack(h, stack.ctypes.data, det.ctypes.data, p0.real, p0.imag, ps.real, ps.imag))
        self.probe_stack, self.probe_gain = False, 1.0
        self._set_meas_mode(0j)
        return True

    # ---- probe modes (bdof_set_probe_modes, include/bdof.h) --------------------------------------------------------------
    def set_probe_modes(self, probe_real, probe_imag):
        """M mutually incoherent probe modes, (M, Y, X) arrays: the data term then fits sqrt(sum_m |d_m|^2) (partial coherence;
        modes.py).  They take the place of set_probe's probe until set_probe_modes(None, None) removes them.  With modes set B of
        forward and loss_grad stays the number of windows and batch_max counts wavefields, B M <= batch_max; forward returns
        (M, B, Y, X) and probe_grad (M, Y, X).  Resident and generic engines, transfer-function propagator, one step per voxel
        slice, one detector plane, float32 sweeps with the tape; call it after set_physics."""
        if probe_real is None:
            self.ctx.check(self.lib.bdof_set_probe_modes(self.h, 0, None, None, None))
            self.probe_modes = None
            if self._probe_args is not None:
                self.set_probe(*self._probe_args)      # (the residual splitting of a plane-wave probe comes back with it)
            return
        modes = probe_modes_mod.as_modes(probe_real, probe_imag)
        if modes.shape[1:] != (self.ny, self.nx):
            raise ValueError('probe modes must be (M, {}, {}), not {}'.format(self.ny, self.nx, modes.shape))
        probe_modes_mod.check_probe_modes(modes.shape[0], propagator='fft' if self._conv_kernel is None else 'conv', slice_binning=self.slice_binning,
                                          adjoint_precision='float64' if self.adjoint64 else None)
        if self.optics is None:
            raise RuntimeError('set_physics first')
        if self.n_planes > 1:
            raise ValueError('probe modes run with one detector plane')
        o = self.optics
        hT = o.table(self._step_nm(), tiled=True, fold=False, transpose=True, dtype=np.complex128)
        hdT = self._detector_table(np.complex128, fold=False, transpose=True, tiled=True)
        modes = modes.astype(np.complex64)             # as set_probe rounds its one (np_funcs.py:20-21)
        p = np.ascontiguousarray(modes.transpose(0, 2, 1).astype(np.complex128))
        self.ctx.check(self.lib.bdof_set_probe_modes(self.h, modes.shape[0], p.ctypes.data, hT.ctypes.data, _hp(hdT)))
        self.probe_modes = modes
        self._set_meas_mode(0j)                        # no scalar carrier under modes: plain amplitudes

    @property
    def n_modes(self):
        return 0 if self.probe_modes is None else self.probe_modes.shape[0]

    # ---- gradient w.r.t. the probe (probe_type='optimizable', tensorflow_recon/fullfield.py:311-327) -------------------
    def enable_probe_grad(self, on=True):
        self.ctx.check(self.lib.bdof_enable_probe_grad(self.h, int(bool(on))))
        self._gprobe = DeviceBuffer.zeros(self.ctx, (self.nx, self.ny), np.complex64) if on else None

    def probe_grad(self, accumulate=False, to_host=True):
        """dL/d(probe_real) + i dL/d(probe_imag) of the last loss_grad, summed over its wavefields: (Y, X) complex — with probe
        modes (M, Y, X), one gradient per mode.  to_host=False: the device accumulator itself, [x][y] per plane."""
        if self.probe_modes is not None:
            shape = (self.n_modes, self.nx, self.ny)
            if self._gprobe.shape != shape:            # (enabled before the modes were set, or their number changed)
                self._gprobe = DeviceBuffer.zeros(self.ctx, shape, np.complex64)
            self.ctx.check(self.lib.bdof_probe_grad_modes(self.h, self._gprobe.ptr, int(bool(accumulate))))
        else:
            if self._gprobe.shape != (self.nx, self.ny):
                self._gprobe = DeviceBuffer.zeros(self.ctx, (self.nx, self.ny), np.complex64)
            self.ctx.check(self.lib.bdof_probe_grad(self.h, self._gprobe.ptr, int(bool(accumulate))))
        if not to_host:
            return self._gprobe
        self.ctx.sync()
        return np.ascontiguousarray(np.swapaxes(self._gprobe.download(), -2, -1))

    def set_probe_none(self):
        """No probe of the ctx's own: every wavefield starts from a caller-supplied field (bdof_forward_range), no carrier."""
        self._probe_args = None
        self._set_zero_probe()
        self.ctx.check(self.lib.bdof_set_probe_stack(self.h, None, None))
        self.probe_stack, self.probe_gain = False, 1.0
        self._set_meas_mode(0j)

    def _set_meas_mode(self, a0):
        """Residual splitting at the detector (include/bdof.h, bdof_set_meas_mode): with a plane-wave carrier and a real-space
        detector the measured amplitudes go to the device as m - |a0|.  The amplitudes a caller keeps resident on the device
        are laid out for the reference in force when they were uploaded (meas_layout), so a probe that is re-set between
        steps (probe_type='optimizable') must not move it: the solvers switch the splitting off for that case
        (residual_split = False) before they upload."""
        self.meas_ref = 0.0
        if a0 != 0 and self.det_mode != _lib.DET_FAR and self.residual_split:
            self.meas_ref = abs(a0)
        self.ctx.check(self.lib.bdof_set_meas_mode(self.h, 1 if self.meas_ref else 0))

    def set_conv(self, energy_ev, psize_cm, kernel_size=17):
        """Switch the slice-to-slice step to the truncated real-space kernel of multislice_propagate_cnn
        (cnn_propagator/propagation.py:18-44): k uses numpy's pi there (:25), the kernel the reference's PI literal."""
        self._admit(_SET_CONV)
        o = util.Optics(energy_ev, psize_cm, None, np.pi, self.ny, self.nx)         # o.k: numpy's pi, unlike set_physics
        ky, kx, e = util.conv_kernel_separable(o.delta_nm, o.lmbda_nm, o.voxel_nm, (self.ny, self.nx), kernel_size)   # pi=util.PI
        ksum = e * ky.sum() * kx.sum()
        self._conv_kernel = (ky, kx, e)
        kyf, kxf = [np.ascontiguousarray(t.astype(np.complex64)) for t in (ky, kx)]
        self.ctx.check(self.lib.bdof_set_conv(self.h, kyf.ctypes.data, kxf.ctypes.data, int(kernel_size), e.real, e.imag,
                                              ksum.real, ksum.imag, o.k))
        # the taps in float64 as well: dithered copies, one per slice (include/bdof.h)
        ky64, kx64 = [np.ascontiguousarray(t.astype(np.complex128)) for t in (ky, kx)]
        self.ctx.check(self.lib.bdof_set_conv_taps_f64(self.h, ky64.ctypes.data, kx64.ctypes.data, float(e.real), float(e.imag)))
        self._conv_k64 = o.k
        if self._probe_args is not None:
            self.set_probe(*self._probe_args)      # the carrier (scalar or field) of the probe follows the propagator

    def enable_tf_f64(self):
        """The transfer-function model's loss + gradient entirely in float64 on this context (bdof_loss_grad_tf_f64;
        loss_grad(..., f64=True)): what the reference's autograd differentiates (np_funcs.py:15-65 in numpy float64).  The
        accuracy path of the first minibatch of an epoch (adjoint_precision='first-step') — no second engine — and a float64 twin
        of the fused kernels for tests.  Hands the probe and the transfer function(s) over in float64; call again after
        set_physics / set_probe."""
        self._admit(_TF_F64)
        if self.optics is None or self._probe_args is None:
            raise RuntimeError('set_physics and set_probe first')
        o = self.optics
        ht = o.table(o.delta_nm, tiled=True, transpose=True, dtype=np.complex128)       # set_physics' float64 table as [kx][ky]
        hd = self._detector_table(np.complex128, transpose=True)
        # the reference's wavefront starts as complex64 (np_funcs.py:20-21) and becomes complex128 at the first product
        probe = np.ascontiguousarray(self._probe_field().T.astype(np.complex128))
        self.ctx.check(self.lib.bdof_set_tf_f64(self.h, probe.ctypes.data, ht.ctypes.data, _hp(hd), float(o.k)))
        self.tf_f64 = True

    def enable_conv_f64(self):
        """The real-space propagator's loss + gradient entirely in float64 (bdof_loss_grad_conv_f64; loss_grad(..., conv=True,
        f64=True)): the accuracy path for the first minibatch of an epoch (adjoint_precision='first-step' / 'float64' with
        propagator='conv').  Square fields.  Hands the probe and the transform of the zero-padded
        ks x ks kernel over in float64 (overlap-save on the padded (N + ks - 1)^2 grid)."""
        self._admit(_CONV_F64)
        if self._conv_kernel is None or self._probe_args is None:
            raise RuntimeError('set_conv and set_probe first')
        if self.nx != self.ny:
            raise ValueError('the float64 real-space path takes square wavefields')
        ky, kx, e = self._conv_kernel
        ks = len(ky)
        m = self.nx + ks - 1
        kpad = np.zeros((m, m), dtype=np.complex128)
        kpad[:ks, :ks] = e * np.outer(ky, kx)                                    # K[p][q] = e ky[p] kx[q]   (numpy (Y, X) order)
        khat = np.ascontiguousarray((np.fft.fft2(kpad) / float(m * m)).T)       # [kx][ky]
        ksum = e * ky.sum() * kx.sum()
        probe = np.ascontiguousarray(self._probe_field(round_c64=False).T.astype(np.complex128))
        self.ctx.check(self.lib.bdof_set_conv_f64(self.h, probe.ctypes.data, khat.ctypes.data, ks, float(ksum.real), float(ksum.imag),
                                                  float(self._conv_k64)))
        hd = self._detector_table(np.complex128, transpose=True)                 # propagation.py:122-124: one transfer-function step
        self.ctx.check(self.lib.bdof_set_conv_f64_detector(self.h, _hp(hd)))
        self.conv_f64 = True

    # ---- object --------------------------------------------------------------------------------
    def set_object_batch(self, grid_delta_batch, grid_beta_batch):
        """Already rotated objects, (B, Y, X, S) each (the np_funcs.py:15 argument convention)."""
        rows = util.batch_to_rows(grid_delta_batch, grid_beta_batch)
        buf = DeviceBuffer.from_host(self.ctx, rows)
        self._keep['obj'] = buf
        self.ctx.check(self.lib.bdof_set_object(self.h, buf.ptr, rows.shape[0] * rows.shape[1] * rows.shape[2], self.ny, None, 0, 0))
        return buf

    def set_volume(self, vol_buf, n_rows, vol_ny, tab_buf, vol_nx, n_angles):
        """Un-rotated volume rows [n_rows = X*Z][vol_ny] pairs + rotation table [n_angles][S][vol_nx] (device).
        Must be called again after the volume memory changed (the modulation table is rebuilt)."""
        self._keep['obj'] = vol_buf
        self._keep['tab'] = tab_buf
        self.ctx.check(self.lib.bdof_set_object(self.h, _lib._ptr(vol_buf), int(n_rows), int(vol_ny), _lib._ptr(tab_buf), int(vol_nx), int(n_angles)))

    def modulation_table(self):
        """The table of modulation factors c - 1 the sweeps read (bdof_modulation_table, include/bdof.h), built if stale:
        (complex64 array of one entry per (delta, beta) pair in the bound object's order, complex mean c - 1 as the host
        carries it — of a bin with slice_binning > 1, 0 when no mean rides on the carrier)."""
        table, n, mean = _lib._vp(), ctypes.c_size_t(0), (ctypes.c_double * 2)()
        self.ctx.check(self.lib.bdof_modulation_table(self.h, ctypes.byref(table), ctypes.byref(n), mean))
        self.ctx.sync()
        out = np.empty(n.value, dtype=np.complex64)
        self.ctx.check(self.lib.bdof_memcpy_d2h(self.h, out.ctypes.data, table.value, out.nbytes))
        return out, complex(mean[0], mean[1])

    def set_rotation_adjoint(self, off_buf, order_buf, n_dest):
        self._keep['off'] = off_buf
        self._keep['order'] = order_buf
        self.ctx.check(self.lib.bdof_set_rotation_adjoint(self.h, _lib._ptr(off_buf), _lib._ptr(order_buf), int(n_dest)))

    # ---- forward -------------------------------------------------------------------------------
    def _wave_to_host(self, buf, B):
        if self.det_mode == _lib.DET_FAR:
            w = buf.download((B, self.ny, self.nx), np.complex64)        # un-shifted fft2, [b][ky][kx]
            if self._far_phase is not None:
                w = w * self._far_phase
            return np.ascontiguousarray(np.fft.fftshift(w, axes=(1, 2)))   # np_funcs.py:48
        if self.n_planes > 1:
            return np.ascontiguousarray(buf.download((B, self.n_planes, self.nx, self.ny), np.complex64).transpose(0, 1, 3, 2))
        return np.ascontiguousarray(buf.download((B, self.nx, self.ny), np.complex64).transpose(0, 2, 1))

    def _check_frames(self, meas_abs):
        """Amplitudes are (n, Y, X) frames, or (n, D, Y, X) with D == n_planes detector planes (D = 1: both forms)."""
        shape = np.shape(meas_abs)
        ok = shape[-2:] == (self.ny, self.nx) and (len(shape) == 4 and shape[1] == self.n_planes or len(shape) == 3 and self.n_planes == 1)
        if not ok:
            raise ValueError('amplitudes of shape {} do not fit {} detector plane(s) of {}: (n, {}Y, X)'.format(
                tuple(shape), self.n_planes, (self.ny, self.nx), 'D, ' if self.n_planes > 1 else ''))

    def choose_residual_split(self, meas_abs):
        """Decide, for the amplitudes about to be handed over, whether the residual stays split (bdof_set_meas_mode), and return
        meas_ref.  float32(m - |a0|) is finer than float32(m) only while the amplitudes stay near |a0|.  Behind an object that
        takes most of the wave away (|cbar|^S << 1: the carrier has died out, m << |a0|) it is coarser — at m = 1e-4 |a0| by
        three digits, which is then the error of every residual — so for amplitudes that lie closer to 0 than to |a0| on average
        the splitting is switched off, until the next set_probe.  Called where amplitudes are bound: loss_grad for an array it
        uploads itself, FullfieldSolver.set_measurements for the resident stack.  Everything laid out earlier with the other
        reference must be laid out again (meas_layout) after the mode changed."""
        self._check_frames(meas_abs)
        if self.meas_ref:
            m64 = np.asarray(meas_abs, dtype=np.float64)
            if self.detector_weights is not None:
                m64 = m64.reshape(-1, self.ny, self.nx)[:, self.detector_weights > 0]      # the pixels that count
            if m64.size and np.abs(m64 - self.meas_ref).mean() > np.abs(m64).mean():
                self.meas_ref = 0.0
                self.ctx.check(self.lib.bdof_set_meas_mode(self.h, 0))
        return self.meas_ref

    def meas_layout(self, meas_abs):
        """|measured| (n, Y, X) as libbdof's loss kernels read it under the mode in force: m - meas_ref (residual splitting; 0
        without it) rounded once to float32, in the kernels' index order.  Under detector weights the amplitude is 0 wherever
        w == 0, before anything else looks at it (0 NaN is NaN: the kernels could not keep such a pixel out).  Changes nothing
        on the engine.  With D detector planes the frames are (n, D, Y, X) and every plane shares the weights."""
        self._check_frames(meas_abs)
        if self.detector_weights is not None:
            meas_abs = np.where(self.detector_weights > 0, meas_abs, 0)
        if self.meas_ref:
            m = (np.asarray(meas_abs, dtype=np.float64) - self.meas_ref).astype(np.float32)      # subtract in float64, round once
        else:
            m = np.asarray(meas_abs, dtype=np.float32)
        return self._plane_layout(m)

    def _meas_to_device(self, meas_abs):
        self.choose_residual_split(meas_abs)
        return DeviceBuffer.from_host(self.ctx, self.meas_layout(meas_abs))

    def _idx_bufs(self, *lists):
        """Per-wavefield index lists (angle, xoff, yoff) as int32 on the device (None stays None)."""
        return [None if v is None else DeviceBuffer.from_host(self.ctx, np.asarray(v, dtype=np.int32)) for v in lists]

    def forward(self, B, angle_idx=None, xoff=None, yoff=None, keep_tape=False, to_host=True, conv=False):
        """The detector waves of B wavefields, (B, Y, X) — with D detector planes (B, D, Y, X), in the order of the distances; with
        M probe modes (set_probe_modes) of B windows (M, B, Y, X)."""
        D = self.n_planes
        if self.probe_modes is not None and not conv:
            M = self.n_modes                     # frames [M][B]: one detector wave per (mode, window)
            a, xo, yo = self._idx_bufs(angle_idx, xoff, yoff)
            out = DeviceBuffer(self.ctx, M * B * self.nx * self.ny * 8, np.complex64, (M * B, self.nx, self.ny))
            self.ctx.check(self.lib.bdof_forward(self.h, B, _lib._ptr(a), _lib._ptr(xo), _lib._ptr(yo), out.ptr, int(keep_tape)))
            self.ctx.sync()
            return self._wave_to_host(out, M * B).reshape(M, B, self.ny, self.nx) if to_host else out
        out = DeviceBuffer(self.ctx, B * D * self.nx * self.ny * 8, np.complex64, (B, self.nx, self.ny) if D == 1 else (B, D, self.nx, self.ny))
        a, xo, yo = self._idx_bufs(angle_idx, xoff, yoff)
        if conv:
            self._admit(_FORWARD_CONV)
            self.ctx.check(self.lib.bdof_forward_conv(self.h, B, _lib._ptr(a), _lib._ptr(xo), _lib._ptr(yo), out.ptr))
        else:
            self.ctx.check(self.lib.bdof_forward(self.h, B, _lib._ptr(a), _lib._ptr(xo), _lib._ptr(yo), out.ptr, int(keep_tape)))
        self.ctx.sync()
        return self._wave_to_host(out, B) if to_host else out

    def probe_array(self, B):
        """Per-step wavefields, (n_steps, B, Y, X) — the second return value of np_funcs.py:65 (n_steps = S without binning)."""
        out = DeviceBuffer(self.ctx, B * self.nx * self.ny * 8, np.complex64, (B, self.nx, self.ny))
        res = np.empty((self.n_steps, B, self.ny, self.nx), dtype=np.complex64)
        for i in range(self.n_steps):
            self.ctx.check(self.lib.bdof_tape_to_real(self.h, i, B, out.ptr))
            res[i] = out.download((B, self.nx, self.ny), np.complex64).transpose(0, 2, 1)
        return res

    # ---- loss + gradient -----------------------------------------------------------------------
    def loss_grad_device(self, B, angle, xoff, yoff, meas, conv=False, f64=False):
        """Enqueue forward + loss + adjoint of B wavefields; every array argument is a device pointer (or None).  The one
        place that picks among the four entry points: conv — the real-space propagator; f64 — the model's float64 path on
        this context, which takes the residual-splitting reference as a number."""
        if conv or f64:
            self._admit(_LOSS_GRAD_OFF)
        if f64:
            if conv and not self.conv_f64:
                raise RuntimeError('the real-space propagator\'s float64 path: enable_conv_f64() first')
            if not conv and not self.tf_f64:
                raise RuntimeError('the transfer-function model\'s float64 path: enable_tf_f64() first')
            fn, last = (self.lib.bdof_loss_grad_conv_f64 if conv else self.lib.bdof_loss_grad_tf_f64), float(self.meas_ref)
        else:
            fn, last = (self.lib.bdof_loss_grad_conv if conv else self.lib.bdof_loss_grad), None
        self.ctx.check(fn(self.h, B, angle, xoff, yoff, meas, last))

    def get_loss(self):
        """The loss of the last loss_grad_device (waits for it)."""
        loss = ctypes.c_double(0)
        self.ctx.check(self.lib.bdof_get_loss(self.h, ctypes.byref(loss)))
        return loss.value

    def loss_grad(self, B, meas_abs, angle_idx=None, xoff=None, yoff=None, meas_on_device=False, conv=False, f64=False):
        """Runs forward + loss + adjoint; returns the loss.  The gradient stays on the device.  f64: the float64 path of the
        model on the same context (enable_tf_f64 / with conv: enable_conv_f64)."""
        m = meas_abs if meas_on_device else self._meas_to_device(meas_abs)
        a, xo, yo = self._idx_bufs(angle_idx, xoff, yoff)
        self.loss_grad_device(B, _lib._ptr(a), _lib._ptr(xo), _lib._ptr(yo), _lib._ptr(m), conv=conv, f64=f64)
        loss = self.get_loss()
        self._keep['last_idx'] = (a, xo, yo, m)
        return loss

    def adjoint_carrier(self, B):
        """(gcar, gt0), complex128 [B]: the float64 DC-bin seed per wavefield and conj(a_end) times it, as the last loss_grad left
        them (bdof_adjoint_carrier) — or None where the configuration does not carry the DC seed as a scalar."""
        gcar, gt0 = np.zeros(B, dtype=np.complex128), np.zeros(B, dtype=np.complex128)
        r = self.lib.bdof_adjoint_carrier(self.h, int(B), _hp(gcar), _hp(gt0))
        if r < 0:
            self.ctx.check(r)
        return (gcar, gt0) if r == 1 else None

    def grad_batch_to_host(self, B):
        """Gradient w.r.t. the rotated object batch: (g_delta, g_beta), each (B, Y, X, S)."""
        n = B * self.n_slice * self.nx * self.ny
        out = np.empty((B, self.n_slice, self.nx, self.ny, 2), dtype=np.float32)
        self.ctx.check(self.lib.bdof_memcpy_d2h(self.h, out.ctypes.data, self.lib.bdof_grot(self.h), n * 8))
        return util.rows_to_batch(out)

    def rotation_adjoint(self, B, angle_idx, gvol_buf, accumulate=False, scale=1.0):
        a, = self._idx_bufs(angle_idx)
        self.ctx.check(self.lib.bdof_rotation_adjoint(self.h, B, a.ptr, _lib._ptr(gvol_buf), int(accumulate), float(scale)))
        self.ctx.sync()

    def adam_step(self, x_old, x_new, g, m, v, mask, shape_xzy, i_batch, lr, g_scale=1.0, alpha_d=0.0, alpha_b=0.0,
                  gamma=0.0, b1=0.9, b2=0.999, eps=1e-8, clip=True, slab=None):
        """slab = (x0, nx): update only that range of x-planes (pipelined with the gradient all-reduce)."""
        nxv, nzv, nyv = [int(s) for s in shape_xzy]
        x0, nx = (0, nxv) if slab is None else (int(slab[0]), int(slab[1]))
        self.ctx.check(self.lib.bdof_adam_step_slab(self.h, _lib._ptr(x_old), _lib._ptr(x_new), _lib._ptr(g), _lib._ptr(m),
                                                    _lib._ptr(v), _lib._ptr(mask), nxv, nzv, nyv, g_scale, alpha_d, alpha_b,
                                                    gamma, lr, b1, b2, eps, int(i_batch), int(clip), x0, nx))

    def stream_ptr(self):
        return int(self.lib.bdof_stream(self.h) or 0)

    # ---- profiling -----------------------------------------------------------------------------
    def set_streams(self, n=-1):
        """Number of concurrent sub-batches of the fused FFT engine (-1: automatic, see include/bdof.h)."""
        self.ctx.check(self.lib.bdof_set_streams(self.h, int(n)))

    def batch_groups(self, B):
        return int(self.lib.bdof_batch_groups(self.h, int(B)))

    def set_sweep_fusion(self, mode):
        """Fused forward sweep of loss_grad (bdof_set_sweep_fusion, include/bdof.h): 0 never, 1 the forward sweep; 2 is accepted and
        runs 1, the highest stage this switch carries (the fused adjoint sweep has a switch of its own, set_adjoint_fusion).  An
        engine starts at 0, so that its results stay bit for bit those of the tape-free adjoint's forward sweep; FullfieldSolver
        switches to 1.  Ineligible configurations run the two-kernel sweep."""
        self.ctx.check(self.lib.bdof_set_sweep_fusion(self.h, int(mode)))

    def set_adjoint_fusion(self, on=True):
        """Fused adjoint sweep of loss_grad (bdof_set_adjoint_fusion): one kernel per slice below the top one, wherever the fused
        forward sweep runs (set_sweep_fusion(1) and an eligible configuration).  An engine starts with it off."""
        self.ctx.check(self.lib.bdof_set_adjoint_fusion(self.h, 1 if on else 0))

    @property
    def adjoint_fused(self):
        """1 if the last loss_grad ran the fused adjoint sweep (bdof_adjoint_fused)."""
        return int(self.lib.bdof_adjoint_fused(self.h))

    @property
    def sweep_fused(self):
        """The mode the last loss_grad actually ran (bdof_sweep_fused): 0 = the two-kernel sweep."""
        return int(self.lib.bdof_sweep_fused(self.h))

    def profile_enable(self, on=True, stride=1):
        self.ctx.check(self.lib.bdof_profile_enable(self.h, int(stride) if on else 0))

    def profile_read(self):
        res = {}
        for cls, name in enumerate(_lib.KERNEL_CLASS_NAMES):
            n = ctypes.c_int(0)
            ms = ctypes.c_double(0)
            self.ctx.check(self.lib.bdof_profile_read(self.h, cls, ctypes.byref(n), ctypes.byref(ms)))
            res[name] = (n.value, ms.value)
        return res

    def sync(self):
        self.ctx.sync()
