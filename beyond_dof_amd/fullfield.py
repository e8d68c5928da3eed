"""reconstruct_fullfield — drop-in for cnn_propagator/fullfield.py:19-392 with the forward + gradient loop on
the GPU (libbdof.so).  Same keyword surface (unknown keywords are accepted and ignored, as the reference's
**kwargs does), same input file (`exchange/data` HDF5), same outputs (delta_ds_*.tiff, beta_ds_*.tiff,
intermediate/current.tiff, summary.txt).

Differences, all deliberate:
  * by default the multislice forward is the FFT propagator of np_funcs.py (what BASELINE.json's north_star names);
    pass propagator='conv' for the truncated real-space convolution of propagation.py that the reference calls here
    (then `kernel_size` is honoured);
  * Q7: the index list is padded with its first entries (the reference's np.concatenate call is malformed);
  * Q8: shrink-wrap runs as intended (mask *= delta > 1e-15 once i_epoch >= shrink_cycle);
  * Q12: the per-minibatch TIFF dump is behind save_intermediate;
  * n_epochs='auto' stops when the loss reduction rate falls below crit_conv_rate or at max_nepochs
    (the reference loops forever in that case, fullfield.py:376-377);
  * a missing finite-support mask means "no mask" instead of a Paganin reconstruction from files that do not exist.
"""
import os
import struct
import time

import numpy as np

from . import analytic, h5io, resolution, tiffio, util
from .comm import get_comm, minibatch_schedule
from .misc import create_summary, SUMMARY_PRESET_FF, SUMMARY_GEOMETRY, SUMMARY_ANALYTIC
from .engine import check_model_options, read_detector_weights
from .rotation import check_refine
from .solver import FullfieldSolver
from .util import print_flush

PI = util.PI


upsample_2x = util.upsample_2x      # cnn_propagator/util.py:350-360


def create_probe_initial_guess(data_fname, dist_nm, energy_ev, psize_nm):
    """cnn_propagator/util.py:405-415 (including its 1.24/energy wavelength)."""
    dat = h5io.read_dataset(data_fname)
    wavefront = np.mean(np.abs(dat), axis=0)
    lmbda_nm = 1.24 / energy_ev
    h = util.get_kernel(-dist_nm, lmbda_nm, [psize_nm, psize_nm], wavefront.shape)
    wavefront = np.fft.fftshift(np.fft.fft2(wavefront)) * h
    return np.fft.ifft2(np.fft.ifftshift(wavefront))


def _read_mask(save_path, n_slices):
    for loader in (lambda: tiffio.read_tiff_stack(os.path.join(save_path, 'fin_sup_mask', 'mask_00000.tiff'), range(n_slices), 5),
                   lambda: tiffio.read_tiff(os.path.join(save_path, 'fin_sup_mask', 'mask.tiff'))):
        try:
            return np.asarray(loader(), dtype=np.float32)
        except (IOError, OSError, KeyError, ValueError, IndexError, struct.error):      # missing or not a TIFF we can parse
            continue
    return None


def reconstruct_fullfield(fname, theta_st=0, theta_end=PI, n_epochs='auto', crit_conv_rate=0.03, max_nepochs=200,
                          alpha=1e-7, alpha_d=None, alpha_b=None, gamma=1e-6, learning_rate=1.0,
                          output_folder=None, minibatch_size=None, save_intermediate=False, full_intermediate=False,
                          energy_ev=5000, psize_cm=1e-7, n_epochs_mask_release=None, cpu_only=False, save_path='.',
                          phantom_path='phantom', shrink_cycle=20, core_parallelization=True, free_prop_cm=None,
                          multiscale_level=1, n_epoch_final_pass=None, initial_guess=None, n_batch_per_update=5,
                          dynamic_rate=True, probe_type='plane', probe_initial=None, probe_learning_rate=1e-3,
                          pupil_function=None, theta_downsample=None, forward_algorithm='fresnel', random_theta=True,
                          object_type='normal', kernel_size=17, debug=False, loss_type='lsq', poisson_multiplier=2e6, slice_binning=1,
                          detector_weights=None, fsc_reference=None, fsc_threshold='half-bit', delta_beta_ratio=10.,
                          ctf_regularization=1e-2, write_support_mask=None, **kwargs):
    """Reconstruct a beyond-depth-of-focus object from full-field projections (see the module docstring and
    cnn_propagator/fullfield.py:28-77 for the parameters).  Returns (obj_delta, obj_beta) of the finest level.
    initial_guess='ctf-fbp': the first (coarsest) multiscale level starts from the analytic volume of
    FullfieldSolver.analytic_volume — CTF retrieval of all detector planes for a homogeneous object delta = delta_beta_ratio *
    beta, regularised by ctf_regularization, and a filtered back-projection through the level's own rotation — formed from that
    level's strided data with its voxel size; summary.txt gets the lines initial_guess, delta_beta_ratio and ctf_regularization.
    write_support_mask=threshold: rank 0 also writes analytic.support_mask(delta, threshold) of that start, brought to the full
    resolution, as <save_path>/fin_sup_mask/mask_*.tiff — after the last level and before the closing barrier, so no level of this
    run reads it (a mask that was there serves this run and is then replaced): it is for the NEXT run.  Any other string raises."""
    t_zero = time.time()
    analytic_start = isinstance(initial_guess, str)
    if analytic_start and initial_guess != 'ctf-fbp':
        raise ValueError("initial_guess takes None, the arrays [delta, beta] or 'ctf-fbp', not {!r}".format(initial_guess))
    if write_support_mask is not None:           # on every rank, before anything runs: rank 0 alone writes it, in front of a barrier
        if not analytic_start:
            raise ValueError("write_support_mask is formed from the analytic start: initial_guess='ctf-fbp'")
        if isinstance(write_support_mask, (str, bool)) or np.ndim(write_support_mask) != 0 or not np.isfinite(write_support_mask) \
                or write_support_mask < 0:
            raise ValueError('write_support_mask is a threshold on delta: one finite number >= 0, not {!r}'.format(write_support_mask))
        if not os.path.isdir(save_path) or not os.access(save_path, os.W_OK | os.X_OK):
            raise ValueError('write_support_mask: save_path {!r} is not a directory this run can write to'.format(save_path))
    comm = kwargs.get('comm') or get_comm()
    size, rank = comm.size, comm.rank
    seed = kwargs.get('seed', int(time.time() / 60))
    variant = kwargs.get('variant', 'numpy_skip_last')
    # 'fft' (default): transfer-function propagator of np_funcs.py; 'conv': truncated real-space kernel of propagation.py,
    # the reference's own choice in this entry point, with `kernel_size` taps per axis
    propagator = kwargs.get('propagator', 'fft')
    # 'float64': the adjoint sweep in float64 (bdof_configure flag 64, transfer-function propagator only) — follows the
    # reference's float64 loop voxel by voxel where float32's 3e-6 on the gradient is too coarse; 'first-step': the
    # first minibatch of every epoch (Adam's restart: the one step in which a float32 gradient shows) through the model's float64
    # path on the same context (bdof_loss_grad_tf_f64; needs room for a complex128 tape of one minibatch), the rest in float32
    adjoint_precision = kwargs.get('adjoint_precision', 'float32')
    if adjoint_precision not in ('float32', 'float64', 'first-step'):
        raise ValueError("adjoint_precision must be 'float32', 'float64' or 'first-step'")
    # 'lsq': mean((|d| - m)^2), the reference's active line; 'poisson': the photon-counting likelihood next to it in
    # tensorflow_recon/ptychography.py, as its deviance (include/bdof.h, bdof_set_loss), with poisson_multiplier photons per unit
    # intensity.  Near the fit it is ~ 2 poisson_multiplier times the least-squares term: rescale alpha_d / alpha_b / gamma with it.
    # detector_weights: one (Y, X) plane w >= 0 shared by every projection — 0 for dead or hot pixels and module gaps — as an array or
    # as the name of a dataset of the data file ('exchange/weights').  L = sum(w l) / (number of pixels), and a pixel with w = 0
    # takes no part whatever the file holds there (MultisliceEngine.set_detector_weights).
    # slice_binning=b: one propagation step per b voxel slices (include/bdof.h, bdof_set_slice_binning) — a step only has to stay
    # below the depth of focus; every multiscale level's depth must divide by b.
    # free_prop_cm=[z_0, ..]: D detector planes per angle (holotomography; include/bdof.h, bdof_set_detector_planes).  The file's
    # exchange/data is then (n_theta, D, Y, X), in the order of the distances; a sequence of one is its scalar.
    # What each of the four needs of propagator, adjoint precision, rotation and detector kernel: engine.OPTION_NEEDS.
    n_planes = check_model_options(loss_type, poisson_multiplier, detector_weights, slice_binning, free_prop_cm, propagator=propagator,
                                   adjoint_precision=kwargs.get('adjoint_precision'), rotation=kwargs.get('rotation', 'nearest'),
                                   detector_kernel=kwargs.get('detector_kernel', 'TF'))
    if n_planes > 1 and probe_type == 'optimizable' and probe_initial is None:
        raise ValueError("several detector planes with probe_type='optimizable' need probe_initial: the initial guess back-propagates one plane")
    # gradient accumulation over n_batch_per_update minibatches exists only in the TF twin (tensorflow_recon/fullfield.py:
    # 413-425); the cnn variant accepts the keyword and ignores it (default 5!), so it is opt-in here
    accumulate = bool(kwargs.get('accumulate_gradients', False))
    if analytic_start:                           # the host-side refusals, before the file is read (the probe's when the solver has it)
        analytic.check_analytic(propagator, None, None, delta_beta_ratio, ctf_regularization, object_type, free_prop_cm)
        if probe_type not in ('plane', 'fixed', 'optimizable'):
            raise ValueError("initial_guess='ctf-fbp' assumes a plane-wave probe: not with probe_type={!r}".format(probe_type))
    # 'nearest': the cnn variant's lookup tables over linspace(0, 2 pi) (quirk Q5); 'bilinear': the TF twin's tf_rotate with the true
    # angles theta = -linspace(theta_st, theta_end) (tensorflow_recon/fullfield.py:96,216); 'trilinear': a rigid map per angle
    # (FullfieldSolver) with the same theta and the geometry keywords of util.RotationKeywords
    geo = util.RotationKeywords(kwargs)
    rotation, trilinear = geo.rotation, geo.trilinear
    # refine_geometry=('center', 'axis_tilt', ...): the solver moves these with the volume (FullfieldSolver); what a multiscale level
    # reaches is the next level's start, and geometry.npy / summary.txt record it in full-resolution units
    check_refine(geo.refine, rotation, geo.rotation_matrices)
    if geo.refine and accumulate and n_batch_per_update > 1:
        raise ValueError('refine_geometry moves the geometry at every minibatch: not together with accumulate_gradients')

    print_flush('Reading data...', 0, rank)
    t0 = time.time()
    prj_0 = np.asarray(h5io.read_dataset(os.path.join(save_path, fname))).astype('complex64')
    if n_planes > 1 and (prj_0.ndim != 4 or prj_0.shape[1] != n_planes):
        raise ValueError('free_prop_cm holds {} detector planes: exchange/data must have the shape (n_theta, {}, Y, X), not {}'.format(
            n_planes, n_planes, prj_0.shape))
    if n_planes == 1 and prj_0.ndim == 4 and prj_0.shape[1] == 1:
        prj_0 = prj_0[:, 0]                    # one plane written as (n_theta, 1, Y, X)
    theta = -np.linspace(theta_st, theta_end, prj_0.shape[0], dtype='float32')
    weights_0 = read_detector_weights(detector_weights, os.path.join(save_path, fname), prj_0.shape[-2:])
    if theta_downsample is not None:
        prj_0 = prj_0[::theta_downsample]
        theta = theta[::theta_downsample]
    n_theta = len(theta)
    geo.select(n_theta, None if theta_downsample is None else slice(None, None, theta_downsample))
    original_shape = prj_0.shape
    print_flush('Data reading: {} s'.format(time.time() - t0), 0, rank)
    print_flush('Data shape: {}'.format(original_shape), 0, rank)

    if output_folder is None:
        output_folder = ('recon_360_minibatch_{}_mskrls_{}_shrink_{}_iter_{}_alphad_{}_alphab_{}_gamma_{}_rate_{}_energy_{}_'
                         'size_{}_ntheta_{}_prop_{}_ms_{}_cpu_{}').format(
            minibatch_size, n_epochs_mask_release, shrink_cycle, n_epochs, alpha_d, alpha_b, gamma, learning_rate, energy_ev,
            prj_0.shape[-1], prj_0.shape[0], free_prop_cm if n_planes == 1 else '_'.join(str(z) for z in free_prop_cm), multiscale_level, cpu_only)
        if abs(PI - theta_end) < 1e-3:
            output_folder += '_180'
    if save_path != '.':
        output_folder = os.path.join(save_path, output_folder)

    # regulariser weights: the alpha branch of fullfield.py:109-111 counts delta twice and never beta (quirk Q6)
    reg_d, reg_b = (2 * alpha, 0.0) if alpha_d is None else (alpha_d, alpha_b)

    for lv in range(multiscale_level):          # the depths without a mask, before any level has run (a mask's are checked per level)
        if len(range(0, prj_0.shape[-1], 2 ** lv)) % slice_binning:
            raise ValueError('slice_binning={} does not divide the depth of multiscale level {}'.format(slice_binning, 2 ** lv))

    # fsc_reference=(delta, beta), arrays or two .npy / TIFF paths: after the last level rank 0 compares the final resident volume
    # with it by Fourier shell correlation (resolution.py; nothing but the shell sums leaves the device), writes fsc.npy and adds the
    # lines resolution_delta / resolution_beta, at fsc_threshold ('half-bit', or a number such as 0.5 or 0.143), to summary.txt
    if fsc_reference is not None:
        resolution.threshold_curve(fsc_threshold, 1)
        final_mask = _read_mask(save_path, prj_0.shape[-2])
        fsc_reference = resolution.read_reference(fsc_reference, list(prj_0.shape[-2:]) + [final_mask.shape[-1] if final_mask is not None else prj_0.shape[-1]])
        del final_mask

    obj_delta = obj_beta = support_from = None
    first_level = True
    for ds_level in range(multiscale_level - 1, -1, -1):
        ds_level = 2 ** ds_level
        print_flush('Multiscale downsampling level: {}'.format(ds_level), 0, rank)
        prj = prj_0[..., ::ds_level, ::ds_level] if ds_level > 1 else prj_0
        dim_y, dim_x = prj.shape[-2:]
        weights = weights_0 if weights_0 is None or ds_level == 1 else weights_0[::ds_level, ::ds_level]      # strided as the data are
        if minibatch_size is None:
            minibatch_size = n_theta
        if n_epochs_mask_release is None:
            n_epochs_mask_release = np.inf

        mask = _read_mask(save_path, prj_0.shape[-2])
        full_z = mask.shape[-1] if mask is not None else prj_0.shape[-1]      # the depth at full resolution
        if mask is not None and ds_level > 1:
            mask = mask[::ds_level, ::ds_level, ::ds_level]
        dim_z = mask.shape[-1] if mask is not None else dim_x
        if dim_z % slice_binning:
            raise ValueError('slice_binning={} does not divide the depth {} of multiscale level {}'.format(slice_binning, dim_z, ds_level))

        np.random.seed(seed)          # same seed on every rank (fullfield.py:242-245)
        if first_level:
            if analytic_start:
                print_flush('Initializing with CTF retrieval and filtered back-projection.', 0, rank)
                obj_delta = obj_beta = np.zeros([dim_y, dim_x, dim_z])        # until the solver, which forms it, exists
            elif initial_guess is None:
                print_flush('Initializing with Gaussian random.', 0, rank)
                obj_delta = np.random.normal(size=[dim_y, dim_x, dim_z], loc=8.7e-7, scale=1e-7)
                obj_beta = np.random.normal(size=[dim_y, dim_x, dim_z], loc=5.1e-8, scale=1e-8)
            else:
                print_flush('Using supplied initial guess.', 0, rank)
                obj_delta, obj_beta = np.array(initial_guess[0], dtype=float), np.array(initial_guess[1], dtype=float)
        else:
            obj_delta = upsample_2x(obj_delta) + np.random.normal(size=[dim_y, dim_x, dim_z], loc=8.7e-7, scale=1e-7)
            obj_beta = upsample_2x(obj_beta) + np.random.normal(size=[dim_y, dim_x, dim_z], loc=5.1e-8, scale=1e-8)
        if mask is not None:
            obj_delta, obj_beta = obj_delta * mask, obj_beta * mask
        obj_delta, obj_beta = np.clip(obj_delta, 0, None), np.clip(obj_beta, 0, None)
        if object_type == 'phase_only':
            obj_beta[...] = 0
        elif object_type == 'absorption_only':
            obj_delta[...] = 0
        obj_size = obj_delta.shape

        if probe_type == 'point':
            # cnn_propagator/fullfield.py:298-301 fills in a plane wave for 'point' with the note "this should be in spherical
            # coordinates": the spherical-wave propagator is out of scope here (simulation.py refuses it too), and silently
            # reconstructing with the plane-wave one would be a different experiment
            raise ValueError("probe_type='point' (spherical-wave propagator) is not supported; use 'plane', 'fixed' or 'optimizable'")
        if probe_type == 'plane':
            probe_real, probe_imag = np.ones([dim_y, dim_x]), np.zeros([dim_y, dim_x])
        elif probe_type == 'optimizable':
            if probe_initial is not None:
                probe_real, probe_imag = util.mag_phase_to_real_imag(*probe_initial)
            else:
                back_prop_cm = (free_prop_cm + psize_cm * obj_size[2]) if free_prop_cm is not None else psize_cm * obj_size[2]
                probe_init = create_probe_initial_guess(os.path.join(save_path, fname), back_prop_cm * 1.e7, energy_ev, psize_cm * 1.e7)
                probe_real, probe_imag = probe_init.real, probe_init.imag
            if pupil_function is not None:
                probe_real, probe_imag = probe_real * pupil_function, probe_imag * pupil_function
        elif probe_type == 'fixed':
            probe_real, probe_imag = util.mag_phase_to_real_imag(*probe_initial)
        elif probe_type == 'gaussian':
            probe_real, probe_imag = util.gaussian_probe(obj_size[:2], kwargs['probe_mag_sigma'], kwargs['probe_phase_sigma'],
                                                         kwargs['probe_phase_max'])
        else:
            raise ValueError("Invalid wavefront type. Choose from 'plane', 'fixed', 'optimizable'.")

        coord_ls = None if rotation in ('bilinear', 'trilinear') else util.rotation_lookup_files([dim_y, dim_x, dim_x], n_theta, comm)
        solver = FullfieldSolver(dim_y, dim_x, dim_z, n_theta, minibatch_size, energy_ev, psize_cm * ds_level,
                                 free_prop_cm=free_prop_cm, probe_real=probe_real, probe_imag=probe_imag, variant=variant,
                                 comm=comm, device=comm.local_rank, coord_ls=coord_ls, propagator=propagator, kernel_size=kernel_size,
                                 rotation=rotation, theta=theta, adjoint64={'float32': None, 'float64': True, 'first-step': 'first'}[adjoint_precision],
                                 detector_kernel=kwargs.get('detector_kernel', 'TF'),   # 'IR' / 'auto': np_funcs.py:51-61
                                 loss_type=loss_type, poisson_multiplier=poisson_multiplier, slice_binning=slice_binning,
                                 detector_weights=weights, **geo.for_level(ds_level))
        if geo.refine and geo.refined is not None:
            solver.set_geometry(**geo.level_values(ds_level))
        solver.set_volume(obj_delta, obj_beta)
        solver.set_mask(mask)
        solver.set_measurements(np.abs(prj))
        if analytic_start and first_level:
            solver.analytic_volume(np.abs(prj), delta_beta_ratio, ctf_regularization, object_type)
            if write_support_mask is not None and rank == 0:
                coarse = solver.get_volume()[0]
                for axis in range(3):            # the level's voxels are every ds_level-th of the full resolution's: repeated back
                    coarse = np.repeat(coarse, ds_level, axis=axis)
                support_from = coarse[:prj_0.shape[-2], :prj_0.shape[-1], :full_z]      # written after the LAST level: every level of this run reads the mask that was there
        solver.tune_tail()                       # N ranks: slab count of the exchange + Adam pipeline, by measurement; step() uses it
        if probe_type == 'optimizable':          # the probe is a variable too (tensorflow_recon/fullfield.py:311-327,442-455)
            solver.enable_probe_optimization(probe_real, probe_imag, probe_learning_rate, pupil_function)

        print_flush('Optimizer started.', 0, rank)
        if rank == 0:
            lines = SUMMARY_PRESET_FF + (SUMMARY_GEOMETRY if trilinear else []) + (SUMMARY_ANALYTIC if analytic_start else [])
            if lines != SUMMARY_PRESET_FF:       # the geometry this level ran with and the analytic start, behind the preset's lines
                create_summary(output_folder, dict(locals(), **(geo.summary() if trilinear else {})), var_list=lines)
            else:
                create_summary(output_folder, locals(), preset='fullfield')

        this_n_epochs = n_epochs
        if ds_level == 1 and n_epoch_final_pass is not None and multiscale_level > 1:
            this_n_epochs = n_epoch_final_pass
        # the angles are shuffled ONCE per resolution level and every epoch walks the same minibatches
        # (cnn_propagator/fullfield.py:196-203 sits outside the epoch loop; pinned by golden vectors G10 / G13)
        ind_ls = minibatch_schedule(n_theta, size, minibatch_size, rng=np.random.RandomState(seed), shuffle=random_theta)
        i_epoch, last_loss, cont = 0, None, True
        while cont:
            solver.reset_moments()                                   # m, v = (None, None), fullfield.py:338
            use_mask = i_epoch < n_epochs_mask_release
            t0 = time.time()
            for i_batch, chunk in enumerate(ind_ls):
                t00 = time.time()
                this_ind_batch = chunk[rank * minibatch_size:(rank + 1) * minibatch_size]
                # loss_grad -> Allreduce -> /size -> Adam -> mask, clip (fullfield.py:345-362): one pipelined device step
                solver.step(i_batch, this_ind_batch, learning_rate, reg_d, reg_b, gamma, use_mask=use_mask,
                            n_batch_per_update=n_batch_per_update if accumulate else 1, last_of_epoch=i_batch == len(ind_ls) - 1)
                if save_intermediate and rank == 0:
                    d, _ = solver.get_volume()
                    tiffio.write_tiff(d, os.path.join(output_folder, 'intermediate', 'current'), dtype='float32', overwrite=True)
                    if geo.refine:
                        geo.record(solver.geometry(), ds_level, output_folder)
                if shrink_cycle is not None and i_epoch >= shrink_cycle:
                    solver.shrink_wrap()
                if debug:
                    solver.ctx.sync()
                    print_flush('Minibatch done in {} s (rank {})'.format(time.time() - t00, rank))
                    if i_batch % 10 == 0:
                        # cnn_propagator/fullfield.py:372-374: |exit waves| of this rank's minibatch through the updated object
                        temp_exit = solver.forward_angles(this_ind_batch)
                        tiffio.write_tiff(np.abs(temp_exit), os.path.join(output_folder, 'exits', '{}-{}'.format(i_epoch, i_batch)),
                                          dtype='float32', overwrite=True)
            this_loss = solver.loss_and_grad(this_ind_batch, want_loss=True)
            if size > 1:
                this_loss = float(comm.allreduce_sum_host(np.array([this_loss]))[0]) / size
            i_epoch += 1
            reg_loss = solver.regularizer(reg_d, reg_b, gamma)       # the reference's epoch line is calculate_loss: data + regulariser
            print_flush('Epoch {} (rank {}); loss = {} (data term {}); Delta-t = {} s; current time = {}.'.format(
                i_epoch, rank, this_loss + reg_loss, this_loss, time.time() - t0, time.time() - t_zero), 0, rank)
            if this_n_epochs == 'auto':
                if last_loss is not None and last_loss > 0 and (last_loss - this_loss) / last_loss < crit_conv_rate:
                    cont = False
                if i_epoch >= max_nepochs:
                    cont = False
                last_loss = this_loss
            elif i_epoch >= this_n_epochs:
                cont = False

        obj_delta, obj_beta = solver.get_volume()
        if geo.refine:                               # every rank holds the same values (the gradient was summed over the ranks)
            geo.keep(solver.geometry(), ds_level)
            if rank == 0:
                geo.record(solver.geometry(), ds_level, output_folder, summary=True)
        if rank == 0:
            tiffio.write_tiff(obj_delta, os.path.join(output_folder, 'delta_ds_{}'.format(ds_level)), dtype='float32', overwrite=True)
            tiffio.write_tiff(obj_beta, os.path.join(output_folder, 'beta_ds_{}'.format(ds_level)), dtype='float32', overwrite=True)
            if probe_type == 'optimizable':      # tensorflow_recon/fullfield.py:604-607 writes probe_mag / probe_phase
                pr_f, pi_f = solver.get_probe()
                tiffio.write_tiff(np.sqrt(pr_f ** 2 + pi_f ** 2), os.path.join(output_folder, 'probe_mag_ds_{}'.format(ds_level)), dtype='float32', overwrite=True)
                tiffio.write_tiff(np.arctan2(pi_f, pr_f), os.path.join(output_folder, 'probe_phase_ds_{}'.format(ds_level)), dtype='float32', overwrite=True)
        if fsc_reference is not None and ds_level == 1 and rank == 0:
            resolution.write_report(solver.shell_correlation(fsc_reference, psize_cm), output_folder, fsc_threshold, psize_cm)
        obj_delta, obj_beta = obj_delta.astype(float), obj_beta.astype(float)
        first_level = False
        del solver
        print_flush('Current iteration finished.', 0, rank)
    if support_from is not None:                 # rank 0 alone holds it; no level of this run reads fin_sup_mask after this point
        analytic.support_mask(support_from, write_support_mask, save_path=save_path)
    comm.Barrier()                               # (and no rank returns, to start a next run that reads the mask, before it is whole)
    return obj_delta, obj_beta
