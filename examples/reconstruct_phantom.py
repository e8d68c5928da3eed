"""A complete small reconstruction, the way the reference's driver scripts run one (cnn_propagator/reconstruct_fullfield.py):
simulate a full-field dataset of a phantom with the product's forward model, write it as exchange/data, reconstruct with
reconstruct_fullfield and compare with the phantom.  The detector distance decides how much of the phase the intensities
carry: at 10 um (free_prop_cm=1e-3) 100 epochs recover delta to a correlation of 0.988 with the phantom (relative L2 error
0.16) in 2.6 s on one MI355X; at 1 um the low spatial frequencies are barely encoded and the same run stalls at 0.82; in
the far field with a plane probe (one bright bin) it does not converge — properties of the measurement, the same for the
reference.

    python examples/reconstruct_phantom.py [n=128] [n_theta=60] [n_epochs=100] [learning_rate=2e-8] [free_prop_cm=1e-3] [minibatch=10]
                                           [propagator=fft] [--loss lsq|poisson] [--poisson-multiplier 2e6] [--slice-binning 1]
                                           [--refine-geometry center,axis_tilt] [--fsc] [--analytic-start]

--loss poisson minimises the photon-counting likelihood (loss_type='poisson'); its data term is ~ 2 * multiplier times the
least-squares one, and the L1 weights are scaled with it here.
free_prop_cm=5e-4,1e-3,2e-3 (distances separated by commas) simulates and fits several detector planes per angle: the data file
is then (n_theta, D, Y, X) and run(..., fp=(5e-4, 1e-3, 2e-3)) is the same from Python.
--slice-binning b reconstructs with one propagation step per b voxel slices (slice_binning=b); the data are always simulated
with one step per voxel slice.
--refine-geometry names: the data are simulated with rotation='trilinear' about an axis that is OFFSET (OFFSET below: the centre
1.5 pixels, the tilt 0.01 rad off the nominal geometry) and reconstructed from the nominal one with refine_geometry=names; the
refined values (out/geometry.npy) are printed beside the truth.
--analytic-start: the run starts from initial_guess='ctf-fbp' (CTF retrieval and filtered back-projection on the device,
FullfieldSolver.analytic_volume) instead of zeros; the correlation of that start itself with the phantom is printed first.  Combines
with --refine-geometry: the start is then formed with the nominal (wrong) geometry the refinement begins from.
--fsc: the resolution of the run by Fourier shell correlation (beyond_dof_amd/resolution.py).  The data are simulated and fitted
with rotation='bilinear' (the true angles, so that a subset of them is a data set of its own).  Printed: the curve of the
reconstruction against the phantom (fsc_reference=) with the half-bit resolution of delta and beta; then the even and the odd
angles are reconstructed separately, each from its own data file with theta_st / theta_end at its first and last angle, and the
half-bit resolution of the two halves against each other — the figure a user with measured data, who has no phantom, can get.
"""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beyond_dof_amd import h5io, resolution                       # noqa: E402
from beyond_dof_amd.fullfield import reconstruct_fullfield       # noqa: E402
from beyond_dof_amd.solver import FullfieldSolver                # noqa: E402


def phantom(n, rng):
    """A few soft blobs inside the central cylinder: delta up to ~1.5e-6, beta = delta / 10."""
    z, y, x = np.mgrid[:n, :n, :n].astype(np.float32)
    d = np.zeros((n, n, n), dtype=np.float32)
    for _ in range(10):
        c = rng.uniform(n * 0.3, n * 0.7, size=3)
        r = rng.uniform(n * 0.04, n * 0.12)
        d += 1e-6 * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * r ** 2))
    return d


OFFSET = dict(center=1.5, axis_tilt=0.01)


def run(n=128, n_theta=60, n_epochs=100, lr=2e-8, fp=1e-3, quiet=False, mb=10, propagator='fft', loss='lsq', multiplier=2e6, slice_binning=1,
        refine=(), analytic_start=False):
    """Simulate, write exchange/data, reconstruct, compare with the phantom: returns the figures main() prints
    (tests/test_gpu_convergence.py asserts them)."""
    import contextlib
    import io
    rng = np.random.default_rng(0)
    d = phantom(n, rng)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        nominal = dict(center=(n - 1) / 2., axis_tilt=0.)
        truth = {k: v + OFFSET[k] for k, v in nominal.items()}
        theta = -np.linspace(0, 2 * np.pi, n_theta, dtype='float32')          # the entry point's angles
        sim = dict(rotation='trilinear', theta=theta, **truth) if refine else {}
        fit = dict(rotation='trilinear', refine_geometry=tuple(refine), **nominal) if refine else {}
        s = FullfieldSolver(n, n, n, n_theta, mb, 5000., 1e-7, free_prop_cm=fp, propagator=propagator, **sim)
        s.set_volume(d, 0.1 * d)
        prj = s.forward_angles(np.arange(n_theta))
        del s
        os.makedirs('case')
        h5io.write_dataset('case/data.h5', 'exchange/data', prj.astype(np.complex64))
        reg = 2 * multiplier if loss == 'poisson' else 1.0      # the regulariser keeps its weight beside the data term
        start_corr = None
        if analytic_start:                                     # the start by itself, as the entry point will form it
            a = FullfieldSolver(n, n, n, n_theta, mb, 5000., 1e-7, free_prop_cm=fp, propagator=propagator, slice_binning=slice_binning,
                                **(dict(rotation='trilinear', theta=theta, **nominal) if refine else {}))
            a.analytic_volume(np.abs(prj))
            start_corr = float(np.corrcoef(a.get_volume()[0].ravel(), d.ravel())[0, 1])
            del a
        t0 = time.time()
        with (contextlib.redirect_stdout(io.StringIO()) if quiet else contextlib.nullcontext()):
            rd, rb = reconstruct_fullfield('data.h5', theta_st=0, theta_end=2 * np.pi, n_epochs=n_epochs, learning_rate=lr,
                                           minibatch_size=mb, energy_ev=5000, psize_cm=1e-7, free_prop_cm=fp, save_path='case',
                                           output_folder='out', shrink_cycle=None, seed=3, alpha_d=1e-9 * reg, alpha_b=1e-10 * reg, gamma=0,
                                           initial_guess='ctf-fbp' if analytic_start else [np.zeros_like(d), np.zeros_like(d)],
                                           propagator=propagator, loss_type=loss, poisson_multiplier=multiplier, slice_binning=slice_binning, **fit)
        dt = time.time() - t0
        refined = np.load(os.path.join('case', 'out', 'geometry.npy'), allow_pickle=True).item() if refine else {}
        os.chdir(cwd)
    inner = (slice(n // 4, -n // 4),) * 3
    return {'n': n, 'n_theta': n_theta, 'n_epochs': n_epochs, 'seconds': dt, 'start_corr': start_corr,
            'geometry': {k: (nominal[k], float(refined[k]), truth[k]) for k in refine if k in nominal},
            'delta_corr': float(np.corrcoef(rd.ravel(), d.ravel())[0, 1]),
            'delta_corr_inner': float(np.corrcoef(rd[inner].ravel(), d[inner].ravel())[0, 1]),
            'delta_rel_l2': float(np.linalg.norm(rd - d) / np.linalg.norm(d)), 'delta_peak': float(rd.max()), 'phantom_peak': float(d.max()),
            'beta_corr': float(np.corrcoef(rb.ravel(), 0.1 * d.ravel())[0, 1])}


def _resolution_text(res):
    return ', '.join('{} {}'.format(k, 'no crossing' if r is None else '{:.3g} nm half period (shell {:.2f})'.format(1e7 * r.half_period, r.shell))
                     for k, r in sorted(res.items(), reverse=True))


def run_fsc(n=128, n_theta=60, n_epochs=100, lr=2e-8, fp=1e-3, mb=10, propagator='fft', quiet=True, psize_cm=1e-7):
    """The run of run() with rotation='bilinear', measured by Fourier shell correlation: against the phantom, and the even against
    the odd angles.  Returns {'phantom': record, 'halves': record} (resolution.ShellRecord)."""
    import contextlib
    import io
    rng = np.random.default_rng(0)
    d = phantom(n, rng)
    angles = np.linspace(0, 2 * np.pi, n_theta)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            s = FullfieldSolver(n, n, n, n_theta, mb, 5000., psize_cm, free_prop_cm=fp, propagator=propagator, rotation='bilinear',
                                theta=-angles.astype('float32'))
            s.set_volume(d, 0.1 * d)
            prj = s.forward_angles(np.arange(n_theta)).astype(np.complex64)
            del s
            os.makedirs('case')
            sets = {'all': slice(None), 'even': slice(0, None, 2), 'odd': slice(1, None, 2)}
            out = {}
            for name, part in sets.items():
                h5io.write_dataset('case/{}.h5'.format(name), 'exchange/data', prj[part])
                with (contextlib.redirect_stdout(io.StringIO()) if quiet else contextlib.nullcontext()):
                    out[name] = reconstruct_fullfield(
                        name + '.h5', theta_st=angles[part][0], theta_end=angles[part][-1], n_epochs=n_epochs, learning_rate=lr,
                        minibatch_size=min(mb, len(angles[part])), energy_ev=5000, psize_cm=psize_cm, free_prop_cm=fp, save_path='case',
                        output_folder='out_' + name, shrink_cycle=None, seed=3, alpha_d=1e-9, alpha_b=1e-10, gamma=0,
                        initial_guess=[np.zeros_like(d), np.zeros_like(d)], propagator=propagator, rotation='bilinear',
                        fsc_reference=(d, 0.1 * d) if name == 'all' else None)
            saved = np.load(os.path.join('case', 'out_all', 'fsc.npy'), allow_pickle=True).item()
        finally:
            os.chdir(cwd)
    return {'phantom': resolution.ShellRecord(**saved), 'halves': resolution.fourier_shell_correlation(out['even'], out['odd'], psize_cm)}


def _option(name, default):
    """--name value, taken out of sys.argv (the positional arguments keep their places)."""
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    value = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    return value


def main():
    loss = _option('--loss', 'lsq')
    multiplier = float(_option('--poisson-multiplier', 2e6))
    slice_binning = int(_option('--slice-binning', 1))
    refine = tuple(k for k in _option('--refine-geometry', '').split(',') if k)
    fsc = '--fsc' in sys.argv
    if fsc:
        sys.argv.remove('--fsc')
    analytic_start = '--analytic-start' in sys.argv
    if analytic_start:
        sys.argv.remove('--analytic-start')
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    n_theta = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    n_epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    lr = float(sys.argv[4]) if len(sys.argv) > 4 else 2e-8
    fp = sys.argv[5] if len(sys.argv) > 5 else '1e-3'
    fp = 'inf' if fp == 'inf' else tuple(float(z) for z in fp.split(',')) if ',' in fp else float(fp)
    mb = int(sys.argv[6]) if len(sys.argv) > 6 else 10
    propagator = sys.argv[7] if len(sys.argv) > 7 else 'fft'
    if fsc:
        r = run_fsc(n, n_theta, n_epochs, lr, fp, mb=mb, propagator=propagator)
        rec = r['phantom']
        print('Fourier shell correlation with the phantom, {}^3, {} angles, {} epochs:'.format(n, n_theta, n_epochs))
        print('  shell  cycles/voxel  n_points  fsc_delta  fsc_beta  half-bit')
        for row in zip(rec.shell, rec.frequency, rec.n_points, rec.fsc_delta, rec.fsc_beta, resolution.threshold_curve('half-bit', rec.n_points)):
            print('  {:5d}  {:12.4f}  {:8d}  {:9.4f}  {:8.4f}  {:8.4f}'.format(*row))
        print('resolution against the phantom (half-bit): ' + _resolution_text(resolution.resolution(rec, 'half-bit')))
        print('resolution of the even against the odd angles (half-bit): ' + _resolution_text(resolution.resolution(r['halves'], 'half-bit')))
        return
    r = run(n, n_theta, n_epochs, lr, fp, mb=mb, propagator=propagator, loss=loss, multiplier=multiplier, slice_binning=slice_binning,
            refine=refine, analytic_start=analytic_start)
    if analytic_start:
        print('analytic start (CTF retrieval + filtered back-projection): delta correlation with the phantom {:.4f}'.format(r['start_corr']))
    for k, (start, reached, truth) in r['geometry'].items():
        print('{}: nominal {:.4f}, refined {:.4f}, simulated with {:.4f}'.format(k, start, reached, truth))
    if slice_binning > 1:
        print('slice_binning {}: {} propagation steps per angle'.format(slice_binning, n // slice_binning))
    print('reconstruct_fullfield (propagator {}, loss {}) {}^3, {} angles, {} epochs in minibatches of {}: {:.1f} s ({:.1f} ms per Adam step, entry point to files)'.format(
        propagator, loss, n, n_theta, n_epochs, mb, r['seconds'], 1e3 * r['seconds'] / (n_epochs * max(1, n_theta // mb))))
    print('delta: correlation with the phantom {:.4f} (central half {:.4f}); relative L2 error {:.3f}; peak {:.3e} vs {:.3e}'.format(
        r['delta_corr'], r['delta_corr_inner'], r['delta_rel_l2'], r['delta_peak'], r['phantom_peak']))
    print('beta : correlation {:.4f}'.format(r['beta_corr']))


if __name__ == '__main__':
    main()
