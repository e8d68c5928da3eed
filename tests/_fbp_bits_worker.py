"""Worker of tests/test_gpu_fbp.py: reconstruct_fullfield(initial_guess=[zeros, zeros]) — the path the analytic start must leave
alone — with the package under ROOT, for rotation='nearest' and 'trilinear'; delta, beta and summary.txt of each go to OUT.npz.
usage: _fbp_bits_worker.py ROOT WORKDIR OUT.npz"""
import contextlib
import io
import os
import sys

import numpy as np


def main(root, work, out):
    out = os.path.abspath(out)
    sys.path.insert(0, root)
    import beyond_dof_amd
    assert os.path.abspath(os.path.dirname(beyond_dof_amd.__file__)).startswith(os.path.abspath(root))
    from beyond_dof_amd import h5io
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from beyond_dof_amd.solver import FullfieldSolver
    n, nt, mb = 32, 24, 8
    os.makedirs(work, exist_ok=True)
    os.chdir(work)
    rng = np.random.default_rng(0)
    z, y, x = np.mgrid[:n, :n, :n].astype(np.float64)
    d = np.zeros((n, n, n))
    for _ in range(10):
        c = rng.uniform(n * 0.3, n * 0.7, size=3)
        r = rng.uniform(n * 0.04, n * 0.12)
        d += 1e-6 * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * r ** 2))
    res = {}
    for rotation in ('nearest', 'trilinear'):
        kw = {} if rotation == 'nearest' else dict(rotation='trilinear')
        s = FullfieldSolver(n, n, n, nt, mb, 5000., 1e-7, free_prop_cm=1e-3, theta=-np.linspace(0, 2 * np.pi, nt, dtype='float32'), **kw)
        s.set_volume(d, 0.1 * d)
        prj = s.forward_angles(np.arange(nt))
        del s
        os.makedirs('case_' + rotation, exist_ok=True)
        h5io.write_dataset('case_{}/data.h5'.format(rotation), 'exchange/data', prj.astype(np.complex64))
        with contextlib.redirect_stdout(io.StringIO()):
            rd, rb = reconstruct_fullfield('data.h5', theta_st=0, theta_end=2 * np.pi, n_epochs=2, learning_rate=2e-8, minibatch_size=mb,
                                           energy_ev=5000, psize_cm=1e-7, free_prop_cm=1e-3, save_path='case_' + rotation, output_folder='out',
                                           shrink_cycle=None, seed=3, alpha_d=1e-9, alpha_b=1e-10, gamma=0,
                                           initial_guess=[np.zeros_like(d), np.zeros_like(d)], **kw)
        assert np.array_equal(rd, rd.astype(np.float32)) and np.array_equal(rb, rb.astype(np.float32))      # float32 values: stored as such
        res['d_' + rotation], res['b_' + rotation] = rd.astype(np.float32), rb.astype(np.float32)
        res['summary_' + rotation] = np.array(open('case_{}/out/summary.txt'.format(rotation)).read())
    np.savez_compressed(out, **res)


if __name__ == '__main__':
    main(*sys.argv[1:4])
