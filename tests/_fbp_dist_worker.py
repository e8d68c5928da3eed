"""Worker of tests/test_gpu_fbp.py: one rank of two that share ONE GPU (gloo) forms the analytic starting volume.  Every rank
computes the whole volume from all angles; nothing is communicated."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def problem():
    """amplitudes that need no device to make: a weak random contrast about 1, 16^3, 6 angles in minibatches of 4"""
    rng = np.random.default_rng(5)
    n, n_theta, mb = 16, 6, 4
    return n, n_theta, mb, 1 + 0.01 * rng.normal(size=(n_theta, n, n))


def run(comm):
    from beyond_dof_amd.solver import FullfieldSolver
    n, n_theta, mb, meas = problem()
    s = FullfieldSolver(n, n, n, n_theta, mb, 5000., 1e-7, free_prop_cm=1e-3, rotation='trilinear', theta=-np.linspace(0, np.pi, n_theta),
                        axis_tilt=0.1, comm=comm)
    s.analytic_volume(meas)
    return s.get_volume()


def main(out_dir):
    from beyond_dof_amd.comm import get_comm
    comm = get_comm()                      # BDOF_COMM_BACKEND=gloo in the environment
    assert comm.size == 2
    d, b = run(comm)
    np.savez(os.path.join(out_dir, 'fbp_rank{}.npz'.format(comm.rank)), d=d, b=b)
    comm.Barrier()
    comm.close()


if __name__ == '__main__':
    main(sys.argv[1])
