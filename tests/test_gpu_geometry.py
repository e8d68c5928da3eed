"""The geometry gradient and refine_geometry through FullfieldSolver and PtychoSolver (rotation='trilinear').

geometry_gradient() after loss_and_grad against the float64 reference of tests/geometry_reference.py (the restatement of
dL/d(M | t) on the model's float64 rotated-frame gradient, then util.rigid_geometry_gradient): every entry within
GEOMETRY_GRADIENT_BOUND / PTYCHO_GEOMETRY_GRADIENT_BOUND of the sum of the absolute values of its terms (geometry_term_sums), the
bounds tests/test_geometry_reference.py derives on the CPU.  refine_geometry=() leaves a step's bits alone.  Recovery: data
simulated with the axis 1.5 pixels (0.02 rad) off, the true volume, volume learning rate 0 — the refined value must come at least
10 times closer to the truth within the step budget (100 steps; a step of the 32^3 case takes about a millisecond).  Reached on
one MI355X (MEASUREMENTS.md, "Geometry gradient"): center 15.5 -> 16.9908 of 17.0 at geometry_learning_rate 0.05; axis_tilt
0.3 -> 0.319894 of 0.32 at the lowered rate 0.01 (0.000625 rad per step: at 0.05 Adam's step alone, 0.003 rad, exceeds the 0.002 rad
the ratio allows).  The gradient tests: every geometry entry within 2.4e-4 of its bound, dL/d(M | t) within 3.1e-9 of its term sums."""
import numpy as np
import pytest

import geometry_reference as gr
import rigid_reference as rr

pytestmark = pytest.mark.gpu

N, N_THETA, MB = rr.N, rr.N_THETA, rr.MB
IDX = np.array(rr.IDX)


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


def held(got, ref, sums, bound, names, what):
    worst = 0.0
    for name in names:
        ratio = np.abs(np.asarray(got[name]) - np.asarray(ref[name])) / (bound * np.asarray(sums[name]))
        print(what, name, 'device', np.asarray(got[name]), 'reference', np.asarray(ref[name]), '|difference| / bound', ratio)
        worst = max(worst, float(np.max(ratio)))
    assert worst <= 1.0, what


def test_fullfield_geometry_gradient(built):
    from beyond_dof_amd.solver import FullfieldSolver
    p, ref = rr.solver_problem(gr.FP), gr.solver_geometry_problem()
    s = FullfieldSolver(N, N, N, N_THETA, MB, rr.E_EV, rr.PSIZE_CM, free_prop_cm=gr.FP, rotation='trilinear', theta=rr.solver_theta(),
                        axis_tilt=rr.TILT, axis_roll=rr.ROLL, center=rr.CENTER)
    s.set_volume(p['od'], p['ob'])
    prj = np.zeros((N_THETA, N, N))
    prj[IDX] = p['meas']
    s.set_measurements(prj)
    s.loss_and_grad(IDX)
    got = s.geometry_gradient()
    again = s.geometry_gradient()
    assert all(np.array_equal(got[k], again[k]) for k in got)
    sums = gr.geometry_term_sums(ref['T'], IDX, rr.solver_theta(), (N, N, N), rr.TILT, rr.ROLL, rr.CENTER)
    held(got, ref['geometry'], sums, gr.GEOMETRY_GRADIENT_BOUND, ('center', 'axis_tilt', 'axis_roll', 'theta', 'shifts'), 'full field')
    # the rows themselves, relative to their own term sums
    d = s.rot.param_gradient(s.x[s.cur])
    worst = float(np.max(np.abs(d - ref['d']) / ref['T']))
    print('dL/d(M | t): largest |device - reference| / sum |terms|', worst, 'bound', gr.GEOMETRY_GRADIENT_BOUND)
    assert worst <= gr.GEOMETRY_GRADIENT_BOUND
    geo = s.geometry()
    assert geo['center'] == rr.CENTER and geo['axis_tilt'] == rr.TILT and np.array_equal(geo['theta'], rr.solver_theta()) and not np.any(geo['shifts'])


def test_ptycho_geometry_gradient(built):
    from beyond_dof_amd.solver import PtychoSolver
    psz = 32
    p, ref = rr.ptycho_problem(psz), gr.ptycho_geometry_problem(psz)
    s = PtychoSolver(rr.PTY_SHAPE, (psz, psz), rr.PTY_POS, rr.PTY_N_THETA, len(rr.PTY_POS), rr.E_EV, rr.PSIZE_CM, p['pr'], p['pi'],
                     rotation='trilinear', theta=rr.ptycho_theta(), axis_tilt=rr.PTY_TILT)
    s.set_volume(p['od'], p['ob'])
    s.loss_and_grad(rr.PTY_THETA, np.arange(len(rr.PTY_POS)), p['meas'])
    got = s.geometry_gradient()
    assert got['theta'].shape == (1,) and got['shifts'].shape == (1, 2)
    sums = gr.geometry_term_sums(ref['T'], np.array([rr.PTY_THETA]), rr.ptycho_theta(), rr.PTY_SHAPE, rr.PTY_TILT, 0., None)
    held(got, ref['geometry'], sums, gr.PTYCHO_GEOMETRY_GRADIENT_BOUND, ('center', 'axis_tilt', 'axis_roll', 'theta', 'shifts'), 'ptychography')


def test_no_refinement_leaves_the_bits_of_a_step(built):
    """refine_geometry=() against a solver built without the keyword: two steps, the same volume bit for bit; and a solver that
    refines refuses gradient accumulation"""
    from beyond_dof_amd.solver import FullfieldSolver
    p = rr.solver_problem(gr.FP)
    prj = np.zeros((N_THETA, N, N))
    prj[IDX] = p['meas']
    geo = dict(theta=rr.solver_theta(), axis_tilt=rr.TILT, axis_roll=rr.ROLL, center=rr.CENTER)
    vols = []
    for kw in ({}, dict(refine_geometry=()), dict(refine_geometry=('center', 'theta'))):
        s = FullfieldSolver(N, N, N, N_THETA, MB, rr.E_EV, rr.PSIZE_CM, free_prop_cm=gr.FP, rotation='trilinear', **dict(geo, **kw))
        s.set_volume(p['od'] * 0.9, p['ob'] * 0.9)
        s.set_measurements(prj)
        s.reset_moments()
        if kw.get('refine_geometry'):
            with pytest.raises(ValueError, match='n_batch_per_update'):
                s.step(0, IDX, 1e-8, n_batch_per_update=2)
        prm = s.rot.prm.copy()
        for i in range(2):
            s.step(i, IDX, 1e-8)
        moved = not np.array_equal(s.rot.prm, prm)
        assert moved == bool(kw.get('refine_geometry'))
        if moved:
            assert np.array_equal(np.nonzero(s.geometry()['theta'] != rr.solver_theta())[0], IDX)       # only the step's angles
        vols.append(s.get_volume())
    assert np.array_equal(vols[0][0], vols[1][0]) and np.array_equal(vols[0][1], vols[1][1])
    assert not np.array_equal(vols[0][0], vols[2][0])


# ---- recovery ----------------------------------------------------------------------------------------------------------------------------
R, R_THETA, STEPS = 32, 8, 100


def _phantom():
    """three gaussian blobs of unequal weight away from the axis and from each other, zero near the faces"""
    y, x, z = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing='ij')
    od = np.zeros((R, R, R))
    for (cy, cx, cz), w, a in (((11, 20, 14), 3.0, 2e-4), ((21, 10, 19), 2.5, 1.5e-4), ((16, 17, 9), 2.0, 1e-4)):
        od += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2 + (z - cz) ** 2) / (2 * w ** 2))
    od[od < 1e-6] = 0.
    return od, 0.1 * od


@pytest.mark.parametrize('name,nominal,off,rate', [('center', (R - 1) / 2., 1.5, 0.05), ('axis_tilt', 0.3, 0.02, 0.01)])
def test_refinement_recovers_the_geometry(built, name, nominal, off, rate):
    from beyond_dof_amd.solver import FullfieldSolver
    od, ob = _phantom()
    theta = -np.linspace(0, np.pi, R_THETA, endpoint=False)
    idx = np.arange(R_THETA)
    base = dict(center=(R - 1) / 2., axis_tilt=0.3)

    def solver(value, **kw):
        s = FullfieldSolver(R, R, R, R_THETA, R_THETA, rr.E_EV, rr.PSIZE_CM, free_prop_cm=1e-4, rotation='trilinear', theta=theta,
                            **dict(base, **{name: value}), **kw)
        s.set_volume(od, ob)
        return s
    data = np.abs(solver(nominal + off).forward_angles(idx))
    s = solver(nominal, refine_geometry=(name,), geometry_learning_rate=rate)
    s.set_measurements(data)
    s.reset_moments()
    first = s.step(0, idx, 0.0, want_loss=True)
    for i in range(1, STEPS):
        s.step(i, idx, 0.0)
    last = s.loss_and_grad(idx)
    reached = float(s.geometry()[name])
    print(name, 'from', nominal, 'truth', nominal + off, 'reached', reached, 'after', STEPS, 'steps; loss', first, '->', last)
    d, b = s.get_volume()
    assert np.array_equal(d, od.astype(np.float32)) and np.array_equal(b, ob.astype(np.float32))           # the volume stood still
    assert abs(reached - (nominal + off)) <= off / 10.


def test_reconstruct_fullfield_refines_records_and_carries_the_centre(built, tmp_path, monkeypatch):
    """the entry point over two multiscale levels, data with the axis 1.5 pixels off: the fine level starts from the coarse level's
    centre in its own units, geometry.npy and summary.txt hold the refined values in full-resolution units, the centre has moved towards the truth"""
    import os
    from beyond_dof_amd import fullfield, h5io
    from beyond_dof_amd.solver import FullfieldSolver
    monkeypatch.chdir(tmp_path)
    od, ob = _phantom()
    theta = -np.linspace(0, np.pi, R_THETA, dtype='float32')
    sim = FullfieldSolver(R, R, R, R_THETA, R_THETA, rr.E_EV, rr.PSIZE_CM, free_prop_cm=1e-4, rotation='trilinear', theta=theta, center=17.0)
    sim.set_volume(od, ob)
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', np.abs(sim.forward_angles(np.arange(R_THETA))).astype(np.complex64))
    starts = []
    real = fullfield.FullfieldSolver.set_geometry
    monkeypatch.setattr(fullfield.FullfieldSolver, 'set_geometry', lambda self, **kw: (starts.append(float(kw['center'])), real(self, **kw))[1])
    fullfield.reconstruct_fullfield('data.h5', theta_st=0, theta_end=np.pi, n_epochs=10, learning_rate=0., minibatch_size=R_THETA, energy_ev=rr.E_EV,
                                    psize_cm=rr.PSIZE_CM, free_prop_cm=1e-4, save_path='case', output_folder='out',
                                    initial_guess=[od[::2, ::2, ::2], ob[::2, ::2, ::2]], shrink_cycle=None, seed=1, alpha_d=0., alpha_b=0., gamma=0.,
                                    rotation='trilinear', center=15.5, multiscale_level=2, refine_geometry=('center',), geometry_learning_rate=0.05)
    rec = np.load(os.path.join('case', 'out', 'geometry.npy'), allow_pickle=True).item()
    assert sorted(rec) == ['axis_roll', 'axis_tilt', 'center', 'shifts', 'theta'] and rec['shifts'].shape == (R_THETA, 2)
    coarse_end = starts[0]                       # (level_values of the finest level: full-resolution units)
    print('centre: start 15.5, after the coarse level', coarse_end, 'at the end', float(rec['center']), '(data simulated with 17.0)')
    assert len(starts) == 1 and coarse_end != 15.5
    assert 15.5 < float(rec['center']) <= 17.5
    text = open(os.path.join('case', 'out', 'summary.txt')).read()
    assert 'refined_center' in text and 'refined_shifts' in text
    with pytest.raises(ValueError, match="rotation='trilinear' only"):
        fullfield.reconstruct_fullfield('data.h5', save_path='case', rotation='bilinear', refine_geometry=('center',))
    with pytest.raises(ValueError, match='accumulate_gradients'):
        fullfield.reconstruct_fullfield('data.h5', save_path='case', rotation='trilinear', refine_geometry=('center',), accumulate_gradients=True)
