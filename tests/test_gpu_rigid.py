"""rotation='trilinear' through FullfieldSolver, PtychoSolver and the two entry points: a tilted, rolled, off-centre axis (and the
same geometry handed over as rotation_matrices) against the float64 restatement of tests/rigid_reference.py composed with the
oracle.  The gradient bounds are rigid_reference.SOLVER_GRADIENT_BOUND and PTYCHO_GRADIENT_BOUND, which
tests/test_rigid_reference.py derives on the CPU."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import bdof_oracle as orc

import rigid_reference as rr

pytestmark = pytest.mark.gpu

N, N_THETA, MB = rr.N, rr.N_THETA, rr.MB
IDX = np.array(rr.IDX)


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _geometry(how):
    if how == 'keywords':
        return dict(theta=rr.solver_theta(), axis_tilt=rr.TILT, axis_roll=rr.ROLL, center=rr.CENTER)
    return dict(rotation_matrices=rr.solver_geometry().reshape(N_THETA, 3, 4))


@pytest.mark.parametrize('fp,how', [(1e-4, 'keywords'), (None, 'keywords'), (1e-4, 'matrices')])
def test_trilinear_rotation_forward_gradient_and_adam(built, fp, how):
    from beyond_dof_amd import rotation
    from beyond_dof_amd.solver import FullfieldSolver
    p = rr.solver_problem(fp)
    geo = _geometry(how)
    s = FullfieldSolver(N, N, N, N_THETA, MB, rr.E_EV, rr.PSIZE_CM, free_prop_cm=fp, rotation='trilinear', **geo)
    assert type(s.rot) is rotation.MaterialisedRotation and s.rot.kind is rotation.KINDS['trilinear'] and s.rot.kind is not rotation.KINDS['bilinear']
    s.set_volume(p['od'], p['ob'])
    w = s.forward_angles(IDX)
    e_int, e_wave = rel(np.abs(w) ** 2, np.abs(p['wave']) ** 2), rel(w, p['wave'])
    print('intensity', e_int, 'wave', e_wave)
    assert e_int <= 1e-5 and e_wave <= 1e-5
    prj = np.zeros((N_THETA, N, N))
    prj[IDX] = p['meas']
    s.set_measurements(prj)
    loss = s.loss_and_grad(IDX)
    gd, gb = s.gradient_to_host()
    e_loss, e_gd, e_gb = abs(loss - p['loss']) / abs(p['loss']), rel(gd, p['gd']), rel(gb, p['gb'])
    print('loss', e_loss, 'g_delta', e_gd, 'g_beta', e_gb, 'bound', rr.SOLVER_GRADIENT_BOUND)
    assert e_loss <= 1e-5
    assert e_gd <= rr.SOLVER_GRADIENT_BOUND and e_gb <= rr.SOLVER_GRADIENT_BOUND
    # two Adam steps on 3 % data: whole volume and slab-wise sharded give the same volume, bit for bit; the loss goes down
    rng = np.random.default_rng(11)
    prj[IDX] = (np.abs(p['wave']) * (1 + 0.03 * rng.normal(size=p['wave'].shape))).astype(np.float32)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_fullfield import _LoopbackComm
    vols = []
    for comm, kw in ((None, {}), (_LoopbackComm(), dict(n_slabs=4, sharded=True))):
        s2 = FullfieldSolver(N, N, N, N_THETA, MB, rr.E_EV, rr.PSIZE_CM, free_prop_cm=fp, rotation='trilinear', comm=comm, **geo)
        s2.set_volume(p['od'] * 0.9, p['ob'] * 0.9)
        s2.set_measurements(prj)
        s2.reset_moments()
        l0 = s2.step(0, IDX, 1e-8, alpha_d=1.5e-8, alpha_b=1.5e-9, gamma=1e-11, want_loss=True, **kw)
        s2.step(1, IDX, 1e-8, alpha_d=1.5e-8, alpha_b=1.5e-9, gamma=1e-11, **kw)
        l2 = s2.loss_and_grad(IDX)
        assert l2 < l0
        vols.append(s2.get_volume())
    assert np.array_equal(vols[0][0], vols[1][0]) and np.array_equal(vols[0][1], vols[1][1])


def test_trilinear_binding_for_the_real_space_propagator(built):
    """bdof_set_object_rigid(conv=1) writes the factors for the real-space propagator's k: the same waves as rotating first
    (bdof_rotate_rigid) and binding the rows (bdof_set_object), as the bilinear pair is held to"""
    from beyond_dof_amd._lib import DeviceBuffer
    from beyond_dof_amd.solver import FullfieldSolver
    p = rr.solver_problem(1e-4)
    s = FullfieldSolver(N, N, N, N_THETA, MB, rr.E_EV, rr.PSIZE_CM, free_prop_cm=1e-4, rotation='trilinear', propagator='conv',
                        **_geometry('keywords'))
    s.set_volume(p['od'], p['ob'])
    w = s.forward_angles(IDX)                                             # fused binding, conv sweep
    lib, h = s.ctx.lib, s.ctx.handle
    rows = DeviceBuffer(s.ctx, MB * N * N * N * 8, np.float32, (MB, N, N, N, 2))
    prm = DeviceBuffer.from_host(s.ctx, np.ascontiguousarray(s.rot.prm[IDX]))
    s.ctx.check(lib.bdof_rotate_rigid(h, s.x[s.cur].ptr, N, N, N, prm.ptr, MB, rows.ptr))
    s.eng.set_volume(rows, MB * N * N, N, None, 0, 0)
    assert np.any(np.abs(w - 1) > 1e-4) and np.array_equal(s.eng.forward(MB, conv=True), w)


# ---- the entry point --------------------------------------------------------------------------------------------------------------------
ENTRY_THETA = 6


@functools.lru_cache(maxsize=None)
def _entry_data(center):
    """(truth delta, beta, complex64 projections) of 6 angles under axis_tilt = 0.5 by the float64 composition"""
    from beyond_dof_amd import util
    rng = np.random.default_rng(0)
    od = np.zeros((N, N, N))
    od[:, 8:-8, 8:-8] = rng.uniform(0, 2e-6, size=(N, N - 16, N - 16))
    ob = 0.1 * od
    theta = -np.linspace(0, 2 * np.pi, ENTRY_THETA, dtype='float32')
    prm = util.rigid_geometry(theta, (N, N, N), 0.5, 0., center)
    obj = np.stack([od, ob], axis=3)
    rot = np.stack([rr.rotate_volume(obj, q) for q in prm])
    one, zero = np.ones((N, N)), np.zeros((N, N))
    prj, _ = orc.multislice_propagate_batch_numpy(rot[..., 0], rot[..., 1], one, zero, 5000., 1e-7, 1e-4, rot[..., 0].shape, return_probe_array=False)
    return od, ob, prj.astype(np.complex64)


def _summary(path):
    return dict(line.split(None, 1) if len(line.split(None, 1)) == 2 else (line.strip(), '') for line in open(path).read().splitlines())


def test_reconstruct_fullfield_trilinear(built, tmp_path, monkeypatch):
    """one epoch from 0.9 x truth moves towards the truth, writes no lookup-table folder and records the geometry"""
    from beyond_dof_amd import h5io
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    monkeypatch.chdir(tmp_path)
    od, ob, prj = _entry_data(None)
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', prj)
    d, b = reconstruct_fullfield('data.h5', theta_st=0, theta_end=2 * np.pi, n_epochs=1, learning_rate=1e-8, minibatch_size=3, energy_ev=5000,
                                 psize_cm=1e-7, free_prop_cm=1e-4, save_path='case', output_folder='out', initial_guess=[od * 0.9, ob * 0.9],
                                 shrink_cycle=None, seed=1, alpha_d=0., alpha_b=0., gamma=0., rotation='trilinear', axis_tilt=0.5)
    assert os.path.exists(os.path.join('case', 'out', 'delta_ds_1.tiff')) and d.shape == (N, N, N)
    assert not [f for f in os.listdir('.') if f.startswith('arrsize_')]
    assert np.linalg.norm(d - od) < np.linalg.norm(0.9 * od - od)
    rec = _summary(os.path.join('case', 'out', 'summary.txt'))
    assert rec['rotation'].strip() == 'trilinear' and float(rec['axis_tilt']) == 0.5 and float(rec['axis_roll']) == 0.0
    assert rec['center'].strip() == 'None' and rec['rotation_matrices'].strip() == 'None'


def test_reconstruct_fullfield_trilinear_multiscale_center(built, tmp_path, monkeypatch):
    """two multiscale levels with an explicit centre: the coarse level runs with center / 2, the fine one with center"""
    from beyond_dof_amd import fullfield, h5io
    monkeypatch.chdir(tmp_path)
    od, ob, prj = _entry_data(30.4)
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', prj)
    seen = []
    real = fullfield.FullfieldSolver

    def recording(*args, **kw):
        seen.append((args[0], kw.get('rotation'), kw.get('center'), kw.get('axis_tilt')))
        return real(*args, **kw)
    monkeypatch.setattr(fullfield, 'FullfieldSolver', recording)
    d, b = fullfield.reconstruct_fullfield('data.h5', theta_st=0, theta_end=2 * np.pi, n_epochs=1, learning_rate=1e-8, minibatch_size=3,
                                           energy_ev=5000, psize_cm=1e-7, free_prop_cm=1e-4, save_path='case', output_folder='out',
                                           initial_guess=[od[::2, ::2, ::2] * 0.9, ob[::2, ::2, ::2] * 0.9], shrink_cycle=None, seed=1,
                                           alpha_d=0., alpha_b=0., gamma=0., rotation='trilinear', axis_tilt=0.5, center=30.4,
                                           multiscale_level=2)
    assert seen == [(32, 'trilinear', 15.2, 0.5), (64, 'trilinear', 30.4, 0.5)]
    assert d.shape == (N, N, N) and np.all(np.isfinite(d)) and np.all(np.isfinite(b))
    for lv in (1, 2):
        assert os.path.exists(os.path.join('case', 'out', 'delta_ds_{}.tiff'.format(lv)))
    assert not [f for f in os.listdir('.') if f.startswith('arrsize_')]
    assert float(_summary(os.path.join('case', 'out', 'summary.txt'))['center']) == 30.4


def test_other_rotations_ignore_the_geometry_keywords(built, tmp_path, monkeypatch):
    """rotation='bilinear' with axis_tilt / center given: the solver is built without them, summary.txt has no geometry lines"""
    from beyond_dof_amd import fullfield, h5io
    monkeypatch.chdir(tmp_path)
    od, ob, prj = _entry_data(None)
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', prj)
    seen = []
    real = fullfield.FullfieldSolver

    def recording(*args, **kw):
        seen.append(sorted(k for k in kw if k in ('axis_tilt', 'axis_roll', 'center', 'rotation_matrices')))
        return real(*args, **kw)
    monkeypatch.setattr(fullfield, 'FullfieldSolver', recording)
    fullfield.reconstruct_fullfield('data.h5', theta_st=0, theta_end=2 * np.pi, n_epochs=1, learning_rate=1e-8, minibatch_size=3, energy_ev=5000,
                                    psize_cm=1e-7, free_prop_cm=1e-4, save_path='case', output_folder='out', initial_guess=[od * 0.9, ob * 0.9],
                                    shrink_cycle=None, seed=1, alpha_d=0., alpha_b=0., gamma=0., rotation='bilinear', axis_tilt=0.5, center=30.4)
    assert seen == [[]]
    assert 'axis_tilt' not in open(os.path.join('case', 'out', 'summary.txt')).read()


# ---- ptychography -----------------------------------------------------------------------------------------------------------------------
def _ptycho_solver(psz, **kw):
    from beyond_dof_amd.solver import PtychoSolver
    p = rr.ptycho_problem(psz)
    s = PtychoSolver(rr.PTY_SHAPE, (psz, psz), rr.PTY_POS, rr.PTY_N_THETA, len(rr.PTY_POS), rr.E_EV, rr.PSIZE_CM, p['pr'], p['pi'],
                     rotation='trilinear', theta=rr.ptycho_theta(), axis_tilt=rr.PTY_TILT, **kw)
    s.set_volume(p['od'], p['ob'])
    return p, s


@pytest.mark.parametrize('psz,kw,f64', [(32, {}, False), (64, dict(engine='streaming'), False), (32, dict(adjoint64='first'), True)],
                         ids=['32-resident', '64-streaming', '32-float64-first-step'])
def test_ptycho_trilinear_forward_loss_and_gradient(built, psz, kw, f64):
    """a (64, 64, 32) volume, one angle under axis_tilt = 0.5, 9 windows (two overhang): waves, loss and gradient against the
    restatement composed with the windows and the far-field model; the gradient bound is the CPU rule's
    (rigid_reference.PTYCHO_GRADIENT_BOUND), intensities and loss 1e-5 as for full field.  engine=None pins the resident engine
    for the 32^2 probe, engine='streaming' the streaming one for 64^2 (PtychoSolver); the third case runs both sweeps in float64"""
    p, s = _ptycho_solver(psz, **kw)
    sel = np.arange(len(rr.PTY_POS))
    w = s.forward(rr.PTY_THETA, sel)
    e_int = rel(np.abs(w) ** 2, np.abs(p['wave']) ** 2)
    loss = s.loss_and_grad(rr.PTY_THETA, sel, p['meas'], f64=f64)
    gd, gb = s.gradient_to_host()
    e_loss, e_gd, e_gb = abs(loss - p['loss']) / abs(p['loss']), rel(gd, p['gd']), rel(gb, p['gb'])
    print('probe', psz, kw, 'intensity', e_int, 'loss', e_loss, 'g_delta', e_gd, 'g_beta', e_gb, 'bound', rr.PTYCHO_GRADIENT_BOUND[psz])
    assert e_int <= 1e-5 and e_loss <= 1e-5
    assert e_gd <= rr.PTYCHO_GRADIENT_BOUND[psz] and e_gb <= rr.PTYCHO_GRADIENT_BOUND[psz]


def test_ptycho_trilinear_steps_lower_the_loss(built):
    """two Adam steps from 0.9 x the object on 3 % data: the loss goes down, whole-volume and slab-wise sharded runs agree bit for bit"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_fullfield import _LoopbackComm
    p = rr.ptycho_problem(32)
    rng = np.random.default_rng(12)
    meas = (np.abs(p['wave']) * (1 + 0.03 * rng.normal(size=p['wave'].shape))).astype(np.float32)
    sel = np.arange(len(rr.PTY_POS))
    vols = []
    for comm, kw in ((None, {}), (_LoopbackComm(), dict(n_slabs=4, sharded=True))):
        _, s = _ptycho_solver(32, comm=comm)
        s.set_volume(p['od'] * 0.9, p['ob'] * 0.9)
        s.reset_moments()
        l0 = s.step(0, rr.PTY_THETA, sel, meas, 1e-8, want_loss=True, **kw)
        s.step(1, rr.PTY_THETA, sel, meas, 1e-8, **kw)
        assert s.loss_and_grad(rr.PTY_THETA, sel, meas) < l0
        vols.append(s.get_volume())
    assert np.array_equal(vols[0][0], vols[1][0]) and np.array_equal(vols[0][1], vols[1][1])


def test_reconstruct_ptychography_trilinear(built, tmp_path, monkeypatch):
    """the entry point: data by the float64 composition at every angle, one epoch from 0.9 x truth moves towards the truth, writes
    no lookup-table folder and records the geometry"""
    from beyond_dof_amd import h5io, util
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    import reference_model as ref_model
    monkeypatch.chdir(tmp_path)
    psz = 32
    p = rr.ptycho_problem(psz)
    theta = -np.linspace(0, 2 * np.pi, rr.PTY_N_THETA, dtype='float32')
    prm = util.rigid_geometry(theta, rr.PTY_SHAPE, rr.PTY_TILT)
    obj = np.stack([p['od'], p['ob']], axis=3)
    data = []
    for q in prm:
        subs = rr.ptycho_windows(rr.rotate_volume(obj, q), psz)
        data.append(ref_model.forward(subs[..., 0], subs[..., 1], p['pr'], p['pi'], rr.E_EV, rr.PSIZE_CM, 'inf')[0])
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', np.stack(data).astype(np.complex64))
    d, b = reconstruct_ptychography('data.h5', rr.PTY_POS, (psz, psz), rr.PTY_SHAPE, theta_st=0, theta_end=2 * np.pi, n_epochs=1,
                                    learning_rate=1e-8, minibatch_size=len(rr.PTY_POS), energy_ev=rr.E_EV, psize_cm=rr.PSIZE_CM,
                                    save_path='case', output_folder='out', initial_guess=[p['od'] * 0.9, p['ob'] * 0.9], seed=1,
                                    probe_type='gaussian', probe_mag_sigma=psz / 10., probe_phase_sigma=psz / 10., probe_phase_max=0.5,
                                    rotation='trilinear', axis_tilt=rr.PTY_TILT)
    assert d.shape == rr.PTY_SHAPE and os.path.exists(os.path.join('case', 'out', 'delta_ds_1.tiff'))
    assert not [f for f in os.listdir('.') if f.startswith('arrsize_')]
    assert np.linalg.norm(d - p['od']) < np.linalg.norm(0.9 * p['od'] - p['od'])
    rec = _summary(os.path.join('case', 'out', 'summary.txt'))
    assert rec['rotation'].strip() == 'trilinear' and float(rec['axis_tilt']) == rr.PTY_TILT and rec['center'].strip() == 'None'
