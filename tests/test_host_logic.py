"""Host-side set-up code of the product (beyond_dof_amd/util.py, comm.py) against the golden vectors
captured from the reference and against the oracle.  No GPU needed."""
import os

import numpy as np
import pytest

from beyond_dof_amd import util
from beyond_dof_amd.comm import minibatch_schedule, PseudoComm
from oracle import bdof_oracle as orc


def test_get_kernel_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g1_get_kernel.npz'))
    for key in g.files:
        _, Y, X, dist = key.split('_')
        H = util.get_kernel(float(dist), 0.248, [1., 1., 1.], [int(Y), int(X), 4])
        np.testing.assert_allclose(H, g[key], rtol=0, atol=1e-13)


def test_get_kernel_anisotropic_voxels_match_oracle():
    H = util.get_kernel(3.0, 0.3, [1.5, 2.5, 1.0], [10, 12])
    np.testing.assert_allclose(H, orc.get_kernel(3.0, 0.3, [1.5, 2.5, 1.0], [10, 12, 1]), rtol=0, atol=1e-14)


def test_device_transfer_function_is_the_fft_domain_multiplier():
    ny, nx = 8, 16
    hs = util.device_transfer_function(1.0, 0.248, [1., 1., 1.], ny, nx)
    rng = np.random.default_rng(0)
    w = rng.normal(size=(1, ny, nx)) + 1j * rng.normal(size=(1, ny, nx))
    ref = orc._propagate(w, orc.get_kernel(1.0, 0.248, [1., 1., 1.], (ny, nx, 1)))
    mine = np.fft.fft2(w[0]) * (hs * nx * ny)
    mine = np.fft.ifft2(mine)
    np.testing.assert_allclose(mine, ref[0], rtol=0, atol=5e-7)


def test_rotation_lookup_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g3_rotation.npz'))
    for size, n in [((8, 8, 8), 5), ((64, 64, 64), 4), ((6, 10, 10), 7)]:
        key = 'x'.join(map(str, size)) + '_n{}'.format(n)
        assert np.array_equal(np.stack(util.rotation_lookup(list(size), n)), g['coords_' + key])


def test_save_rotation_lookup_files(tmp_path, golden_dir):
    g = np.load(os.path.join(golden_dir, 'g3_rotation.npz'))
    folder = str(tmp_path / 'tables')
    util.save_rotation_lookup([8, 8, 8], 5, dest_folder=folder)
    coords = util.read_all_origin_coords(folder, 5)
    assert np.array_equal(np.stack(coords), g['coords_8x8x8_n5'])
    c0, c1, c2 = [np.load(os.path.join(folder, 'coord{}_vec.npy'.format(i))) for i in range(3)]
    # the flat (i0, i1, i2) enumeration apply_rotation relies on (cnn_propagator/util.py:386-396)
    assert np.array_equal(c0, np.repeat(np.arange(8), 64))
    assert np.array_equal(c1, np.tile(np.repeat(np.arange(8), 8), 8))
    assert np.array_equal(c2, np.tile(np.arange(8), 64))


def test_device_rotation_tables_gather_and_inverse():
    ny, nx, nz, n_theta = 4, 9, 9, 6
    coords = util.rotation_lookup([ny, nx, nz], n_theta)
    tab, off, order = util.device_rotation_tables(coords, nx, nz)
    rng = np.random.default_rng(0)
    obj = rng.normal(size=(ny, nx, nz, 2))
    rows = util.volume_to_rows(obj[..., 0], obj[..., 1]).reshape(nx * nz, ny, 2)
    for a in range(n_theta):
        rot = orc.apply_rotation(obj, coords[a])                    # (Y, X, Z, 2)
        mine = rows[tab[a]]                                         # [z][x][y][2]
        np.testing.assert_array_equal(mine.transpose(2, 1, 0, 3), rot.astype(np.float32))
        # inverse table: every destination lists exactly the rotated rows gathered from it
        dest = tab[a].reshape(-1)
        for d in range(nx * nz):
            src = order[a][off[a][d]:off[a][d + 1]]
            assert np.array_equal(np.sort(src), np.flatnonzero(dest == d))
        assert off[a][-1] == nx * nz


def test_layout_round_trips():
    rng = np.random.default_rng(1)
    d, b = rng.normal(size=(3, 4, 5)), rng.normal(size=(3, 4, 5))
    d2, b2 = util.rows_to_volume(util.volume_to_rows(d, b))
    np.testing.assert_array_equal(d2, d.astype(np.float32))
    np.testing.assert_array_equal(b2, b.astype(np.float32))
    gd, gb = rng.normal(size=(2, 3, 4, 5)), rng.normal(size=(2, 3, 4, 5))
    r = util.batch_to_rows(gd, gb)
    assert r.shape == (2, 5, 4, 3, 2)
    gd2, gb2 = util.rows_to_batch(r)
    np.testing.assert_array_equal(gd2, gd.astype(np.float32))


def test_split_tasks_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g6_split_tasks.npz'))
    parts = util.split_tasks(g['arr'], int(g['split_size']))
    assert [len(p) for p in parts] == list(g['lengths'])


def test_minibatch_schedule_pads_and_partitions():
    rng = np.random.default_rng(0)
    sched = minibatch_schedule(23, size=2, minibatch_size=4, rng=rng)
    assert all(len(c) == 8 for c in sched) and len(sched) == 3
    assert all(np.all(np.diff(c) >= 0) for c in sched)
    flat = np.concatenate(sched)
    assert set(flat.tolist()) == set(range(23))          # every angle is visited, one is repeated as padding
    assert len(flat) == 24
    assert PseudoComm().size == 1


def test_gaussian_probe_matches_oracle():
    a = util.gaussian_probe((7, 9), 2.0, 3.0, 0.5)
    b = orc.gaussian_probe((7, 9), 2.0, 3.0, 0.5)
    np.testing.assert_allclose(a[0], b[0])
    np.testing.assert_allclose(a[1], b[1])


def test_conv_kernel_separable_matches_reference_recipe():
    """The separable taps reproduce the reference's 2-D kernel (propagation.py:35-44) restated in the oracle."""
    for shape, ks in [((64, 64, 8), 17), ((64, 128, 8), 5), ((96, 64, 4), 9)]:
        ky, kx, e = util.conv_kernel_separable(1.0, 0.248, np.array([1., 1., 1.]), shape, ks)
        k2 = orc.conv_kernel_2d(1.0, 0.248, np.array([1., 1., 1.]), np.array(shape), ks)
        np.testing.assert_allclose(e * np.outer(ky, kx), k2, rtol=0, atol=1e-13 * np.abs(k2).max())


def test_ptychography_epoch_schedule():
    """cnn_propagator/ptychography.py:269-282: every angle once, in shuffled order; each angle's position list padded to a
    multiple of the minibatch with positions drawn from its own head, so that minibatches never mix angles."""
    from beyond_dof_amd.ptychography import epoch_schedule
    n_theta, n_pos, mb = 5, 23, 4
    sched = epoch_schedule(n_theta, n_pos, mb, np.random.RandomState(3))
    per_theta = 24
    assert sched.shape == (n_theta * per_theta, 2)
    assert sorted(set(sched[:, 0].tolist())) == list(range(n_theta))
    for i in range(n_theta):
        blk = sched[i * per_theta:(i + 1) * per_theta]
        assert len(set(blk[:, 0].tolist())) == 1                       # one angle per block -> per minibatch
        assert np.array_equal(blk[:n_pos, 1], np.arange(n_pos))
        assert np.all(blk[n_pos:, 1] < n_pos - n_pos % mb)             # padding drawn from spots[:-(n_pos % mb)]
    again = epoch_schedule(n_theta, n_pos, mb, np.random.RandomState(3))
    assert np.array_equal(sched, again)                                # every rank derives the same schedule from the seed
    exact = epoch_schedule(2, 8, 4, np.random.RandomState(0))
    assert exact.shape == (16, 2)


def test_rotation_tables_square_and_non_square():
    """util.rotation_lookup equals the reference's tables (oracle restatement, golden vector G3) whenever the rotation plane is
    square (X = Z) — every case the reference drivers run.  For X != Z the reference enumerates the new coordinates with
    np.reshape(np.tile(coord1, Z), [X, Z]) (cnn_propagator/util.py:304-306), which is only the intended repeat when X = Z:
    its (x, z) pairs then repeat some voxels and skip others, i.e. the rotated object is scrambled.  The product keeps the
    intended enumeration there — a deliberate deviation, found by executing the reference's loop on a (64, 64, 32) object."""
    from oracle import bdof_oracle as orc
    for size in ([8, 8, 8], [6, 10, 10], [12, 5, 5]):
        assert all(np.array_equal(a, b) for a, b in zip(orc.rotation_lookup(size, 5), util.rotation_lookup(size, 5)))
    size = [8, 10, 6]
    ours = util.rotation_lookup(size, 1)[0]                       # theta = 0: the identity map of the enumeration
    pairs = set(map(tuple, ours))
    assert len(pairs) == size[1] * size[2]                        # every (x, z) once
    theirs = orc.rotation_lookup(size, 1)[0]
    assert len(set(map(tuple, theirs))) < size[1] * size[2]       # the reference's enumeration repeats pairs


def test_point_probe_is_refused_by_both_entry_points(tmp_path):
    """probe_type='point' needs the spherical-wave propagator (cnn_propagator/fullfield.py:298-301 says so itself): refused by
    reconstruct_fullfield as by the simulators, before anything touches a GPU."""
    import pytest
    from beyond_dof_amd import h5io
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    h5io.write_dataset(str(tmp_path / 'data.h5'), 'exchange/data', np.ones((2, 8, 8), dtype=np.complex64))
    with pytest.raises(ValueError, match='point'):
        reconstruct_fullfield('data.h5', save_path=str(tmp_path), n_epochs=1, minibatch_size=1, probe_type='point',
                              initial_guess=[np.zeros((8, 8, 8)), np.zeros((8, 8, 8))])


def test_adjoint_precision_values_are_checked_before_anything_touches_a_gpu(tmp_path):
    """adjoint_precision: 'float32' | 'float64' | 'first-step' in both entry points (the first minibatch of an epoch through the
    model's float64 path); anything else is a ValueError at the top of the call."""
    import pytest
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    with pytest.raises(ValueError, match='adjoint_precision'):
        reconstruct_fullfield('data.h5', save_path=str(tmp_path), n_epochs=1, minibatch_size=1, adjoint_precision='double')
    with pytest.raises(ValueError, match='adjoint_precision'):
        reconstruct_ptychography('data.h5', [(4, 4)], (4, 4), (8, 8, 8), save_path=str(tmp_path), n_epochs=1, minibatch_size=1,
                                 adjoint_precision='first')


def test_rotation_keywords_of_the_entry_points():
    """util.RotationKeywords, the one reader of rotation / axis_tilt / axis_roll / center / rotation_matrices for both entry points:
    per multiscale level an explicit centre and column 3 of every (3, 4) matrix divide by ds_level, a None centre stays None; the
    angle selection is applied before check_rigid; what is not rigid is a ValueError; each entry point's rule for the rotation
    keyword is the one it always had."""
    import pytest
    from beyond_dof_amd import ptychography
    from beyond_dof_amd.solver import FullfieldSolver, PtychoSolver
    c, s = 0.6, 0.8                                                    # an exact rotation about y by a 3-4-5 angle
    M = np.array([[c, s, 0.], [-s, c, 0.], [0., 0., 1.]])
    mats = np.stack([np.concatenate([M if i % 2 else np.eye(3), [[8. * i + 4.], [-16.], [2.]]], axis=1) for i in range(4)])
    geo = util.RotationKeywords(dict(rotation='trilinear', axis_tilt=0.5, axis_roll='0.25', center=30, rotation_matrices=mats.tolist()))
    assert geo.rotation == 'trilinear' and geo.trilinear
    with pytest.raises(ValueError, match=r'\(2, 3, 4\)'):            # four matrices for two angles: the selection comes first
        util.RotationKeywords(dict(rotation='trilinear', rotation_matrices=mats)).select(2)
    geo.select(2, slice(None, None, 2))                                # theta_downsample = 2 keeps angles 0 and 2
    for ds, center, t0 in ((1, 30., [4., 20.]), (2, 15., [2., 10.]), (4, 7.5, [1., 5.])):
        kw = geo.for_level(ds)
        assert sorted(kw) == ['axis_roll', 'axis_tilt', 'center', 'rotation_matrices']
        assert kw['axis_tilt'] == 0.5 and kw['axis_roll'] == 0.25 and kw['center'] == center
        m = kw['rotation_matrices']
        assert m.shape == (2, 3, 4) and np.array_equal(m[:, :, :3], np.stack([np.eye(3)] * 2))      # only column 3 is divided
        assert np.array_equal(m[:, 0, 3], t0) and np.array_equal(m[:, 1, 3], [-16. / ds] * 2) and np.array_equal(m[:, 2, 3], [2. / ds] * 2)
    assert np.array_equal(geo.for_level(1)['rotation_matrices'], mats[::2])                     # a level does not change the record
    # an index array selects as a slice does (reconstruct_ptychography); no centre, no matrices
    odd = util.RotationKeywords(dict(rotation='trilinear', rotation_matrices=mats))
    odd.select(2, np.array([1, 3]))
    assert np.array_equal(odd.for_level(2)['rotation_matrices'][:, :, :3], np.stack([M] * 2))
    assert np.array_equal(odd.for_level(2)['rotation_matrices'][:, 0, 3], [6., 14.])
    plain = util.RotationKeywords(dict(rotation='trilinear'))
    plain.select(3)
    assert all(plain.for_level(ds) == dict(axis_tilt=0., axis_roll=0., center=None) for ds in (1, 2, 4))
    sheared = mats.copy()
    sheared[1, 0, 1] += 1e-3
    with pytest.raises(ValueError, match='rigid'):
        util.RotationKeywords(dict(rotation='trilinear', rotation_matrices=sheared)).select(4)
    util.RotationKeywords(dict(rotation='trilinear', rotation_matrices=sheared)).select(2, slice(None, None, 2))     # ... of a kept angle only
    # the geometry is ignored with any other rotation, whatever it holds
    for rot in ('nearest', 'bilinear'):
        other = util.RotationKeywords(dict(rotation=rot, center=3, rotation_matrices=sheared))
        other.select(2)
        assert other.rotation == rot and other.for_level(2) == {}
    # reconstruct_fullfield hands any value on (the solver refuses what it does not know); reconstruct_ptychography acts on
    # 'trilinear' alone and ignores every other value
    assert util.RotationKeywords({}).rotation == 'nearest' and util.RotationKeywords(dict(rotation='cubic')).rotation == 'cubic'
    assert ptychography.ROTATIONS == ('trilinear',)
    assert [util.RotationKeywords(dict(rotation=r), only=ptychography.ROTATIONS).rotation for r in ('trilinear', 'nearest', 'bilinear', 'cubic', None)] \
        == ['trilinear', 'nearest', 'nearest', 'nearest', 'nearest']
    assert util.RotationKeywords({}, only=ptychography.ROTATIONS).rotation == 'nearest'
    with pytest.raises(ValueError, match="rotation must be 'nearest', 'bilinear' or 'trilinear'"):
        FullfieldSolver(8, 8, 8, 2, 1, 5000., 1e-7, rotation='cubic')
    with pytest.raises(ValueError, match="rotation must be 'nearest' or 'trilinear'"):
        PtychoSolver((8, 8, 8), (4, 4), [(4, 4)], 2, 1, 5000., 1e-7, np.ones((4, 4)), np.zeros((4, 4)), rotation='bilinear')


def test_tiled_propagator_auto_halo():
    """TiledPropagator(halo='auto') (host arithmetic only): 64 pixels for plain stitching; with the long-range correction twice the
    band edge's reach over one 16-slice range plus 16 pixels — 24 at 5 keV / 1 nm (81 tiles of 512^2 on the 4096^2 field) — or plus 40
    where the tiles ride on per-tile carriers (48: 100 tiles, of which the few that touch the object run)."""
    from beyond_dof_amd.tiling import TiledPropagator

    class Probe(TiledPropagator):
        def __init__(self, n_slice, tile):
            self.n_slice, self.tile = n_slice, tile
    assert Probe(1024, 512)._auto_halo(5000., 1e-7, 0.5, None, 'auto', None) == 24           # full-amplitude float32 sweeps (gradient)
    assert Probe(1024, 512)._auto_halo(5000., 1e-7, 0.5, None, 'auto', None, True) == 48     # per-tile carriers (the forward model)
    assert Probe(1024, 512)._auto_halo(5000., 1e-7, 0.5, None, False, None) == 64
    assert Probe(96, 512)._auto_halo(5000., 1e-7, 0.5, None, 'auto', None, True) == 64       # one plain range: no correction
    assert Probe(1024, 128)._auto_halo(5000., 1e-7, 0.5, None, 'auto', None) == 24
    assert Probe(1024, 64)._auto_halo(5000., 1e-7, 0.5, None, True, None, True) == 16        # never more than a quarter of the tile
    assert (-(-4096 // (512 - 2 * 24))) ** 2 == 81 and (-(-4096 // (512 - 2 * 48))) ** 2 == 100


def test_detector_kernel_choice_and_impulse_response_table(golden_dir):
    """SURVEY §8 a3 on the host: 'TF' / 'IR' / 'auto' for the detector step (cnn_propagator/np_funcs.py:51-61: the criterion is
    computed there and then overridden with 'TF'); the device table of the 'IR' choice is get_kernel_ir (golden vector G8) in
    the layout of every other table; the oracle's 'IR' branch multiplies by that kernel."""
    import os
    import pytest
    from oracle import bdof_oracle as orc
    assert util.detector_kernel_kind('TF', 1e3, 0.248, [1., 1., 1.], (64, 64)) == 'TF'
    assert util.detector_kernel_kind('IR', 1.0, 0.248, [1., 1., 1.], (64, 64)) == 'IR'
    assert util.detector_kernel_kind('auto', 1e3, 0.248, [1., 1., 1.], (64, 64)) == 'IR'      # lambda z / L = 3.9 nm > 1 nm voxels
    assert util.detector_kernel_kind('auto', 10., 0.248, [1., 1., 1.], (64, 64)) == 'TF'
    with pytest.raises(ValueError):
        util.detector_kernel_kind('exact', 1e3, 0.248, [1., 1., 1.], (64, 64))
    g = np.load(os.path.join(golden_dir, 'g8_kernel_ir_upsample.npz'))
    t = util.device_transfer_function(1000., 0.248, [1., 1., 1.], 32, 32, kernel='IR', dtype=np.complex128)
    np.testing.assert_allclose(t, np.fft.ifftshift(g['Hir_32_32_1000']) / 1024., rtol=0, atol=1e-12 * np.abs(g['Hir_32_32_1000']).max())
    dc = util.transfer_function_dc(1000., 0.248, [1., 1., 1.], 32, 32, kernel='IR')
    assert abs(complex(*dc) - np.fft.ifftshift(g['Hir_32_32_1000'])[0, 0]) <= 1e-12 * abs(complex(*dc))
    with pytest.raises(ValueError):
        util.device_transfer_function(1000., 0.248, [1., 1., 1.], 32, 32, kernel='IR', field_shape=(64, 64))
    # oracle: the IR branch is the same propagation with the other multiplier
    rng = np.random.default_rng(0)
    d = rng.uniform(0, 1e-5, size=(1, 16, 16, 3))
    one, zero = np.ones((16, 16)), np.zeros((16, 16))
    none, _ = orc.multislice_propagate_batch_numpy(d, 0.1 * d, one, zero, 5000., 1e-7, None, d.shape)
    ir, _ = orc.multislice_propagate_batch_numpy(d, 0.1 * d, one, zero, 5000., 1e-7, 1e-4, d.shape, detector_kernel='IR')
    want = orc._propagate(none, orc.get_kernel_ir(1000., 0.248, np.array([1., 1., 1.]), (16, 16, 3)))
    np.testing.assert_allclose(ir, want, rtol=0, atol=1e-13)


def test_summary_columns_and_build_id(tmp_path):
    """summary.txt keeps the reference's '{:<20}{}' layout (cnn_propagator/misc.py:61-77) and still separates a name that fills the
    column from its value; _lib.build_id names what a measurement belongs to."""
    from beyond_dof_amd.misc import create_summary
    from beyond_dof_amd import _lib
    create_summary(str(tmp_path), {'obj_size': (8, 8, 8), 'adjoint_precision': 'first-step', 'adjoint_precision_effective': 'float32'}, preset='ptycho')
    rows = dict(line.split(None, 1) for line in open(str(tmp_path / 'summary.txt')).read().splitlines() if len(line.split(None, 1)) == 2)
    assert rows['obj_size'].strip() == '(8, 8, 8)' and rows['adjoint_precision'].strip() == 'first-step'
    assert rows['adjoint_precision_effective'].strip() == 'float32'
    assert open(str(tmp_path / 'summary.txt')).read().splitlines()[0] == '{:<20}{}'.format('obj_size', '(8, 8, 8)')
    b = _lib.build_id()
    assert set(b) == {'source_sha256', 'flags', 'lib_sha256'} and len(b['source_sha256']) == 16


def test_optics_record_hands_out_the_parent_expressions_bit_for_bit():
    """util.Optics against the expressions the engine and the tiled propagator spelled out before it existed, written here from
    get_kernel / get_kernel_tile / get_kernel_ir and ifftshift with dtype and transposition: np.array_equal, no tolerance.
    Both forms of psize_cm, with and without field_shape, 'TF' and 'IR', free_prop_cm None / a distance / 'inf'."""
    import itertools
    import pytest
    ifs, c64, c128 = np.fft.ifftshift, np.complex64, np.complex128
    energy_ev, ny, nx = 5000., 12, 16
    for psize_cm, fs, free_prop_cm, pi in itertools.product((1e-7, (1.5e-7, 2.5e-7, 2e-7)), (None, (40, 48)), (None, 1e-4, 'inf'),
                                                            (util.PI, np.pi)):
        o = util.Optics(energy_ev, psize_cm, free_prop_cm, pi, ny, nx, fs)
        voxel_nm = np.array([psize_cm] * 3) * 1.e7 if np.isscalar(psize_cm) else np.array(psize_cm) * 1.e7
        lmbda_nm = 1240. / energy_ev
        delta_nm = voxel_nm[-1]
        assert np.array_equal(o.voxel_nm, voxel_nm) and o.lmbda_nm == lmbda_nm and o.delta_nm == delta_nm == voxel_nm[2]
        assert o.k == 2. * pi * delta_nm / lmbda_nm and o.pi == pi and o.field_shape == fs and (o.ny, o.nx) == (ny, nx)

        def whole(d):
            return util.get_kernel(d, lmbda_nm, voxel_nm, (ny, nx), pi=pi)

        def tile(d):            # what a tile of the field applies; the field's own mesh without field_shape
            return util.get_kernel_tile(d, lmbda_nm, voxel_nm, (ny, nx), fs, pi=pi) if fs is not None else whole(d)

        # the slice step
        assert np.array_equal(o.slice_kernel(tiled=True), tile(delta_nm))
        assert np.array_equal(o.slice_kernel(tiled=False), whole(delta_nm))
        hs64 = o.table(delta_nm, tiled=True, dtype=c128)                           # set_physics: bdof_set_transfer_f64
        assert hs64.dtype == c128 and hs64.flags.c_contiguous
        assert np.array_equal(hs64, np.ascontiguousarray((ifs(tile(delta_nm)) / float(nx * ny)).astype(c128)))
        assert np.array_equal(hs64.astype(c64), np.ascontiguousarray((ifs(tile(delta_nm)) / float(nx * ny)).astype(c128)).astype(c64))
        t = o.table(delta_nm, tiled=True)                                          # complex64 is the default
        assert t.dtype == c64 and np.array_equal(t, (ifs(tile(delta_nm)) / float(nx * ny)).astype(c64))
        t = o.table(delta_nm, tiled=True, transpose=True, dtype=c128)              # enable_tf_f64; the tiled propagator's [kx][ky]
        assert t.flags.c_contiguous and np.array_equal(t, np.ascontiguousarray(hs64.T))
        assert np.array_equal(t, np.ascontiguousarray((ifs(tile(delta_nm)) / float(nx * ny)).T.astype(c128)))
        t = o.table(delta_nm * 7, tiled=True, dtype=c64)                           # tiling: 7 steps, the fused kernels' layout
        assert np.array_equal(t, np.ascontiguousarray((ifs(tile(delta_nm * 7)) / float(nx * ny)).astype(c64)))
        t = o.table(delta_nm, tiled=False, fold=False, dtype=c128)                 # the host's carrier stack
        assert np.array_equal(t, ifs(whole(delta_nm)))
        t = o.table(delta_nm, tiled=True, fold=False, transpose=True, dtype=c128)  # bdof_set_probe_field
        assert t.flags.c_contiguous and np.array_equal(t, np.ascontiguousarray(ifs(tile(delta_nm)).T.astype(c128)))
        dc = o.dc(delta_nm, tiled=True)
        assert dc.shape == (2,) and complex(*dc) == complex(ifs(tile(delta_nm))[0, 0])
        assert np.array_equal(dc, np.array(util.transfer_function_dc(delta_nm, lmbda_nm, voxel_nm, ny, nx, pi=pi, field_shape=fs)))

        # the step to the detector
        if free_prop_cm is None or free_prop_cm == 'inf':
            assert o.det_nm is None
            continue
        dist = free_prop_cm * 1e7
        assert o.det_nm == dist
        ir = util.get_kernel_ir(dist, lmbda_nm, voxel_nm, (ny, nx), pi=pi)
        assert np.array_equal(o.detector_kernel('TF'), whole(dist)) and np.array_equal(o.detector_kernel('TF', tiled=True), tile(dist))
        assert np.array_equal(o.detector_kernel('IR'), ir)
        for kind, centred in (('TF', whole(dist)), ('IR', ir)):
            for dtype in (c64, c128):                                              # set_physics / its adjoint64 table
                t = o.table(dist, kind, dtype=dtype)
                assert t.dtype == dtype and np.array_equal(t, np.ascontiguousarray((ifs(centred) / float(nx * ny)).astype(dtype)))
            t = o.table(dist, kind, transpose=True, dtype=c128)                    # enable_tf_f64 / enable_conv_f64
            assert t.flags.c_contiguous
            assert np.array_equal(t, np.ascontiguousarray(np.ascontiguousarray((ifs(centred) / float(nx * ny)).astype(c128)).T))
            assert np.array_equal(o.table(dist, kind, fold=False, dtype=c128), ifs(centred))       # the carrier stacks on the host
            t = o.table(dist, kind, fold=False, transpose=True, dtype=c128)
            assert np.array_equal(t, np.ascontiguousarray(ifs(centred).T.astype(c128)))
            assert complex(*o.dc(dist, kind)) == complex(ifs(centred)[0, 0])
        t = o.table(dist, 'TF', tiled=True, fold=False, transpose=True, dtype=c128)                # bdof_set_probe_field, 'TF'
        assert np.array_equal(t, np.ascontiguousarray(ifs(tile(dist)).T.astype(c128)))
        if fs is not None:
            with pytest.raises(ValueError):
                o.detector_kernel('IR', tiled=True)                                # the impulse response is a whole field's
    with pytest.raises(ValueError, match='free_prop_cm'):
        util.Optics(energy_ev, 1e-7, 'far', util.PI, ny, nx)


def test_engine_host_state_is_declared_and_the_loss_call_is_single():
    """The static conditions of the host clean-up: the scalar-or-triple pixel size is converted in one place, the engine and the
    solvers no longer ask their own objects what they hold, and each bdof_loss_grad* entry point is called from one place."""
    import re
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'beyond_dof_amd')
    src = {f: open(os.path.join(pkg, f)).read() for f in sorted(os.listdir(pkg)) if f.endswith('.py')}
    assert sum(s.count('np.isscalar(psize_cm)') for s in src.values()) == 1 and 'np.isscalar(psize_cm)' in src['util.py']
    assert 'getattr(self, ' not in src['engine.py'] and 'hasattr(self, ' not in src['engine.py']
    assert 'getattr(self.eng, ' not in src['solver.py']
    assert not any('_physics_args' in s or '_tf64_args' in s for s in src.values())
    calls = [m for f, s in src.items() if f != '_lib.py' for m in re.findall(r'lib\.(bdof_loss_grad\w*)', s)]
    assert sorted(calls) == ['bdof_loss_grad', 'bdof_loss_grad_conv', 'bdof_loss_grad_conv_f64', 'bdof_loss_grad_tf_f64']
    from beyond_dof_amd.engine import MultisliceEngine
    assert callable(MultisliceEngine._reset_host_state) and callable(MultisliceEngine.loss_grad_device)


def _probe_apply_before_hostopt(self, b1=0.9, b2=0.999, eps=1e-8):
    """_VolumeSolver._probe_apply as it stood before hostopt.ProbeVariable, verbatim"""
    if self.probe is None or self._pacc == 0:
        return
    self.ctx.sync()
    g = np.ascontiguousarray(np.swapaxes(self._pgrad.download(), -2, -1)).astype(np.complex128) / self._pacc
    self._pacc = 0
    if self.comm.size > 1:
        g = self.comm.allreduce_sum_host(g) / self.comm.size
    self.probe_t += 1
    self.probe_m = b1 * self.probe_m + (1 - b1) * g
    self.probe_v = b2 * self.probe_v + (1 - b2) * (g.real ** 2 + 1j * g.imag ** 2)
    mh = self.probe_m / (1 - b1 ** self.probe_t)
    vh = self.probe_v / (1 - b2 ** self.probe_t)
    self.probe = self.probe - self.probe_lr * (mh.real / (np.sqrt(vh.real) + eps) + 1j * mh.imag / (np.sqrt(vh.imag) + eps))
    if self.pupil is not None:
        self.probe = self.probe * self.pupil
    self._probe_to_engine()


@pytest.mark.parametrize('pupil', [False, True], ids=['no_pupil', 'pupil'])
@pytest.mark.parametrize('shape', [(8, 8), (3, 8, 8)], ids=['probe', 'modes'])
def test_probe_variable_has_the_bits_of_the_update_it_replaced(shape, pupil):
    """hostopt.ProbeVariable behind the solver's _probe_collect / _probe_apply, on an object without a device: four steps of two
    accumulated minibatches each, the other of two ranks' gradients added by a stand-in communicator.  probe, probe_m, probe_v,
    probe_t and what the engine is handed: the same bits as the complex Adam that stood in the solver."""
    import types
    from beyond_dof_amd.hostopt import ProbeVariable
    from beyond_dof_amd.solver import _VolumeSolver
    rng = np.random.default_rng(21)
    cplx = lambda s: rng.normal(size=s) + 1j * rng.normal(size=s)
    handed = []

    class Comm(object):
        size, other = 2, None

        def allreduce_sum_host(self, a):
            return a + self.other

    class Engine(object):          # the device accumulator of the probe gradient, [x][y] per plane, complex64
        acc = None

        def probe_grad(self, accumulate, to_host):
            assert not to_host
            g = cplx(shape).astype(np.complex64)
            self.acc = self.acc + g if accumulate else g
            return types.SimpleNamespace(download=lambda: self.acc.copy())

        def set_probe(self, re, im):
            handed.append(('probe', re + 1j * im))

        def set_probe_modes(self, re, im):
            handed.append(('modes', re + 1j * im))

    start = cplx(shape)
    pupil = (rng.uniform(size=(8, 8)) > 0.3).astype(np.float64) if pupil else None
    comm, ctx = Comm(), types.SimpleNamespace(sync=lambda: None)
    s = _VolumeSolver.__new__(_VolumeSolver)
    s.comm, s.ctx, s.eng, s.pvar = comm, ctx, Engine(), ProbeVariable(start.copy(), 2e-3, pupil)
    old = types.SimpleNamespace(comm=comm, ctx=ctx, probe=start.copy(), probe_lr=2e-3, pupil=pupil, probe_m=np.zeros_like(start),
                                probe_v=np.zeros_like(start), probe_t=0, _probe_to_engine=lambda: None)
    s._probe_apply()                                    # nothing collected: nothing moves
    assert s.probe_t == 0 and np.array_equal(s.probe, start) and not handed
    for step in range(4):
        s._probe_collect()
        s._probe_collect()
        old._pgrad, old._pacc = types.SimpleNamespace(download=lambda: s.eng.acc.copy()), 2
        comm.other = cplx(shape)
        _probe_apply_before_hostopt(old)
        s._probe_apply()
        assert s.pvar.n_acc == 0 and s.probe_t == old.probe_t == step + 1
        assert np.array_equal(s.probe, old.probe) and np.array_equal(s.probe_m, old.probe_m) and np.array_equal(s.probe_v, old.probe_v), step
        assert handed[-1][0] == ('modes' if len(shape) == 3 else 'probe') and np.array_equal(handed[-1][1], old.probe) and len(handed) == step + 1
    assert all(np.array_equal(a, b) for a, b in zip(s.get_probe(), (old.probe.real, old.probe.imag)))
    if pupil is not None:
        assert not np.any(s.probe[..., pupil == 0]) and np.any(s.probe_m[..., pupil == 0])
