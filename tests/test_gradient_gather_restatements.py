"""No device: the numpy restatements that tests/test_gpu_gradient_gathers.py holds the gradient gather kernels to are themselves
checked here — against the oracle's scatter-add on a real rotation table, against the oracle's pad / slice bookkeeping by the
dot-product identity — and every case's geometry and data are shown to discriminate: its preconditions hold (the builders assert
them), and dropping the last window or tile, or moving one origin by one pixel, changes the expected output."""
import numpy as np

from oracle import bdof_oracle as orc

import test_gpu_gradient_gathers as gg


def test_rotation_restatement_is_the_oracles_scatter_add():
    """table-driven scatter-add == orc.apply_rotation_adjoint on orc.rotation_lookup's lists (non-square: X = 9, Z = 12)"""
    ny, nx, nz, n_theta = 6, 9, 12, 5
    from beyond_dof_amd import util
    coords = orc.rotation_lookup([ny, nx, nz], n_theta)
    tab, off, order = util.device_rotation_tables(coords, nx, nz)
    rng = np.random.default_rng(0)
    angles = [3, 1, 3, 4]
    grot = gg.ints(rng, (len(angles), nz * nx, ny, 2))                 # [b][z * nx + x][y][c]
    mine = gg.rot_adjoint_restated(grot, tab, angles)
    want = np.zeros((ny, nx, nz, 2))
    for b, a in enumerate(angles):
        want += orc.apply_rotation_adjoint(np.ascontiguousarray(grot[b].astype(np.float64).reshape(nz, nx, ny, 2).transpose(2, 1, 0, 3)), coords[a])
    assert np.array_equal(mine.reshape(nx, nz, ny, 2).transpose(2, 0, 1, 3), want)
    # the CSR form the kernels read says the same: row d's sources are order[off[d] : off[d + 1]]
    for a in set(angles):
        for d in (0, 17, nx * nz - 1):
            assert sorted(order[a][off[a][d]:off[a][d + 1]]) == sorted(np.nonzero(tab[a].reshape(-1) == d)[0])


def test_window_restatement_is_the_adjoint_of_rotate_pad_and_slice():
    """<W v, g> = <v, W^T g> with W = rotate (table gather), zero-pad, cut one window per origin — the bookkeeping of
    orc.ptycho_loss_and_grad — on integers, so the identity is exact"""
    for shape in gg.WINDOW_SHAPES:
        c = gg.window_case(*shape)
        tab, _, _ = gg.tables_from_dests(c['dests'], c['volNX'], c['S'])
        rng = np.random.default_rng(1)
        vol = rng.integers(-4, 5, size=(c['volNX'] * c['S'], c['volNY'], 2))
        rot = vol[tab[c['angle']].reshape(-1)].reshape(c['S'], c['volNX'], c['volNY'], 2)
        px, py = max(c['NX'], -int(c['xoff'].min())), max(c['NY'], -int(c['yoff'].min()))
        qx, qy = int(c['xoff'].max()) + c['NX'], int(c['yoff'].max()) + c['NY']
        padded = np.pad(rot, ((0, 0), (px, qx), (py, qy), (0, 0)))
        wins = np.stack([padded[:, px + x:px + x + c['NX'], py + y:py + y + c['NY']] for x, y in zip(c['xoff'], c['yoff'])])
        g = c['grot'].astype(np.int64)
        adj = gg.window_adjoint_restated(c['grot'], tab[c['angle']], c['xoff'], c['yoff'], c['volNX'], c['volNY'])
        assert wins.shape == g.shape and np.sum(wins * g) == np.sum(vol * adj) != 0


def _changed(fn, c, keys, B):
    """the expected output changes when the last of the B elements is dropped and when the first origin moves by one"""
    full = fn(c, B, c[keys[0]], c[keys[1]])
    assert not np.array_equal(full, fn(c, B - 1, c[keys[0]], c[keys[1]]))
    for k in (0, 1):
        moved = [c[keys[0]].copy(), c[keys[1]].copy()]
        moved[k][0] += 1
        assert not np.array_equal(full, fn(c, B, *moved))


def test_every_case_discriminates():
    def window(c, B, xoff, yoff):
        tab, _, _ = gg.tables_from_dests(c['dests'], c['volNX'], c['S'])
        return gg.window_adjoint_restated(c['grot'][:B], tab[c['angle']], xoff[:B], yoff[:B], c['volNX'], c['volNY'])

    def tiles(c, B, x0, y0):
        return gg.tiles_grad_restated(c['grot'][:B], c['tab'], x0[:B], y0[:B], c['z0'], c['n_rows'], c['volNY'])

    def cut(c, B, x0, y0):
        return gg.cut_adjoint_restated(c['tiles'][:B], x0[:B], y0[:B], c['FX'], c['FY'])

    for shape in gg.WINDOW_SHAPES:
        _changed(window, gg.window_case(*shape), ('xoff', 'yoff'), gg.window_case(*shape)['B'])
    lim = gg.window_case_limit()
    _changed(window, lim, ('xoff', 'yoff'), 1025)
    _changed(window, lim, ('xoff', 'yoff'), 1024)
    for case in gg.TILE_CASES:
        c = gg.tile_case(*case)
        _changed(tiles, c, ('x0', 'y0'), c['B'])
    for c in (gg.tile_case_grid(), gg.tile_case_cap()):
        _changed(tiles, c, ('x0', 'y0'), c['B'])
    c = gg.cut_case_cap()
    _changed(cut, c, ('x0', 'y0'), c['B'])
    # the cap cases: what a list cut at 1024 entries would lose is not nothing
    assert np.any(tiles(gg.tile_case_cap(), 1100, gg.tile_case_cap()['x0'], gg.tile_case_cap()['y0'])
                  != tiles(gg.tile_case_cap(), 1024, gg.tile_case_cap()['x0'], gg.tile_case_cap()['y0']))
    assert np.any(cut(c, 1100, c['x0'], c['y0']) != cut(c, 1024, c['x0'], c['y0']))


def test_rotation_cases_hold_their_preconditions_and_discriminate():
    """the builders assert the list lengths they promise; a table with two sources of one row swapped to another row, or a batch
    with one angle changed, gives another output"""
    c = gg.rot_case_main()
    tab, off, order = gg.tables_from_dests(c['dests'], c['nx'], c['nz'])
    full = gg.rot_adjoint_restated(c['grot'], tab, c['ang_b'])
    other = c['ang_b'].copy()
    other[-1] = 0
    assert not np.array_equal(full, gg.rot_adjoint_restated(c['grot'], tab, other))
    assert not np.array_equal(full[:, :, :], gg.rot_adjoint_restated(c['grot'][:65], tab, c['ang_b'][:65]))
    # integers far below 2^24 even on the heaviest row, halves included
    assert np.abs(full).max() * 3 < 2 ** 23
    for ny in (130, 516):
        w = gg.rot_case_wide(ny)
        assert w['grot'].shape[2] == ny
    g = gg.rot_case_grid()
    assert g['nx'] * g['nz'] == 16384


def test_bilinear_reference_terms_are_consistent():
    """the tap matrices the bound is formed from reproduce the oracle's own forward and adjoint, and its parameters are the solver's"""
    H, W, ny = gg.BILIN_NXV, gg.BILIN_NZV, 4
    rng = np.random.default_rng(2)
    vol = rng.normal(size=(H, W, ny, 2)).astype(np.float32)
    grot = rng.normal(size=(len(gg.BILIN_ANGLES), W, H, ny, 2)).astype(np.float32)
    ref, bound = gg.bilinear_forward_reference(vol, gg.BILIN_ANGLES)
    terms = gg.bilinear_adjoint_terms(grot, gg.BILIN_ANGLES)
    for b, th in enumerate(gg.BILIN_ANGLES):
        Aw, A1 = gg.bilinear_tap_matrices(th, H, W)
        fwd = (Aw.T @ vol.astype(np.float64).reshape(H * W, -1)).reshape(H, W, ny, 2).transpose(1, 0, 2, 3)
        assert np.abs(fwd - ref[b]).max() <= 1e-13
        adj = (Aw @ grot[b].astype(np.float64).transpose(1, 0, 2, 3).reshape(H * W, -1)).reshape(H, W, ny, 2)
        assert np.abs(adj - terms[b][0]).max() <= 1e-13
        assert A1.sum(axis=0).max() <= 4 and np.all(Aw >= 0)
        assert np.allclose(gg.bilinear_prm([th], H, W)[0], orc.rotate_bilinear_params(th, H, W), rtol=0, atol=0)
    a_ref, a_bound = gg.bilinear_adjoint_reference(terms, 9)
    lhs, rhs = np.sum(ref * grot.astype(np.float64)), np.sum(vol.astype(np.float64) * a_ref)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert np.all(bound >= 0) and np.all(a_bound >= 0) and (bound == 0).any()          # some rotated rows have no tap inside
