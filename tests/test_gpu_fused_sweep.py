"""The fused forward sweep of bdof_loss_grad (bdof_set_sweep_fusion; k_slice_y / k_slice_x, csrc/bdof_kernels.h): one kernel per
slice on lines of alternating direction, through the separable Fresnel step.

What is compared: loss, detector wave and the rotated-frame gradient rows of mode 1 (fused forward sweep) and of mode 0 (the
two-kernel sweep) against the float64 twin on the same context (bdof_loss_grad_tf_f64; the detector wave, which the twin does not
hand out, against the host's float64 restatement).  The fused route's error in the detector wave and in the gradient rows may each
be at most TWICE the two-kernel route's at the same shape — a different rounding sequence of the same length; a real mistake is
orders of magnitude — and every error of both routes must sit within what tests/test_gpu_parity.py asserts for its quantity (loss
1e-5, wave 5e-6, gradient 2e-4, all relative).  The loss is ONE sum, whose relative error (1e-9, where its terms carry 3e-8) is a
chance cancellation of the pixels' errors: the fused route's is held to twice the larger of the two-kernel route's loss error and
its wave error, the error of the terms the sum is made of.  The figures are printed.

Stage 2 of the fused sweep (the adjoint kernels, mode 2) is not part of the library: bdof_set_sweep_fusion(2) runs stage 1 and
bdof_sweep_fused reports 1."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

E_EV, PSIZE, FP = 5000., 1e-7, 1e-4
LOSS_TOL, WAVE_TOL, GRAD_TOL = 1e-5, 5e-6, 2e-4      # tests/test_gpu_parity.py's bounds for the float32 kernels
FACTOR = 2.0
MODES = (1,)                                         # the fused stages the library carries


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope='module')
def engine_mod():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import engine
    return engine


def _probe(rng, Y, X):
    """Nearly uniform (within a quarter of its mean, so that MultisliceEngine.set_probe lets it ride on a scalar carrier), with a
    scattered part of its own."""
    return 1 + 0.02 * rng.normal(size=(Y, X)), 0.02 * rng.normal(size=(Y, X))


def _engine(engine_mod, Y, X, S, B, rng, fp=FP, **kw):
    """A streaming engine (never the LDS-resident one) with a nearly uniform random probe: a scalar carrier and a scattered part."""
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine='streaming', **kw)
    eng.set_physics(E_EV, PSIZE, fp)
    pr, pi = _probe(rng, Y, X)
    eng.set_probe(pr, pi)
    return eng, pr, pi


def _run(eng, B, meas, mode, angle_idx=None, xoff=None, yoff=None, f64=False):
    """One loss + gradient: (loss, detector wave (B, Y, X) or None for the twin, g_delta, g_beta, mode that ran)."""
    from beyond_dof_amd import _lib
    if f64:
        loss = eng.loss_grad(B, meas, angle_idx=angle_idx, xoff=xoff, yoff=yoff, f64=True)
        gd, gb = eng.grad_batch_to_host(B)
        return loss, None, gd, gb, None
    eng.set_sweep_fusion(mode)
    m = eng._meas_to_device(meas)
    a, xo, yo = eng._idx_bufs(angle_idx, xoff, yoff)
    out = _lib.DeviceBuffer(eng.ctx, B * eng.nx * eng.ny * 8, np.complex64, (B, eng.nx, eng.ny))
    eng.ctx.check(eng.lib.bdof_loss_grad(eng.h, B, _lib._ptr(a), _lib._ptr(xo), _lib._ptr(yo), m.ptr, out.ptr))
    loss = eng.get_loss()
    ran = eng.sweep_fused
    wave = eng._wave_to_host(out, B)
    gd, gb = eng.grad_batch_to_host(B)
    return loss, wave, gd, gb, ran


def _phi_tape(eng, B, S):
    """Tape slots 0 .. S-2 after a fused forward sweep (bdof_tape_slot): the scattered part of phi_z, [z][b][x][y]."""
    out = np.empty((S - 1, B, eng.nx, eng.ny), dtype=np.complex64)
    eng.ctx.sync()
    for z in range(S - 1):
        ptr = eng.lib.bdof_tape_slot(eng.h, z)
        assert ptr
        eng.ctx.check(eng.lib.bdof_memcpy_d2h(eng.h, out[z].ctypes.data, ptr, out[z].nbytes))
    return out


def _errors(run, twin, ref_wave):
    g = np.stack([run[2], run[3]])
    g64 = np.stack([twin[2], twin[3]])
    return abs(run[0] - twin[0]) / abs(twin[0]), rel(run[1], ref_wave), rel(g, g64)


def _check_pair(name, e_fused, e_two):
    """The factor-two rule and the parity bounds; prints the pair (MEASUREMENTS.md quotes them)."""
    print('fused sweep', name, 'errors (loss, wave, gradient): fused', tuple(float(e) for e in e_fused), ' two-kernel', tuple(float(e) for e in e_two))
    for ef, e2, tol in zip(e_fused, e_two, (LOSS_TOL, WAVE_TOL, GRAD_TOL)):
        assert e2 <= tol and ef <= tol, (name, e_fused, e_two)
    assert e_fused[1] <= FACTOR * e_two[1] and e_fused[2] <= FACTOR * e_two[2], (name, e_fused, e_two)
    assert e_fused[0] <= FACTOR * max(e_two[0], e_two[1]), (name, e_fused, e_two)


def _batch_case(engine_mod, B, Y, X, S, seed, dmax=2e-5, **kw):
    rng = np.random.default_rng(seed)
    eng, pr, pi = _engine(engine_mod, Y, X, S, B, rng, **kw)
    delta = rng.uniform(0, dmax, size=(B, Y, X, S)).astype(np.float32).astype(np.float64)
    beta = (0.1 * delta).astype(np.float32).astype(np.float64)
    eng.set_object_batch(delta, beta)
    p64 = (pr + 1j * pi).astype(np.complex64)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, p64.real.astype(np.float64), p64.imag.astype(np.float64), E_EV, PSIZE, FP,
                                                  delta.shape, return_probe_array=False)
    meas = (np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32).astype(np.float64)
    return eng, delta, beta, ref, meas, rng


def _accuracy(engine_mod, name, B, Y, X, S, seed):
    eng, delta, beta, ref, meas, rng = _batch_case(engine_mod, B, Y, X, S, seed)
    eng.enable_tf_f64()
    twin = _run(eng, B, meas, 0, f64=True)
    two = _run(eng, B, meas, 0)
    assert two[4] == 0
    for mode in MODES:
        fused = _run(eng, B, meas, mode)
        assert fused[4] == mode
        _check_pair('{} mode {}'.format(name, mode), _errors(fused, twin, ref), _errors(two, twin, ref))
    return eng, meas, two


@pytest.mark.parametrize('Y,X', [(64, 128), (128, 64), (256, 64), (64, 256)])
def test_unequal_sides_vs_twin(engine_mod, Y, X):
    """NX != NY, S = 4, 2 fields: every swapped stride, swapped table (hx / hy, twY / twX) or swapped layout shows.  64, 128 and
    256 points are the three plans below the flagship's (two stages; a radix-2 and a radix-4 middle stage)."""
    _accuracy(engine_mod, '{}x{}'.format(Y, X), 2, Y, X, 4, 5)


def test_lookup_table_64_vs_twin(engine_mod):
    """64 x 64 field, S = 6 (the volume's depth is the slice count: a 64 x 64 x 6 volume, [X][Z][Y] rows), 3 angles of a 12-angle
    table built as the solver builds it (rotation_lookup clamps the rows that leave the volume to its border).  The smallest
    streaming size: one tile per field, several rows per wave; the x-line kernel finds its table rows through the lookup, eight
    per thread."""
    from beyond_dof_amd import util, _lib
    n, S, n_theta, B = 64, 6, 12, 3
    rng = np.random.default_rng(11)
    eng, pr, pi = _engine(engine_mod, n, n, S, B, rng)
    od = rng.uniform(0, 2e-5, size=(n, n, S)).astype(np.float32)              # (Y, X, Z)
    ob = (0.1 * od).astype(np.float32)
    coords = orc.rotation_lookup([n, n, S], n_theta)
    tab, _, _ = util.device_rotation_tables(coords, n, S)
    assert any(len(np.unique(t)) < t.size for t in tab)                        # clamped border rows: some source row feeds several
    rows = util.volume_to_rows(od, ob)                                         # [X][Z][Y][2]
    vol = _lib.DeviceBuffer.from_host(eng.ctx, rows)
    tbuf = _lib.DeviceBuffer.from_host(eng.ctx, tab)
    eng.set_volume(vol, n * S, n, tbuf, n, n_theta)
    idx = [1, 5, 10]
    # the rotated batch on the host, for the float64 restatement of the detector wave
    flat = rows.reshape(n * S, n, 2).astype(np.float64)
    batch = np.stack([flat[tab[a]] for a in idx])                              # [b][z][x][y][2]
    delta, beta = util.rows_to_batch(batch)
    p64 = (pr + 1j * pi).astype(np.complex64)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, p64.real.astype(np.float64), p64.imag.astype(np.float64), E_EV, PSIZE, FP,
                                                  delta.shape, return_probe_array=False)
    meas = (np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32).astype(np.float64)
    eng.enable_tf_f64()
    twin = _run(eng, B, meas, 0, angle_idx=idx, f64=True)
    two = _run(eng, B, meas, 0, angle_idx=idx)
    assert two[4] == 0
    for mode in MODES:
        fused = _run(eng, B, meas, mode, angle_idx=idx)
        assert fused[4] == mode
        _check_pair('64^2 lookup mode {}'.format(mode), _errors(fused, twin, ref), _errors(two, twin, ref))


def test_flagship_line_length_second_tile_and_streams(engine_mod):
    """512 x 512, S = 4, 17 fields: PASSES = 2 in the transposed phase, and 17 * 512 / 16 = 544 tiles on 512 workgroup slots — some
    workgroup takes a second tile, so the barriers and the reuse of the row images between tiles are exercised.  One sub-batch
    stream and two: bit-identical."""
    B = 17
    eng, meas, two = _accuracy(engine_mod, '512^2 x 17', B, 512, 512, 4, 7)
    res = {}
    for n in (1, 2):
        eng.set_streams(n)
        assert eng.batch_groups(B) == n
        res[n] = _run(eng, B, meas, 1)
        assert res[n][4] == 1
    eng.set_streams(-1)
    assert res[1][0] == res[2][0]
    for i in (1, 2, 3):
        assert np.array_equal(res[1][i], res[2][i])


def test_adjoint_consistency_through_the_sweep(engine_mod):
    """64^2, S = 4, random object and measurements: the directional derivative of the loss along a random (delta, beta) direction,
    taken from the float64 twin (central difference of its float64 loss), against <grot, direction> of each route.  The fused
    route's relative error may be at most twice what the two-kernel route shows; both within the gradient bound.  "What the
    two-kernel route shows" is the larger of its own scalar-product error and the relative L2 error of its gradient rows against
    the twin's: a scalar product along a random direction carries the rows' relative error with a random factor of either sign
    (error and product shrink alike with the number of terms), so its own figure alone can come out near zero by chance."""
    B, n, S = 2, 64, 4
    eng, delta, beta, ref, meas, rng = _batch_case(engine_mod, B, n, n, S, 13)
    dd = rng.normal(size=delta.shape) * 2e-5
    dbt = rng.normal(size=delta.shape) * 2e-6
    eng.enable_tf_f64()
    h = 1e-3                                           # the loss is smooth at this scale: the central difference is good to h^2
    lp = lm = None
    for sgn in (+1, -1):
        eng.set_object_batch(delta + sgn * h * dd, beta + sgn * h * dbt)
        eng.enable_tf_f64()
        l = _run(eng, B, meas, 0, f64=True)[0]
        lp, lm = (l, lm) if sgn > 0 else (lp, l)
    deriv = (lp - lm) / (2 * h)
    eng.set_object_batch(delta, beta)
    eng.enable_tf_f64()
    twin = _run(eng, B, meas, 0, f64=True)
    d64 = float(np.sum(twin[2] * dd) + np.sum(twin[3] * dbt))
    # float32 object rows: the finite difference sees the rounding of delta +- h dd to float32, so the twin's own <g, d> is the
    # reference the routes are held to, and the difference quotient must agree with it to what that rounding allows
    assert abs(deriv - d64) <= 1e-3 * abs(d64), (deriv, d64)
    errs, rows = {}, {}
    g64 = np.stack([twin[2], twin[3]])
    for mode in (0,) + MODES:
        r = _run(eng, B, meas, mode)
        assert r[4] == mode
        errs[mode] = abs(float(np.sum(r[2].astype(np.float64) * dd) + np.sum(r[3].astype(np.float64) * dbt)) - d64) / abs(d64)
        rows[mode] = float(rel(np.stack([r[2], r[3]]), g64))
    print('fused sweep adjoint consistency 64^2 S=4: relative error of <grot, direction>', errs, ' of the gradient rows', rows)
    for mode in MODES:
        assert errs[0] <= GRAD_TOL and errs[mode] <= GRAD_TOL, errs
        assert errs[mode] <= FACTOR * max(errs[0], rows[0]), (errs, rows)


def test_modulation_position(engine_mod):
    """An object that is zero except for ONE voxel row at a known (x, z) of one wavefield, z odd (an x-line slice), 64^2, S = 4.
    What the one row changes — in the gradient rows of every slice, row by row, and in the detector wave — must be what it changes
    in the float64 twin.  A lookup or an r / j mix-up in the transposed phase puts the row somewhere else: a relative error of
    order one in the rows concerned, which a random object hides in a tolerance."""
    B, n, S = 2, 64, 4
    x0, z0, b0 = 21, 1, 1
    rng = np.random.default_rng(17)
    eng, pr, pi = _engine(engine_mod, n, n, S, B, rng)
    delta = np.zeros((B, n, n, S))
    delta[b0, :, x0, z0] = rng.uniform(1e-2, 2e-2, size=n).astype(np.float32)          # strong: k delta = 0.25 .. 0.5 rad in one slice
    beta = (0.1 * delta).astype(np.float32).astype(np.float64)
    meas = np.abs(1 + 0.05 * rng.normal(size=(B, n, n))).astype(np.float32).astype(np.float64)
    out, phi = {}, {}
    for name, (d, bt) in (('row', (delta, beta)), ('empty', (0 * delta, 0 * beta))):
        eng.set_object_batch(d, bt)
        eng.enable_tf_f64()
        out[name, 'twin'] = _run(eng, B, meas, 0, f64=True)
        for mode in (0,) + MODES:
            out[name, mode] = _run(eng, B, meas, mode)
            assert out[name, mode][4] == mode
            if mode:
                phi[name, mode] = _phi_tape(eng, B, S)
    # The phi tape itself, [z][b][x][y] for z <= S-2: against the empty-object run only the row (b0, x0) of slice z0 differs.  The
    # tape holds the SCATTERED part, and the object's mean factor rides on the carrier of the whole batch, so every entry up to
    # slice z0 moves by one constant per slice (its median over the slice is taken out); what remains elsewhere is rounding of
    # values below 0.1 (1e-6 is 100 of their ulps), in the row it is (c - 1) phi, 0.25 .. 0.5 of a wave of modulus one.
    for mode in MODES:
        d = phi['row', mode].astype(np.complex128) - phi['empty', mode].astype(np.complex128)
        for z in range(z0 + 1):
            dz = d[z] - (np.median(d[z].real) + 1j * np.median(d[z].imag))
            hit = np.zeros(dz.shape, dtype=bool)
            if z == z0:
                hit[b0, x0, :] = True
                assert np.abs(dz[hit]).min() >= 0.1, np.abs(dz[hit]).min()
            assert np.abs(dz[~hit]).max() <= 1e-6, (z, np.abs(dz[~hit]).max(), np.unravel_index(np.argmax(np.abs(dz) * ~hit), dz.shape))
    dt = np.stack([out['row', 'twin'][2] - out['empty', 'twin'][2], out['row', 'twin'][3] - out['empty', 'twin'][3]])     # [2][b][y][x][z]
    scale = np.sqrt((dt ** 2).sum(axis=(0, 2)))                                        # per (b, x, z) row
    assert scale[b0, x0, z0] > 0 and np.all(scale[1 - b0] == 0)                       # the other wavefield sees nothing
    for mode in MODES:
        worst = {}
        for m in (0, mode):
            dm = np.stack([out['row', m][2] - out['empty', m][2], out['row', m][3] - out['empty', m][3]]).astype(np.float64)
            err = np.sqrt(((dm - dt) ** 2).sum(axis=(0, 2)))
            # (all rows of both wavefields: the other one changes by rounding only — the object's mean factor rides on the carrier
            # of the whole batch — and is held to the same bound)
            worst[m] = float((err / scale[b0].max()).max())
        dw = out['row', mode][1] - out['empty', mode][1]
        dw0 = out['row', 0][1] - out['empty', 0][1]
        print('fused sweep modulation position: worst row error of the change in the gradient', worst, ' change of the wave', rel(dw, dw0))
        assert worst[0] <= GRAD_TOL and worst[mode] <= GRAD_TOL and worst[mode] <= FACTOR * worst[0], worst
        # four float32 waves, each within WAVE_TOL of the true one relative to ITS norm: the two changes agree to 4 WAVE_TOL of
        # the wave, not of the change (which is a few per cent of the wave — a misplaced row would be off by the whole change)
        wnorm = np.linalg.norm(out['empty', 0][1])
        assert np.linalg.norm(dw0) >= 1e-2 * wnorm
        assert np.linalg.norm(dw - dw0) <= 4 * WAVE_TOL * wnorm, (np.linalg.norm(dw - dw0), np.linalg.norm(dw0), wnorm)


def _assert_fallback(eng, B, meas, **kw):
    r1 = _run(eng, B, meas, 1, **kw)
    r0 = _run(eng, B, meas, 0, **kw)
    assert r1[4] == 0 and r0[4] == 0
    assert r1[0] == r0[0]
    for i in (1, 2, 3):
        assert np.array_equal(r1[i], r0[i])


@pytest.mark.parametrize('case', ['odd_S', 'S_2', 'binning', 'recompute', 'far_field', 'window_offsets', 'non_separable'])
def test_fallbacks_run_the_two_kernel_sweep(engine_mod, case):
    """Configurations that are not eligible: bdof_sweep_fused reports 0 and the results are bit-identical to mode 0."""
    B, n = 2, 64
    rng = np.random.default_rng(23)
    S = {'odd_S': 5, 'S_2': 2}.get(case, 4)
    kw = {'binning': dict(slice_binning=2), 'recompute': dict(recompute=True)}.get(case, {})
    eng, pr, pi = _engine(engine_mod, n, n, S, B, rng, fp='inf' if case == 'far_field' else FP, **kw)
    delta = rng.uniform(0, 2e-5, size=(B, n, n, S))
    meas = np.abs(1 + 0.05 * rng.normal(size=(B, n, n)))
    run_kw = {}
    if case == 'window_offsets':
        from beyond_dof_amd import util, _lib
        od = rng.uniform(0, 2e-5, size=(n, n, S)).astype(np.float32)
        tab, _, _ = util.device_rotation_tables(orc.rotation_lookup([n, n, S], 4), n, S)
        eng.set_volume(_lib.DeviceBuffer.from_host(eng.ctx, util.volume_to_rows(od, 0.1 * od)), n * S, n,
                       _lib.DeviceBuffer.from_host(eng.ctx, tab), n, 4)
        run_kw = dict(angle_idx=[0, 2], xoff=[0, 0], yoff=[0, 0])             # offsets given, even if zero: the windowed path
    else:
        eng.set_object_batch(delta, 0.1 * delta)
    if case == 'non_separable':
        # a transfer function made non-separable by hand: one entry of the float64 table turned by 1e-6 rad
        hs64 = eng.optics.table(eng._step_nm(), tiled=True, dtype=np.complex128).copy()
        hs64[3, 5] *= np.exp(1e-6j)
        eng.ctx.check(eng.lib.bdof_set_transfer_f64(eng.h, hs64.ctypes.data))
    _assert_fallback(eng, B, meas, **run_kw)
    if case == 'non_separable':
        # ... and the untouched table is eligible again
        hs64 = eng.optics.table(eng._step_nm(), tiled=True, dtype=np.complex128)
        eng.ctx.check(eng.lib.bdof_set_transfer_f64(eng.h, hs64.ctypes.data))
        assert _run(eng, B, meas, 1)[4] == 1


def test_dither_bookkeeping_beyond_the_copies(engine_mod):
    """S = 70 slices at 64^2, more than the 64 dithered copies of every constant: slices 64 .. 69 wrap around to copies 0 .. 5, in
    the twiddles, in sqrt(1/2), in hx / hy and in the adjoint's 2-D table alike.  A step that took another copy than its
    neighbours' bookkeeping says stays within the rule; a step that took a table of the wrong direction or slice range does not."""
    _accuracy(engine_mod, '64^2 S=70', 2, 64, 64, 70, 29)


def test_switch_and_query(engine_mod):
    from beyond_dof_amd import _lib
    rng = np.random.default_rng(31)
    eng, pr, pi = _engine(engine_mod, 64, 64, 4, 1, rng)
    assert eng.sweep_fused == 0                                   # nothing has run yet
    with pytest.raises(_lib.BdofError):
        eng.set_sweep_fusion(3)
    with pytest.raises(_lib.BdofError):
        eng.set_sweep_fusion(-1)
    delta = rng.uniform(0, 2e-5, size=(1, 64, 64, 4))
    eng.set_object_batch(delta, 0.1 * delta)
    meas = np.ones((1, 64, 64))
    eng.loss_grad(1, meas)
    assert eng.sweep_fused == 0                                   # a new ctx runs the two-kernel sweep until it is told otherwise
    assert _run(eng, 1, meas, 2)[4] == 1                          # a mode above the highest stage carried runs that stage
    assert eng.lib.bdof_tape_slot(eng.h, 3) and not eng.lib.bdof_tape_slot(eng.h, 4) and not eng.lib.bdof_tape_slot(eng.h, -1)
    assert _run(eng, 1, meas, 0)[4] == 0
    eng.forward(1)                                                # bdof_forward is not fused and leaves the record alone
    assert eng.sweep_fused == 0
