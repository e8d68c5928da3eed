"""tests/adam_reference.py on the host: its float64 restatements against the oracle and the golden vectors G4 and G5; its float32
restatement of the kernels' arithmetic through every case of tests/test_gpu_update_tail.py (inside every bound, the exact cases
exact); and the same comparisons on copies of that restatement with one error planted each, which must fail."""
import functools
import os

import numpy as np
import pytest

from oracle import bdof_oracle as orc

import adam_reference as ar

PLANTS = ['wrap', 'swap_xz', 'sgn_beta', 'slab_late', 'mask_transposed']


def _to_volume(rows):
    """[X][Z][Y] -> the oracle's (Y, X, Z)"""
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float64).transpose(2, 0, 1))


@pytest.mark.parametrize('gamma', [1e-9, 0.])
@pytest.mark.parametrize('clip', [1, 0])
def test_float64_restatement_is_the_oracle(gamma, clip):
    """regularizer_grad + apply_gradient_adam + mask + clip of the oracle, two steps, whole volume and one slab"""
    rng = np.random.default_rng(21)
    shape = (5, 3, 7)
    x = rng.uniform(-1e-6, 2e-6, size=shape + (2,))
    x[rng.uniform(size=x.shape) < 0.15] = 0
    mask = rng.choice([0., 1., 0.5], size=shape)
    kw = dict(alpha_d=1.5e-8, alpha_b=1.5e-9, gamma=gamma)
    m, v = np.zeros_like(x), np.zeros_like(x)
    for it in range(2):
        g = 1e-8 * rng.normal(size=x.shape)
        ref = ar.adam_step_reference(x, g, m, v, mask, ar.sentinels(shape), g_scale=0.5, lr=1e-7, b1=0.9, b2=0.999, eps=1e-8, i_batch=it, clip=clip, **kw)
        rd, rb = orc.regularizer_grad(_to_volume(x[..., 0]), _to_volume(x[..., 1]), **kw)
        xo = np.array([_to_volume(x[..., 0]), _to_volume(x[..., 1])])
        go = np.array([0.5 * _to_volume(g[..., 0]) + rd, 0.5 * _to_volume(g[..., 1]) + rb])
        xr, mr, vr = orc.apply_gradient_adam(xo, go, it, np.array([_to_volume(m[..., c]) for c in (0, 1)]),
                                             np.array([_to_volume(v[..., c]) for c in (0, 1)]), step_size=1e-7)
        xr = xr * _to_volume(mask)
        if clip:
            xr = np.clip(xr, 0, None)
        for c in (0, 1):
            np.testing.assert_allclose(_to_volume(ref.x_new[..., c]), xr[c], rtol=1e-13, atol=0)
            np.testing.assert_allclose(_to_volume(ref.m[..., c]), mr[c], rtol=1e-13, atol=0)
            np.testing.assert_allclose(_to_volume(ref.v[..., c]), vr[c], rtol=1e-13, atol=0)
        assert clip or np.any(ref.x_new < 0)
        slab = ar.adam_step_reference(x, g, m, v, mask, ar.sentinels(shape), g_scale=0.5, lr=1e-7, b1=0.9, b2=0.999, eps=1e-8, i_batch=it, clip=clip,
                                      x0=1, nx=2, **kw)
        assert np.array_equal(slab.x_new[1:3], ref.x_new[1:3]) and np.array_equal(slab.m[1:3], ref.m[1:3]) and np.array_equal(slab.v[1:3], ref.v[1:3])
        assert np.all(slab.x_new[[0, 3, 4]] == ar.SENTINEL) and np.array_equal(slab.m[[0, 3, 4]], m[[0, 3, 4]]) and np.array_equal(slab.v[[0, 3, 4]], v[[0, 3, 4]])
        assert not np.any(slab.bx[[0, 3, 4]]) and np.array_equal(slab.bx[1:3], ref.bx[1:3])
        x, m, v = ref.x_new, ref.m, ref.v
    sums, _ = ar.reg_value_reference(x)
    want = orc.regularizer(_to_volume(x[..., 0]), _to_volume(x[..., 1]), **kw)
    assert abs(kw['alpha_d'] * sums[0] + kw['alpha_b'] * sums[1] + gamma * sums[2] - want) <= 1e-13 * abs(want)
    assert abs(sums[2] - orc.total_variation_3d(_to_volume(x[..., 0]))) <= 1e-13 * sums[2]


def test_float64_restatement_reproduces_g4_and_g5(golden_dir):
    g4 = np.load(os.path.join(golden_dir, 'g4_adam.npz'))
    rows = lambda a: np.stack([a[0], a[1]], axis=-1).transpose(1, 2, 0, 3)          # (2, Y, X, Z) -> [X][Z][Y][2]
    x = rows(g4['x0'])
    m, v = np.zeros_like(x), np.zeros_like(x)
    for it in range(3):
        ref = ar.adam_step_reference(x, rows(g4['g{}'.format(it)]), m, v, None, np.zeros_like(x), g_scale=1., alpha_d=0., alpha_b=0., gamma=0.,
                                     lr=1e-7, b1=0.9, b2=0.999, eps=1e-8, i_batch=it, clip=0)
        x, m, v = ref.x_new, ref.m, ref.v
        for got, name in ((x, 'x'), (m, 'm'), (v, 'v')):
            np.testing.assert_allclose(got, rows(g4['{}{}'.format(name, it + 1)]), rtol=1e-13, atol=0)
    g5 = np.load(os.path.join(golden_dir, 'g5_tv.npz'))
    sums, _ = ar.reg_value_reference(np.stack([g5['arr'], np.zeros_like(g5['arr'])], axis=-1))
    np.testing.assert_allclose(sums[2], g5['tv'], rtol=1e-14)


def _step(plant=None):
    return functools.partial(ar.adam_step_float32, plant=plant)


def test_float32_restatement_passes_every_case():
    """exact cases exact, every bounded element inside its bound (and every bound under its cap)"""
    worst = 0.
    for shape in ar.EXACT_SHAPES:
        for variant in ar.EXACT_VARIANTS:
            worst = max(worst, ar.run_exact(_step(), shape, variant)['x'])
    for shape in ar.SHAPES_3:
        worst = max(worst, ar.run_slabs(_step(), shape))
    worst = max(worst, ar.run_strided(_step(), 256))
    print('exact cases: largest x_new error / bound of the float32 restatement', worst)
    for case in ar.BOUNDED_CASES:
        r = ar.run_bounded(_step(), case)
        print('bounded case', case, ': largest error / bound of the float32 restatement', r)
        worst = max(worst, *r.values())
    print('all Adam cases: largest error / bound', worst)
    for shape in ar.EXACT_SHAPES + [ar.STRIDED_SHAPE]:
        ar.run_reg(ar.reg_value_float32, shape)
    print('regulariser value, production magnitudes: error / bound', ar.run_reg(ar.reg_value_float32, ar.BOUNDED_SHAPE, production=True))
    for n in ar.SHRINK_NS + (int(np.prod(ar.STRIDED_SHAPE)),):
        for thresh in ar.SHRINK_THRESHOLDS:
            ar.run_shrink(ar.mask_shrink_float32, n, thresh)


@pytest.mark.parametrize('plant', PLANTS)
def test_planted_error_fails_the_comparisons(plant):
    """on both three-extent shapes in the exact cases, and in every bounded case whose data the error touches"""
    for shape in ar.SHAPES_3:
        with pytest.raises(AssertionError):
            ar.run_exact(_step(plant), shape, 'tv_mask_clip')
        with pytest.raises(AssertionError):
            ar.run_slabs(_step(plant), shape)
    # A wrong stencil sign moves gd by gamma, sgn(beta) from delta moves it by alpha_b; the bound on gd is about 4 u sigma.  A bounded
    # case must see the error where it moves gd by more than ten times that (the exact cases see it at any size).
    moves = lambda c: {'wrap': c['gamma'], 'swap_xz': c['gamma'], 'sgn_beta': ar.PRODUCTION['alpha_b']}.get(plant, np.inf)
    bounded = [n for n, c in ar.BOUNDED_CASES.items() if (c['mask'] or plant != 'mask_transposed') and moves(c) > 10 * 4 * ar.U * c['sigma']]
    assert len(bounded) >= 3
    for case in bounded:
        with pytest.raises(AssertionError):
            ar.run_bounded(_step(plant), case)


def test_planted_slab_error_fails_where_only_the_slab_is_wrong():
    """a slab that starts one plane late passes a whole call's inside only if the first plane is compared too: the single plane
    x0 = 0 comes back untouched"""
    shape = ar.SHAPES_3[0]
    x_old, g, m0, v0, mask = ar.exact_data(shape, 2)
    got = ar.adam_step_float32(x_old, g, m0, v0, mask, ar.sentinels(shape), x0=0, nx=1, plant='slab_late', **ar.EXACT)
    assert np.all(got[0] == ar.SENTINEL)
    ref = ar.adam_step_reference(x_old, g, m0, v0, mask, ar.sentinels(shape), x0=0, nx=1, **ar.EXACT)
    with pytest.raises(AssertionError):
        ar.check_adam('single plane', got, ref, True)


@pytest.mark.parametrize('thresh', ar.SHRINK_THRESHOLDS)
@pytest.mark.parametrize('n', ar.SHRINK_NS)
def test_planted_shrink_on_beta_fails(n, thresh):
    with pytest.raises(AssertionError):
        ar.run_shrink(functools.partial(ar.mask_shrink_float32, plant='shrink_beta'), n, thresh)
