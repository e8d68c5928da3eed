"""The model's options against the path of a call (beyond_dof_amd/engine.py: OPTION_NEEDS, check_model_options), off the GPU.

The texts below were recorded from the four functions check_model_options replaced (check_poisson_path, check_weights_path,
check_binning_path, check_planes_path) and from MultisliceEngine's own refusals (its constructor; _need_unbinned /
_need_one_plane in front of set_conv, enable_tf_f64, enable_conv_f64, forward(conv=True), loss_grad(conv=True / f64=True)), each
over the whole grid of its keywords: itertools.product over a grid's values, in the order written, one character per case,
the index of its text in MESSAGES (0: no ValueError)."""
import itertools
import string
import types

import pytest

from beyond_dof_amd import engine as eng

MESSAGES = [
    None,
    'poisson_multiplier must be > 0',
    "loss_type='poisson' runs on the transfer-function propagator (propagator='fft') only",
    "loss_type must be 'lsq' or 'poisson'",
    "detector_weights run on the transfer-function propagator (propagator='fft') only",
    "slice_binning > 1 runs on the rotation tables (rotation='nearest') only",
    "slice_binning > 1 has no float64 twin: adjoint_precision must be 'float32'",
    "slice_binning > 1 runs on the transfer-function propagator (propagator='fft') only",
    'slice_binning must be an integer >= 1',
    "several detector planes share one detector_kernel, 'TF' or 'IR': not 'auto'",
    "several detector planes have no float64 twin: adjoint_precision must be 'float32' (no adjoint64)",
    'several detector planes run with the tape: not recompute',
    "several detector planes run on the rotation tables (rotation='nearest') only",
    "several detector planes (free_prop_cm as a sequence) run on the transfer-function propagator (propagator='fft') only",
    'free_prop_cm as a sequence of detector planes takes finite distances > 0 in cm, not None',
    "slice_binning > 1 runs on the streaming and generic engines with the tape: not engine='resident', recompute, adjoint64 or no_grot",
    'the real-space propagator (set_conv) does not carry several detector planes',
    'the float64 twin (enable_tf_f64) does not carry several detector planes',
    'the real-space propagator (forward(conv=True)) does not carry several detector planes',
    'the real-space propagator / the float64 twin (loss_grad(conv=True / f64=True)) does not carry several detector planes',
    'the real-space propagator (set_conv) does not carry slice_binning > 1',
    'the float64 twin (enable_tf_f64) does not carry slice_binning > 1',
    'the float64 twin (enable_conv_f64) does not carry slice_binning > 1',
]
TWO = [5e-5, 1e-4]
METHODS = (eng._SET_CONV, eng._TF_F64, eng._CONV_F64, eng._FORWARD_CONV, eng._LOSS_GRAD_OFF)
GRIDS = {
    'poisson': dict(loss_type=('lsq', 'poisson', 'bogus'), poisson_multiplier=(2e6, 0), propagator=('fft', 'conv', 'anything-else')),
    'weights': dict(detector_weights=(None, 'exchange/weights'), propagator=('fft', 'conv', 'anything-else')),
    'binning': dict(slice_binning=(1, 2, 0, 1.5), propagator=('fft', 'conv'), adjoint_precision=(None, 'float32', 'float64', 'first-step'),
                    rotation=('nearest', 'bilinear')),
    'planes': dict(free_prop_cm=([1e-4], TWO, [1e-4, None]), propagator=('fft', 'conv'), adjoint_precision=(None, 'float32', 'float64'),
                   rotation=('nearest', 'bilinear'), recompute=(False, True), adjoint64=(False, True), detector_kernel=('TF', 'IR', 'auto')),
    # MultisliceEngine(16, 16, 4, 1, **case)
    'engine': dict(slice_binning=(1, 2), engine=('auto', 'resident'), recompute=(False, True), adjoint64=(False, True), no_grot=(False, True)),
    # an engine with these two attributes, in front of the method
    'method': dict(slice_binning=(1, 2), n_planes=(1, 2), method=METHODS),
}
EXPECTED = {
    'poisson': '000111022111333333',
    'weights': '000044',
    'binning': '0000000000000000050566667777777788888888888888888888888888888888',
    'planes': (
        '000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000'
        '000000000000000000000000000000000000009aaabbbaaacccaaabbbaaa009aaabbbaaacccaaabbbaaaaaaaaaaaaaaaaaaaaaaaaaaa'
        'ddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeee'
        'eeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeeee'
    ),
    'engine': '00000000000000000fffffffffffffff',
    'method': '00000gh0ijklm00klmij',
}
ALPHABET = string.digits + string.ascii_lowercase


def _raised(call, *args, **kw):
    try:
        call(*args, **kw)
    except ValueError as e:
        return str(e)
    return None


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_every_recorded_refusal_is_reproduced(name):
    grid = GRIDS[name]
    cases = [dict(zip(grid, values)) for values in itertools.product(*grid.values())]
    assert len(cases) == len(EXPECTED[name])
    for case, code in zip(cases, EXPECTED[name]):
        if name == 'method':
            fake = types.SimpleNamespace(slice_binning=case['slice_binning'], n_planes=case['n_planes'])
            got = _raised(eng.MultisliceEngine._admit, fake, case['method'])
        else:
            got = _raised(eng.check_model_options, **case)
        assert got == MESSAGES[ALPHABET.index(code)], (case, got)


def test_the_engine_constructor_asks_the_table(monkeypatch):
    """MultisliceEngine hands its four path keywords and the binning over; nothing of the device is touched before that."""
    seen = []

    def asked(**kw):
        seen.append(kw)
        raise ValueError('asked')

    monkeypatch.setattr(eng, 'check_model_options', asked)
    with pytest.raises(ValueError, match='asked'):
        eng.MultisliceEngine(16, 16, 4, 1, engine='resident', recompute=True, adjoint64=True, no_grot=True, slice_binning=2)
    assert seen == [dict(slice_binning=2, engine='resident', recompute=True, adjoint64=True, no_grot=True)]


# ---- the table itself ----------------------------------------------------------------------------------------------------------
ON = {'poisson': dict(loss_type='poisson'), 'weights': dict(detector_weights='exchange/weights'), 'binning': dict(slice_binning=2),
      'planes': dict(free_prop_cm=TWO)}
# every value a keyword of the path takes in this package, and one it does not
VALUES = dict(propagator=('fft', 'conv', 'anything-else'), adjoint_precision=(None, 'float32', 'float64', 'first-step'),
              rotation=('nearest', 'bilinear'), engine=('auto', 'generic', 'streaming', 'resident'), recompute=(False, True),
              adjoint64=(False, True), no_grot=(False, True), detector_kernel=('TF', 'IR', 'auto'), method=(None,) + METHODS)


def test_the_table_is_what_is_refused():
    """For every option and every value of every keyword of the path, the rest of the path as PATH has it: a ValueError if and only
    if a row of the option's says so, with that row's text; without the option nothing is refused; and no row is dead — each
    is the one that speaks for at least one value."""
    assert set(eng.OPTION_NEEDS) == set(ON) and set(VALUES) == set(eng.PATH)
    assert all(PATH_value in VALUES[key] for key, PATH_value in eng.PATH.items())
    assert _raised(eng.check_model_options) is None
    for option, rows in eng.OPTION_NEEDS.items():
        spoke = set()
        assert all(key in eng.PATH and carries(eng.PATH[key]) for key, carries, _ in rows), option
        for key, values in VALUES.items():
            for value in values:
                want = None
                for i, (row_key, carries, text) in enumerate(rows):
                    if row_key == key and not carries(value):
                        want = text.format(value)
                        spoke.add(i)
                        break
                assert _raised(eng.check_model_options, **dict(ON[option], **{key: value})) == want, (option, key, value)
                assert _raised(eng.check_model_options, **{key: value}) is None, (key, value)
        assert spoke == set(range(len(rows))), (option, sorted(set(range(len(rows))) - spoke))


def test_a_keyword_that_is_not_of_the_path_is_an_error():
    with pytest.raises(TypeError, match='not of the path'):
        eng.check_model_options(slice_binning=2, propagater='fft')
