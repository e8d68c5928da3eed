"""What the C library's setters leave behind (csrc/bdof_capi.hip: enter_setter, upload, changed), pinned on the device.

Replaced equals fresh: a context that ran under model A and is then given model B through the setters computes, bit for bit, what
a context created for model B computes — loss, gradient rows and detector wave.  Whatever a setter has to void of the state
derived from A (the float64 twin, the modulation table, the resident engine's constants, dithered copies, detector planes)
shows here as a difference.  A setter called twice with the same arguments leaves what one call leaves, and a float64 twin whose
model has been replaced refuses to run.  Smallest shapes at which the paths exist: 64 x 64 (streaming, resident by its configure
flag, the real-space propagator with 5 and 9 taps), 72 x 72 (generic engine), S = 4, B = 2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BDOF_ERR_STATE = -2
S, B = 4, 2
E, PS = 5000., 1e-7
NEAR, PLANES = 1e-4, [5e-5, 1e-4]
GEOMETRY = {'streaming': (64, 'streaming'), 'resident': (64, 'resident'), 'generic': (72, 'generic')}

# A model: what the setters are given.  det: free_prop_cm; probe: 'uniform' | 'structured' (rides on its mean) | 'gauss' (rides on
# a carrier field); host_stack: the carrier field through bdof_set_probe_stack, not bdof_set_probe_field; hs_other: another float64
# slice step through bdof_set_transfer_f64 alone; one_plane: bdof_set_detector_planes(1) after the planes; conv: taps of the
# real-space propagator; twin: the float64 twin that is handed over and run; bin: bdof_set_slice_binning calls after bdof_configure
MODEL = dict(det=NEAR, variant='numpy_skip_last', probe='uniform', host_stack=False, hs_other=False, one_plane=False, weights=False,
             conv=None, twin=None, bin=(), energy=E)


def model(**kw):
    assert set(kw) <= set(MODEL)
    return dict(MODEL, **kw)


_DATA = {}


def _data(n):
    """Object, amplitudes, probes and weights of an n x n problem, made once."""
    if n not in _DATA:
        rng = np.random.default_rng(n)
        delta = rng.uniform(0, 2e-5, size=(B, n, n, S))
        y, x = np.mgrid[:n, :n] - n / 2.0
        _DATA[n] = dict(
            delta=delta, beta=0.1 * delta, meas=1 + 0.05 * rng.normal(size=(B, 2, n, n)),
            uniform=(np.ones((n, n)), np.zeros((n, n))),
            structured=(1 + 0.05 * rng.normal(size=(n, n)), 0.05 * rng.normal(size=(n, n))),
            gauss=(np.exp(-(x * x + y * y) / (2 * (n / 8.0) ** 2)), np.zeros((n, n))),
            weights=(rng.uniform(size=(n, n)) > 0.2).astype(np.float32))
    return _DATA[n]


def _engine(geometry, m):
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd.engine import MultisliceEngine
    n, engine = GEOMETRY[geometry]
    eng = MultisliceEngine(n, n, S, B, with_grad=True, engine=engine, slice_binning=m['bin'][0] if m['bin'] else 1)
    for b in m['bin'][1:]:
        eng.ctx.check(eng.lib.bdof_set_slice_binning(eng.h, b))
        eng.slice_binning, eng.n_steps = b, S // b
    d = _data(n)
    eng.set_object_batch(d['delta'], d['beta'])
    return eng


def _apply(eng, m, prev, monkeypatch):
    """Hand model m over through the setters: everything on a fresh engine (prev None), else what differs from prev."""
    from beyond_dof_amd import util
    d = _data(eng.ny)
    new = lambda *keys: prev is None or any(m[k] != prev[k] for k in keys)
    monkeypatch.setenv('BDOF_HOST_PROBE_STACK', '1') if m['host_stack'] else monkeypatch.delenv('BDOF_HOST_PROBE_STACK', raising=False)
    if new('det', 'variant', 'energy'):
        eng.set_physics(m['energy'], PS, m['det'], variant=m['variant'])       # (re-issues the probe and the weights it holds)
    if m['hs_other'] and new('hs_other'):
        o = util.Optics(1.02 * E, PS, None, util.PI, eng.ny, eng.nx)
        hs64 = o.table(o.delta_nm, tiled=True, dtype=np.complex128)
        eng.ctx.check(eng.lib.bdof_set_transfer_f64(eng.h, hs64.ctypes.data))
    if m['one_plane'] and new('one_plane'):
        eng.ctx.check(eng.lib.bdof_set_detector_planes(eng.h, 1, None, None))
        eng.n_planes = 1
    if m['conv'] and new('conv'):
        eng.set_conv(E, PS, kernel_size=m['conv'])
    if new('probe', 'host_stack'):
        eng.set_probe(*d[m['probe']])
    if new('weights'):
        eng.set_detector_weights(d['weights'] if m['weights'] else None)
    if m['twin'] == 'tf' and (new('twin') or not eng.tf_f64):
        eng.enable_tf_f64()
    if m['twin'] == 'conv' and (new('twin') or not eng.conv_f64):
        eng.enable_conv_f64()


def _run(eng, m):
    """(loss, gradient rows as the library holds them, detector wave as the library wrote it) of one minibatch under m."""
    from beyond_dof_amd._lib import DeviceBuffer
    lib, h, n, D = eng.lib, eng.h, eng.ny, eng.n_planes
    meas = _data(n)['meas']
    dev = eng._meas_to_device(meas[:, :D] if D > 1 else meas[:, 0])
    wave = DeviceBuffer.zeros(eng.ctx, (B * D * n * n,), np.complex64)
    if m['twin']:
        fn = lib.bdof_loss_grad_conv_f64 if m['twin'] == 'conv' else lib.bdof_loss_grad_tf_f64
        eng.ctx.check(fn(h, B, None, None, None, dev.ptr, float(eng.meas_ref)))
    else:
        fn = lib.bdof_loss_grad_conv if m['conv'] else lib.bdof_loss_grad
        eng.ctx.check(fn(h, B, None, None, None, dev.ptr, wave.ptr))
    loss = eng.get_loss()
    rows = np.empty(B * S * n * n * 2, dtype=np.float32)
    eng.ctx.check(lib.bdof_memcpy_d2h(h, rows.ctypes.data, lib.bdof_grot(h), rows.nbytes))
    return loss, rows, wave.download()


_FRESH = {}


def _fresh(geometry, m, monkeypatch):
    """The result of a context created for model m — computed once per (geometry, model), shared and left unchanged."""
    key = (geometry, repr(sorted(m.items())))
    if key not in _FRESH:
        eng = _engine(geometry, m)
        _apply(eng, m, None, monkeypatch)
        _FRESH[key] = _run(eng, m)
        for a in _FRESH[key][1:]:
            a.setflags(write=False)
        assert np.isfinite(_FRESH[key][0]) and _FRESH[key][0] > 0 and np.any(_FRESH[key][1])
    return _FRESH[key]


def _assert_same(got, want, what):
    assert got[0] == want[0], (what, 'loss', got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, 'gradient rows', float(np.abs(got[1] - want[1]).max()))
    assert np.array_equal(got[2], want[2]), (what, 'wave', float(np.abs(got[2] - want[2]).max()))


CONV = dict(det=None, conv=5)
PAIRS = {
    # bdof_set_physics (with bdof_set_transfer_f64 behind it): near to far, far to none, a variant change
    'physics near -> far': ('streaming', model(), model(det='inf')),
    'physics far -> none': ('streaming', model(det='inf'), model(det=None)),
    'physics variant': ('streaming', model(), model(variant='tf_all')),
    'physics near -> far, generic': ('generic', model(), model(det='inf')),
    'physics near -> far, resident': ('resident', model(), model(det='inf')),
    'physics variant, resident': ('resident', model(), model(variant='tf_all')),
    # bdof_set_transfer_f64 alone
    'transfer_f64': ('streaming', model(), model(hs_other=True)),
    'transfer_f64, resident': ('resident', model(), model(hs_other=True)),
    'transfer_f64, generic': ('generic', model(), model(hs_other=True)),
    # bdof_set_probe
    'probe': ('streaming', model(), model(probe='structured')),
    'probe, resident': ('resident', model(), model(probe='structured')),
    'probe, generic': ('generic', model(), model(probe='structured')),
    # bdof_set_probe_stack: set, then cleared with NULL
    'probe_stack set': ('streaming', model(), model(probe='gauss', host_stack=True)),
    'probe_stack cleared': ('streaming', model(probe='gauss', host_stack=True), model()),
    'probe_stack set, resident': ('resident', model(), model(probe='gauss', host_stack=True)),
    # bdof_set_probe_field
    'probe_field set': ('streaming', model(), model(probe='gauss')),
    'probe_field cleared': ('streaming', model(probe='gauss'), model()),
    'probe_field set, far': ('streaming', model(det='inf'), model(det='inf', probe='gauss')),
    'probe_field set, generic': ('generic', model(), model(probe='gauss')),
    'probe_field set, resident': ('resident', model(), model(probe='gauss')),
    # bdof_set_detector_planes: D = 2, then 1
    'detector_planes 2': ('streaming', model(), model(det=PLANES)),
    'detector_planes 2 -> 1': ('streaming', model(det=PLANES), model(det=PLANES, one_plane=True)),
    'detector_planes 2, generic': ('generic', model(), model(det=PLANES)),
    'detector_planes 2 -> 1, generic': ('generic', model(det=PLANES), model(det=PLANES, one_plane=True)),
    # bdof_set_detector_weights: set, then NULL
    'detector_weights set': ('streaming', model(), model(weights=True)),
    'detector_weights cleared': ('streaming', model(weights=True), model()),
    'detector_weights set, resident': ('resident', model(), model(weights=True)),
    # bdof_set_conv with bdof_set_conv_taps_f64: 5 taps, then 9
    'conv 5 -> 9': ('streaming', model(**CONV), model(det=None, conv=9)),
    'conv 5 -> 9, near': ('streaming', model(conv=5), model(conv=9)),
    'conv 5 -> 9, far': ('streaming', model(det='inf', conv=5), model(det='inf', conv=9)),
    'conv after the transfer-function path': ('streaming', model(det=None), model(**CONV)),
    # bdof_set_conv_probe_stack: set, then cleared
    'conv_probe_stack set': ('streaming', model(**CONV), model(probe='gauss', **CONV)),
    'conv_probe_stack cleared': ('streaming', model(probe='gauss', **CONV), model(**CONV)),
    'conv_probe_stack set, near': ('streaming', model(conv=5), model(conv=5, probe='gauss')),
    # bdof_set_tf_f64, then bdof_set_conv_f64, on one context — and back
    'tf_f64 -> conv_f64': ('streaming', model(twin='tf', **CONV), model(twin='conv', **CONV)),
    'conv_f64 -> tf_f64': ('streaming', model(twin='conv', **CONV), model(twin='tf', **CONV)),
    'tf_f64 after float32': ('streaming', model(), model(twin='tf')),
    'tf_f64 after another probe': ('streaming', model(twin='tf'), model(twin='tf', probe='structured')),
}


@pytest.mark.parametrize('pair', sorted(PAIRS))
def test_replaced_equals_fresh(pair, monkeypatch):
    geometry, a, b = PAIRS[pair]
    eng = _engine(geometry, a)
    _apply(eng, a, None, monkeypatch)
    _assert_same(_run(eng, a), _fresh(geometry, a, monkeypatch), 'model A')
    _apply(eng, b, a, monkeypatch)
    _assert_same(_run(eng, b), _fresh(geometry, b, monkeypatch), 'model B after model A')


def test_slice_binning_two_then_one_is_no_binning(monkeypatch):
    """bdof_set_slice_binning comes right after bdof_configure, so there is no run between: 2, then 1, is a ctx that never binned;
    1, then 2, is one that was configured for 2."""
    for geometry in ('streaming', 'generic'):
        _assert_same(_fresh(geometry, model(bin=(2, 1)), monkeypatch), _fresh(geometry, model(), monkeypatch), geometry)
        _assert_same(_fresh(geometry, model(bin=(1, 2)), monkeypatch), _fresh(geometry, model(bin=(2,)), monkeypatch), geometry)


class _Twice(object):
    """The library with every setter issued twice (the second call's return code is the one passed on)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not (name.startswith('bdof_set_') or name == 'bdof_enable_probe_grad'):
            return fn

        def twice(*args):
            first = fn(*args)
            return first if first != 0 else fn(*args)
        return twice


TWICE = {
    'streaming near': ('streaming', model()), 'streaming far, tf_all': ('streaming', model(det='inf', variant='tf_all')),
    'generic near': ('generic', model()), 'resident near': ('resident', model()), 'resident far': ('resident', model(det='inf')),
    'structured probe': ('streaming', model(probe='structured')), 'probe_stack': ('streaming', model(probe='gauss', host_stack=True)),
    'probe_field': ('streaming', model(probe='gauss')), 'probe_field, generic': ('generic', model(probe='gauss')),
    'transfer_f64': ('streaming', model(hs_other=True)), 'planes': ('streaming', model(det=PLANES)),
    'planes -> 1': ('streaming', model(det=PLANES, one_plane=True)), 'weights': ('streaming', model(weights=True)),
    'binning': ('streaming', model(bin=(2,))), 'conv 5': ('streaming', model(**CONV)), 'conv 9, near': ('streaming', model(conv=9)),
    'conv_probe_stack': ('streaming', model(probe='gauss', **CONV)), 'tf_f64': ('streaming', model(twin='tf')),
    'conv_f64': ('streaming', model(twin='conv', **CONV)),
}


@pytest.mark.parametrize('case', sorted(TWICE))
def test_setter_twice_is_setter_once(case, monkeypatch):
    from beyond_dof_amd import _lib
    geometry, m = TWICE[case]
    want = _fresh(geometry, m, monkeypatch)
    monkeypatch.setattr(_lib, '_lib', _Twice(_lib.load()))
    eng = _engine(geometry, m)
    assert isinstance(eng.lib, _Twice)
    _apply(eng, m, None, monkeypatch)
    _assert_same(_run(eng, m), want, case)


def _voiders(eng):
    """(setter, a well-formed call of it) for the three setters that replace what a float64 twin was handed."""
    n, lib, h = eng.ny, eng.lib, eng.h
    hs = np.full((n, n), 1.0 / (n * n), dtype=np.complex64)
    h00 = np.array([1.0, 0.0])
    probe = np.zeros((n, n), dtype=np.complex64)
    taps = np.zeros(5, dtype=np.complex64)
    taps[2] = 1
    return [('bdof_set_physics', lambda: lib.bdof_set_physics(h, 0.025, hs.ctypes.data, None, h00.ctypes.data, None, 0, 0)),
            ('bdof_set_probe', lambda: lib.bdof_set_probe(h, probe.ctypes.data, 1.0, 0.0)),
            ('bdof_set_conv', lambda: lib.bdof_set_conv(h, taps.ctypes.data, taps.ctypes.data, 5, 1.0, 0.0, 1.0, 0.0, 0.025))]


@pytest.mark.parametrize('twin', ['tf', 'conv'])
def test_stale_twin_refuses(twin, monkeypatch):
    m = model(twin=twin, **CONV)
    eng = _engine('streaming', m)
    _apply(eng, m, None, monkeypatch)
    run = eng.lib.bdof_loss_grad_tf_f64 if twin == 'tf' else eng.lib.bdof_loss_grad_conv_f64
    text = 'bdof_set_tf_f64 has not been called' if twin == 'tf' else 'bdof_set_conv_f64 has not been called'
    dev = eng._meas_to_device(_data(eng.ny)['meas'][:, 0])
    for name, call in _voiders(eng):
        assert run(eng.h, B, None, None, None, dev.ptr, 0.0) == 0, name
        assert call() == 0, name
        assert run(eng.h, B, None, None, None, dev.ptr, 0.0) == BDOF_ERR_STATE, name
        assert eng.lib.bdof_last_error(eng.h).decode() == text, name
        eng.enable_tf_f64() if twin == 'tf' else eng.enable_conv_f64()      # handed over again: it runs
    assert run(eng.h, B, None, None, None, dev.ptr, 0.0) == 0
