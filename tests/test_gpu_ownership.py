"""bdof_ctx owns its device buffers and rocFFT plans by type (csrc/bdof_capi.hip: DevBuf, PlanPair, FftExec, Workspace): what
bdof_configure and the setters allocate goes when it is replaced, when the context is configured again and when it is destroyed,
and a refused call leaves the context as it was.  The work runs in tests/_ownership_gpu_worker.py, a process of its own under a
time limit; the figures it prints are asserted here."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BDOF_ERR_ARG, BDOF_ERR_STATE = -1, -2


def worker(*args, timeout):
    import __graft_entry__ as entry
    entry.build()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_ownership_gpu_worker.py')] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def test_reconfigure_and_reset_do_not_accumulate_memory():
    """Three contexts one after another; each is configured twice in turn for the streaming engine with gradient, the resident
    engine, the generic engine with the float64 adjoint and the tape-free adjoint, and after every bdof_configure every setter
    that allocates is called and a small loss_grad follows it.  Every loss equals, bit for bit, the loss of the first visit of
    that configuration.  The device's memory in use, read after each bdof_ctx_destroy, must not grow from the first context to
    the last by half of the smallest configuration's workspace (450 MiB, computed from the shapes: gradient rows + tape): a
    workspace that outlives its bdof_configure or its context adds at least a whole one per context."""
    res = worker('reconfigure', 3, 2, timeout=600)
    print('losses of the first visits', res['first'])
    print('device memory in use after each bdof_ctx_destroy', res['used'], 'workspaces', res['workspace'])
    assert res['mismatches'] == []
    assert set(res['first']) == set(res['workspace'])
    bound = min(res['workspace'].values()) // 2
    assert bound >= 200 << 20                                     # far above allocator granularity
    assert res['used'][-1] - res['used'][0] < bound, (res['used'], bound)


def test_error_return_leaves_the_context_usable():
    """Calls that the library refuses for their arguments or for the context's state — bdof_configure with a zero size after a
    valid one, bdof_set_probe_stack with one of its two arrays, bdof_set_conv_probe_stack before bdof_set_conv, bdof_set_conv_f64
    with an even kernel size, bdof_loss_grad_conv_f64 under a near-field detector after bdof_set_conv_f64_detector(NULL) — return
    their code, and the valid calls that follow on the same context give the losses of a context that never saw them."""
    res = worker('errors', timeout=300)
    print(res)
    assert res['fresh']['codes'] == {}
    assert res['injected']['codes'] == {'configure_zero_size': BDOF_ERR_ARG, 'probe_stack_one_array': BDOF_ERR_ARG,
                                        'conv_probe_stack_without_conv': BDOF_ERR_STATE, 'conv_f64_even_kernel': BDOF_ERR_ARG,
                                        'conv_f64_near_without_detector': BDOF_ERR_STATE}
    fresh, injected = res['fresh']['losses'], res['injected']['losses']
    assert injected.pop('field_again') == fresh['field']
    assert injected == fresh
    assert all(v == v and v > 0 for v in fresh.values())          # real losses, not NaN
