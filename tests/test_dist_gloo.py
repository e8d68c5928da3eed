"""Multi-rank path on CPU: 2 processes.  (a) gloo:  Each rank produces the gradient of ITS angles (here with the
oracle, the GPU is not needed to test the exchange), the volume gradient is SUM-all-reduced through
beyond_dof_amd.comm.TorchComm and divided by size exactly as the solver does; the result must equal the
single-rank gradient of the union minibatch (cnn_propagator/fullfield.py:343-351)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import bdof_oracle as orc


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _problem():
    rng = np.random.default_rng(0)
    n, n_theta, mb = 8, 6, 2
    od = rng.uniform(0, 1e-3, size=(n, n, n))
    ob = 0.1 * od
    coords = orc.rotation_lookup([n, n, n], n_theta)
    prj = 1 + 0.05 * rng.normal(size=(n_theta, n, n))
    return n, n_theta, mb, od, ob, coords, prj


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from beyond_dof_amd.comm import TorchComm, minibatch_schedule
    comm = TorchComm('gloo')
    assert comm.size == world and comm.rank == rank
    n, n_theta, mb, od, ob, coords, prj = _problem()
    sched = minibatch_schedule(n_theta, world, mb, rng=np.random.RandomState(5))
    chunk = sched[0]
    mine = chunk[rank * mb:(rank + 1) * mb]
    one, zero = np.ones((n, n)), np.zeros((n, n))
    _, gd, gb = orc.fullfield_loss_and_grad(od, ob, coords, mine, prj[mine], one, zero, 5000., 1e-7, free_prop_cm=1e-4,
                                            with_reg=False)
    g = torch.from_numpy(np.stack([gd, gb]))
    comm.allreduce_sum_device(None, g)
    g = g.numpy() / comm.size
    # the collectives of the solver's sharded tail on a slab [lo, lo + size*per): reduce-scatter leaves this rank's part
    # summed, the all-gather hands every rank's part to all — together they equal the all-reduce
    src = torch.from_numpy(np.stack([gd, gb])).reshape(-1)
    g2 = src.clone()
    lo, per = 96, 200
    assert comm.start_reduce_scatter(None, g2, lo, per) is None
    mine_lo = lo + rank * per
    assert np.array_equal(g2[mine_lo:mine_lo + per].numpy() / comm.size, g.reshape(-1)[mine_lo:mine_lo + per])
    g3 = torch.full_like(src, -7.0)
    g3[mine_lo:mine_lo + per] = g2[mine_lo:mine_lo + per]
    comm.start_allgather(None, g3, lo, per)
    comm.wait(None, None)
    assert np.array_equal(g3[lo:lo + world * per].numpy() / comm.size, g.reshape(-1)[lo:lo + world * per])
    assert float(g3[0]) == -7.0 and float(g3[lo + world * per]) == -7.0          # nothing outside the slab is touched
    loss_sum = comm.allreduce_sum_host(np.array([float(rank + 1)]))
    idx = comm.bcast_host(np.arange(4) if rank == 0 else np.zeros(4, dtype=np.int64), root=0)
    comm.Barrier()
    np.savez(os.path.join(out_dir, 'rank{}.npz'.format(rank)), g=g, chunk=chunk, loss_sum=loss_sum, idx=idx)
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_gradient_allreduce_equals_union(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    n, n_theta, mb, od, ob, coords, prj = _problem()
    r0 = np.load(str(tmp_path / 'rank0.npz'))
    r1 = np.load(str(tmp_path / 'rank1.npz'))
    assert np.array_equal(r0['chunk'], r1['chunk'])              # every rank derives the same schedule
    assert np.array_equal(r0['g'], r1['g'])                      # and holds the same reduced gradient
    assert r0['loss_sum'][0] == 3.0 and np.array_equal(r1['idx'], np.arange(4))
    chunk = r0['chunk']
    assert len(chunk) == world * mb and len(set(chunk.tolist())) == world * mb
    one, zero = np.ones((n, n)), np.zeros((n, n))
    _, gd, gb = orc.fullfield_loss_and_grad(od, ob, coords, chunk, prj[chunk], one, zero, 5000., 1e-7, free_prop_cm=1e-4,
                                            with_reg=False)
    np.testing.assert_allclose(r0['g'][0], gd, rtol=0, atol=1e-12 * np.abs(gd).max())
    np.testing.assert_allclose(r0['g'][1], gb, rtol=0, atol=1e-12 * np.abs(gb).max())


def test_single_rank_fallback():
    from beyond_dof_amd.comm import PseudoComm, get_comm
    os.environ.pop('WORLD_SIZE', None)
    c = get_comm()
    assert isinstance(c, PseudoComm) and c.size == 1 and c.rank == 0
    c.Barrier()
    x = np.arange(3.0)
    assert c.allreduce_sum_host(x) is x


# ---- control plane of the native (RCCL) path: unix-socket rendezvous + host collectives, no GPU needed ----------------
def _socket_worker(rank, world, path, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), BDOF_RDZV=path)
    from beyond_dof_amd.comm import RcclComm, get_comm
    comm = get_comm()
    assert isinstance(comm, RcclComm) and comm.size == world and comm.rank == rank and comm.backend == 'rccl'
    tot = comm.allreduce_sum_host(np.array([rank + 1.0, 10.0 * (rank + 1)]))
    mx = comm.allreduce_max_host(np.array([float(rank), -float(rank)]))
    big = comm.bcast_host(np.arange(300000, dtype=np.float64) if rank == 0 else None, root=0)      # > one socket buffer
    uid = comm.group.bcast(b'x' * 128 if rank == 0 else None)
    where = comm.group.allgather(('host', rank))
    comm.Barrier()
    np.savez(os.path.join(out_dir, 'sock{}.npz'.format(rank)), tot=tot, mx=mx, big_sum=big.sum(), uid_len=len(uid),
             where=np.array([w[1] for w in where]))
    comm.close()


@pytest.mark.timeout(120)
def test_socket_rendezvous_and_host_collectives(tmp_path):
    from beyond_dof_amd.comm import rendezvous_dir
    world = 3
    # the socket goes where the library puts its own: a unix socket address holds ~107 bytes, which pytest's tmp_path
    # (base directory, user name, test name) can exceed
    path = os.path.join(rendezvous_dir(), 'test_rdzv_{}.sock'.format(os.getpid()))
    open(path, 'w').close()                       # a stale file of a dead job must not be in the way
    try:
        mp.spawn(_socket_worker, args=(world, path, str(tmp_path)), nprocs=world, join=True)
    except BaseException:
        if os.path.exists(path):
            os.unlink(path)
        raise
    for r in range(world):
        d = np.load(str(tmp_path / 'sock{}.npz'.format(r)))
        assert np.array_equal(d['tot'], [6.0, 60.0]) and np.array_equal(d['mx'], [2.0, 0.0])
        assert d['big_sum'] == 300000 * 299999 / 2 and d['uid_len'] == 128 and np.array_equal(d['where'], [0, 1, 2])
    assert not os.path.exists(path)               # rank 0 removes the socket file once everyone is connected


def test_solver_tail_plan_without_a_gpu():
    """Which form of the exchange a volume of dim_x planes takes (solver._VolumeSolver.tail_plan): pure host logic."""
    from beyond_dof_amd.solver import _VolumeSolver

    class C(object):
        size, rank, sharded = 8, 0, True

    s = _VolumeSolver.__new__(_VolumeSolver)
    s.comm, s._plan = C(), None
    for dim_x, want in ((512, (8, True)), (64, (8, True)), (72, (3, True)), (48, (6, True)), (8, (1, True)), (20, (8, False)), (7, (7, False))):
        s.dim_x = dim_x
        got = s.tail_plan()
        if want[1]:
            assert got == want, (dim_x, got)
            assert dim_x % (got[0] * 8) == 0
        else:
            assert got[1] is False
    s.dim_x = 512
    assert s.tail_plan(n_slabs=3, sharded=False) == (3, False)
    assert sum(nx for _, nx in s.slab_bounds(3)) == 512


def _recorded_tail(size, rank, one_pass=False, **plan):
    """The tail of a step (solver._VolumeSolver._tail) on an object without a device, 16 x-planes of 3 x 5 voxels (30 floats per
    plane): what it asks of the communicator, the engine's Adam, the producer of the gradient and the rotation, in order."""
    from beyond_dof_amd.solver import _VolumeSolver, Update
    events = []

    class Comm(object):
        sharded, always_reduce = True, False

        def _start(self, kind, buf, lo, n):
            events.append(('start', kind, buf, lo, n))
            return '{}{}'.format(kind, sum(e[:2] == ('start', kind) for e in events) - 1)      # the ticket: 'rs0', 'rs1', ...

        def start_allreduce(self, ctx, buf, lo, hi):
            return self._start('ar', buf, lo, hi)

        def start_reduce_scatter(self, ctx, buf, lo, per):
            return self._start('rs', buf, lo, per)

        def start_allgather(self, ctx, buf, lo, per):
            return self._start('ag', buf, lo, per)

        def wait(self, ctx, ticket):
            events.append(('wait', ticket))

    class Engine(object):
        def adam_step(self, x_old, x_new, g, m, v, mask, shape_xzy, i_batch, lr, g_scale=1.0, alpha_d=0.0, alpha_b=0.0, gamma=0.0, clip=True, slab=None):
            assert (x_old, x_new, g, m, v, mask, shape_xzy) == ('x0', 'x1', 'g', 'm', 'v', 'mask', (16, 3, 5))
            assert (i_batch, lr, alpha_d, alpha_b, gamma, clip) == (7, 0.25, 1e-3, 2e-3, 3e-3, False)
            events.append(('adam', slab, g_scale))

    class Rotation(object):
        def bind_volume(self, eng, x):
            events.append(('bind', x))

    s = _VolumeSolver.__new__(_VolumeSolver)
    s.comm, s.ctx, s.eng, s.rot = Comm(), object(), Engine(), Rotation()
    s.comm.size, s.comm.rank = size, rank
    s.dim_x, s.dim_z, s.dim_y = 16, 3, 5
    s.x, s.cur, s.g, s.m, s.v, s.mask = ['x0', 'x1'], 0, 'g', 'm', 'v', 'mask'
    s._plan = s._epoch_plan = s._g_shards = None
    assert s.lookahead == 2 and not s.time_tail
    update = Update(7, 0.25, alpha_d=1e-3, alpha_b=2e-3, gamma=3e-3, clip=False, use_mask=True)
    if one_pass:
        plan['one_pass'] = lambda u, g_scale: events.append(('one_pass', tuple(u), g_scale))
    s._tail(lambda x0, nx: events.append(('produce', x0, nx)), update, **plan)
    assert s.cur == 1
    return events, s


def test_the_tail_keeps_its_schedule():
    """The order of launches, collectives and waits of the tail, written out by hand: a collective is started right behind the
    producer of its slab and awaited two slabs later (lookahead), Adam follows the wait, the sharded form's all-gathers are awaited
    at the end, the new volume is bound last."""
    # sharded: reduce-scatter of this rank's half of each 4-plane slab (60 floats per rank), Adam on rank 1's two planes of it
    events, s = _recorded_tail(2, 1, n_slabs=4, sharded=True)
    assert events == [
        ('produce', 0, 4), ('start', 'rs', 'g', 0, 60),
        ('produce', 4, 4), ('start', 'rs', 'g', 120, 60),
        ('produce', 8, 4), ('start', 'rs', 'g', 240, 60), ('wait', 'rs0'), ('adam', (2, 2), 0.5), ('start', 'ag', 'x1', 0, 60),
        ('produce', 12, 4), ('start', 'rs', 'g', 360, 60), ('wait', 'rs1'), ('adam', (6, 2), 0.5), ('start', 'ag', 'x1', 120, 60),
        ('wait', 'rs2'), ('adam', (10, 2), 0.5), ('start', 'ag', 'x1', 240, 60),
        ('wait', 'rs3'), ('adam', (14, 2), 0.5), ('start', 'ag', 'x1', 360, 60),
        ('wait', 'ag0'), ('wait', 'ag1'), ('wait', 'ag2'), ('wait', 'ag3'),
        ('bind', 'x1')]
    assert s._g_shards == [(0, 4), (4, 4), (8, 4), (12, 4)] and s._epoch_plan == ('taken', (4, True))
    # all-reduce: floats [lo, hi) of every slab, Adam on the whole slab
    events, s = _recorded_tail(2, 0, n_slabs=4, sharded=False)
    assert events == [
        ('produce', 0, 4), ('start', 'ar', 'g', 0, 120),
        ('produce', 4, 4), ('start', 'ar', 'g', 120, 240),
        ('produce', 8, 4), ('start', 'ar', 'g', 240, 360), ('wait', 'ar0'), ('adam', (0, 4), 0.5),
        ('produce', 12, 4), ('start', 'ar', 'g', 360, 480), ('wait', 'ar1'), ('adam', (4, 4), 0.5),
        ('wait', 'ar2'), ('adam', (8, 4), 0.5),
        ('wait', 'ar3'), ('adam', (12, 4), 0.5),
        ('bind', 'x1')]
    assert s._g_shards is None and s._epoch_plan == ('taken', None)
    # one rank: nothing is exchanged, whatever plan is asked for; accumulated minibatches are averaged
    events, s = _recorded_tail(1, 0, n_slabs=4, sharded=True, n_acc=4)
    assert events == [('produce', 0, 16), ('adam', None, 0.25), ('bind', 'x1')] and s._epoch_plan is None
    events, s = _recorded_tail(1, 0, one_pass=True)
    assert events == [('one_pass', (7, 0.25, 1e-3, 2e-3, 3e-3, False, True), 1.0), ('bind', 'x1')]


def test_control_plane_messages_are_parsed_not_executed(tmp_path):
    """The rendezvous socket carries None / bytes / numpy arrays / JSON values in a typed encoding (no pickle), lives in a
    directory only this user can enter, and both ends check the peer's uid (round-2 advice)."""
    from beyond_dof_amd import comm
    for obj in (None, b'\x00\x01' * 64, [3, 'host', 1.5], {'a': [1, 2]}, 7):
        assert comm._decode(comm._encode(obj)) == obj
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    b = comm._decode(comm._encode(a))
    assert b.dtype == a.dtype and np.array_equal(a, b)
    items = comm._decode(comm._encode_list([comm._encode(None), comm._encode(a), comm._encode([1, 2])]))
    assert items[0] is None and np.array_equal(items[1], a) and items[2] == [1, 2]
    with pytest.raises(TypeError):
        comm._encode(np.array([object()]))
    with pytest.raises(ValueError):
        comm._decode(b'\x80\x04junk')                 # a pickle stream is just a malformed message
    src = open(comm.__file__).read()
    assert 'import pickle' not in src and 'pickle.loads' not in src
    d = comm.rendezvous_dir()
    st = os.stat(d)
    assert st.st_uid == os.getuid() and (st.st_mode & 0o077) == 0
    os.environ.pop('BDOF_RDZV', None)
    assert os.path.dirname(comm.rendezvous_path()) == d


@pytest.mark.timeout(300)
@pytest.mark.parametrize('backend', ['rccl', 'gloo'])
def test_bench_self_launch_eight_ranks_rehearsal(backend):
    """`python bench.py --gpus 8` end to end without a GPU (--rehearse-cpu): the parent starts eight ranks, they meet (native
    control plane: socket star in a private directory; gloo: TCP store), cover the 200 angles of cfg3 between them, exchange
    through the backend, take the max-over-ranks time, and rank 0 prints exactly one JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR', 'BDOF_RDZV')}
    env['BDOF_COMM_BACKEND'] = backend
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '8', '--rehearse-cpu', '--steps', '3', '--warmup', '1'],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d['n_gpus'] == 8 and d['rehearsal'] and d['config']['angles_covered'] == 200 and d['config']['exchange_ok']
