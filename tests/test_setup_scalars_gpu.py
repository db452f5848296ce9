"""The pair-independent set-up of the one-wave quotient solvers (mgk_oc.h QSET,
EVSC, LANE_TABS; DESIGN.md section 4a "set-up scalars") on the device: the
rectangle tables computed per lane from the degree histograms, staging loads
without a per-lane guard, the scalars of the evaluation read from behind the
tables, and the output addresses loaded next to the headers.

Small sets of at most 30 graphs; every backend is built without launch
merging (`min_launch=0`), so that a pair runs on the kernel of its own layout
whatever else the call holds -- which is what makes "bit-equal to the matrix
assembled pair by pair" a statement about addressing, and takes the pairs
through several layouts instead of the one they would be merged into."""
import copy
import os
import sys

import networkx as nx
import numpy as np
import pytest

import cases
from graphdot_amd.graph import Graph
from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
from oracle import mgk as oracle
from test_quotient import _atom, _bond, hand_built, molecule, weighted_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTOL = 1e-8
#: the suite's parity tolerance of the double build at FTOL
#: (tests/test_quotient_gpu.py, tests/test_parity_gpu.py)
RTOL = 2e-7


def all_classes(heavy):
    """A graph without hydrogens whose nodes have 4, 3, 2, 2, 1 and 0
    neighbours: every degree class 0..4 of the D = 4 kernels is occupied."""
    g = molecule(heavy, [(0, 1, 1), (0, 2, 1), (0, 3, 2), (0, 4, 1),
                         (1, 2, 1), (1, 3, 1)], [0] * len(heavy))
    return g


def single_node():
    g = nx.Graph()
    _atom(g, 0, 6)
    _bond(g, 0, 0)        # (a graph needs an edge: one node, one self loop)
    return g


def graph_set():
    """name -> nx graph: the hand-built molecules, a single node, a molecule
    with an isolated atom, two graphs with all five degree classes, and a few
    molecules of the benchmark's set."""
    out = {name: g for name, (g, _, _) in hand_built().items()}
    out['single_node'] = single_node()
    iso = molecule([6, 8, 7], [(0, 1, 1)], [3, 1, 0])     # the nitrogen is alone
    out['isolated_node'] = iso
    out['all_classes_a'] = all_classes([6, 6, 7, 8, 9, 16])
    out['all_classes_b'] = all_classes([7, 6, 6, 6, 8, 8])
    return out


@pytest.fixture(scope='module')
def graphs():
    built = graph_set()
    gs = [Graph.from_networkx(g) for g in built.values()]
    gs = Graph.unify_datatype(gs + cases.config3_graphs(12, seed=5))
    assert len(gs) <= 30
    return list(built), gs


def backend(**kw):
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    kw.setdefault('real', np.float64)
    kw.setdefault('min_launch', 0)
    return HIPBackend(**kw)


def kernel(be, ftol=FTOL, q=None):
    knode, kedge, q0 = cases.config3_kernels()
    return MarginalizedGraphKernel(knode, kedge, q=q0 if q is None else q,
                                   backend=be, ftol=ftol)


@pytest.fixture(scope='module')
def reference(graphs):
    """Oracle values of the upper triangle, computed once."""
    _, gs = graphs
    knode, kedge, q = cases.config3_kernels()
    i, j = np.triu_indices(len(gs))
    ref, _ = oracle.TensorProductBatch(gs, knode, kedge).run(
        i, j, q=q, tol=FTOL, real='f64')
    return i, j, ref


@pytest.fixture(scope='module')
def evaluated(graphs):
    """K(X), K(X, Y) in both role orders, diag(X) and the iteration counts of
    the default double build, twice (repeatability)."""
    _, gs = graphs
    m = len(gs) // 2
    runs = []
    for _ in range(2):
        be = backend(record_iterations=True)
        k = kernel(be)
        r = {'K': k(gs)}
        r['quotient'] = be.last_plan.quotient
        r['it'] = be.iterations(be.last_plan).astype(np.int64)
        r['layouts'] = {str(L['variant']) for L in be.last_plan.launches}
        r['Kxy'] = k(gs[:m], gs[m:])
        r['quotient'] &= be.last_plan.quotient
        r['Kyx'] = k(gs[m:], gs[:m])
        r['quotient'] &= be.last_plan.quotient
        r['diag'] = k.diag(gs)
        runs.append(r)
    return runs


def test_degree_histograms_values_against_the_oracle(graphs, reference,
                                                      evaluated):
    """(a) every degree class on both sides and in both role orders, pairs
    with most rectangles empty (methane x water) and with all of them
    occupied (the two all-classes graphs)."""
    names, gs = graphs
    i, j, ref = reference
    r = evaluated[0]
    m = len(gs) // 2
    assert r['quotient']
    print('layouts', sorted(r['layouts']))
    assert len(r['layouts']) > 1          # (not merged into one kernel)
    err = np.abs(r['K'][i, j] / ref - 1)
    print('max rel err vs oracle', err.max(), 'at',
          names[i[err.argmax()]] if i[err.argmax()] < len(names) else i[err.argmax()])
    assert np.allclose(r['K'][i, j], ref, rtol=RTOL, atol=0)
    assert np.array_equal(r['K'], r['K'].T)
    full = np.zeros_like(r['K'])
    full[i, j] = ref
    full[j, i] = ref
    assert np.allclose(r['Kxy'], full[:m, m:], rtol=RTOL, atol=0)
    assert np.allclose(r['Kyx'], full[m:, :m], rtol=RTOL, atol=0)
    assert np.allclose(r['diag'], np.diag(full), rtol=RTOL, atol=0)


def test_degree_histograms_iteration_counts(graphs):
    """(a) iteration counts against the solve on the full images, compared as
    tests/test_quotient_gpu.py compares them: the double build with double
    scalars at FTOL, at most one step apart on at most 2 % of the pairs."""
    _, gs = graphs
    its = {}
    for quotient in (True, False):
        be = backend(quotient=quotient, record_iterations=True,
                     hipcc_extra=['-DGD_OC_FSCAL=0'])
        kernel(be)(gs)
        assert be.last_plan.quotient == quotient
        its[quotient] = be.iterations(be.last_plan).astype(np.int64)
    d = np.abs(its[True] - its[False])
    print('pairs', len(d), 'differ', int((d > 0).sum()), 'max', int(d.max()),
          'mean iterations', its[True].mean(), its[False].mean())
    assert d.max() <= 1
    assert (d > 0).sum() <= 0.02 * len(d)


def test_weighted_hand_built_pair():
    """(a) the tenth hand-built case, weighted stars, against the dense
    solve of the oracle's matrix."""
    gs = weighted_pair()
    knode, kedge, q = cases.config2b_kernels()
    be = backend()
    K = MarginalizedGraphKernel(knode, kedge, q=q, backend=be, ftol=FTOL)(gs)
    assert be.last_plan.quotient
    for a, b in ((0, 0), (0, 1), (1, 1)):
        s1, s2 = oracle._side(gs[a]), oracle._side(gs[b])
        A, Dx = oracle.assemble(s1, s2, oracle.node_table(knode, s1, s2),
                                oracle.edge_table(kedge, s1, s2), q)
        assert K[a, b] == pytest.approx(np.linalg.solve(A, Dx).sum(), rel=RTOL)


def test_repeatability(evaluated):
    """(e) two runs on fresh backends give the same bits."""
    a, b = evaluated
    for name in ('K', 'Kxy', 'Kyx', 'diag', 'it'):
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize('which', ['smallest', 'largest'])
def test_last_blob_of_the_arena(graphs, which):
    """(b) the staging loads read past the end of an image: with the smallest
    and with the largest image as the LAST blob of the arena the values are
    those of the run with it in the middle.  (A cross call, so that the pairs
    keep their role order when the second list is permuted.)"""
    from graphdot_amd.kernel.marginalized._devicegraph import pack_many
    _, gs = graphs
    size = [dg.n_nz * 64 + dg.n_node for dg in pack_many(gs, real=np.float64)]
    t = int(np.argmin(size) if which == 'smallest' else np.argmax(size))
    X = [g for k, g in enumerate(gs) if k != t][:8]
    rest = [g for k, g in enumerate(gs) if k != t][8:]
    half = len(rest) // 2
    middle = rest[:half] + [gs[t]] + rest[half:]
    last = rest + [gs[t]]
    Km = kernel(backend())(X, middle)
    Kl = kernel(backend())(X, last)
    assert np.array_equal(np.delete(Km, half, axis=1), Kl[:, :-1])
    assert np.array_equal(Km[:, half], Kl[:, -1])


def _refresh_sequence(be, gs):
    """Three evaluations on one backend: q, another q, another edge-kernel
    hyperparameter; returns the matrices and the kernels that made them."""
    k0 = kernel(be)
    k1 = copy.deepcopy(k0)
    k1.q = 0.5 * k0.q
    theta = k0.theta.copy()
    theta[-1] += 0.25                     # (the last one: an edge-kernel hyperparameter)
    k2 = k0.clone_with_theta(theta)
    k2.q = k0.q                           # (exp(log(q)) is an ulp off)
    assert k2.q == k0.q and k1.q != k0.q
    assert not np.array_equal(k2.theta, k0.theta)
    ks = [k0, k1, k2]
    return [k(gs) for k in ks], ks


def test_scalars_follow_the_evaluation(graphs):
    """(c) 1 / (1 - q)^2 and q^2 / q0^2 are written once per evaluation: a
    backend that has evaluated with one q gives, with another q and then with
    another kernel hyperparameter, the bits of a fresh backend."""
    _, gs = graphs
    be = backend()
    Ks, ks = _refresh_sequence(be, gs)
    assert not np.array_equal(Ks[0], Ks[1]) and not np.array_equal(Ks[0], Ks[2])
    for K, k in zip(Ks, ks):
        fresh = copy.deepcopy(k)
        fresh.backend = backend()
        assert np.array_equal(K, fresh(gs))


def _sharded_worker(rank, port, path):
    import torch
    import torch.distributed as dist
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=rank, world_size=1,
                            device_id=torch.device('cuda', 0))
    from graphdot_amd.kernel.marginalized._sharded import distributed_backend
    built = graph_set()
    gs = Graph.unify_datatype([Graph.from_networkx(g) for g in built.values()]
                              + cases.config3_graphs(12, seed=5))
    be = distributed_backend(device=0, shard_single_rank=True,
                             real=np.float64, min_launch=0)
    Ks, _ = _refresh_sequence(be, gs)
    assert be.last_step is not None
    np.savez(path, K0=Ks[0], K1=Ks[1], K2=Ks[2])
    dist.destroy_process_group()


def test_scalars_follow_the_evaluation_sharded(graphs, tmp_path):
    """(c) the same three evaluations through `ShardedStep` on a process
    group of one rank."""
    import torch.multiprocessing as mp
    _, gs = graphs
    path = str(tmp_path / 'sharded.npz')
    mp.spawn(_sharded_worker, args=(29900 + os.getpid() % 40, path), nprocs=1,
             join=True)
    r = np.load(path)
    Ks, _ = _refresh_sequence(backend(), gs)
    for n, K in enumerate(Ks):
        assert np.array_equal(r[f'K{n}'], K), n


JOB_T = np.dtype([('i', np.uint32), ('j', np.uint32)])


def _packed(be, k, gs, jobs):
    """Values of `jobs` (pairs of `gs`) in the packed output of one plan."""
    n = len(gs)
    plan = be.prepare(gs, k.node_kernel, k.edge_kernel, k.p, k.q, k.eps,
                      k.ftol, k.gtol, jobs, np.arange(n + 1, dtype=np.uint32),
                      n, n, k.n_dims, k.traits(symmetric=True), packed=True)
    be.launch(plan)
    out = be.collect(plan)
    out = out[0] if isinstance(out, tuple) else out
    return np.asarray(out).ravel()[:len(jobs)].copy(), plan


@pytest.mark.parametrize('record', [True, False], ids=['iters', 'no-iters'])
def test_output_addressing(graphs, record):
    """(d) K(X), K(X, Y) with len(X) != len(Y), diag(X) and the packed output
    of a job list equal, bit for bit, the matrix assembled pair by pair.

    A pair is solved alone as a job list of one pair OF THE SAME GRAPH LIST:
    whether a call takes the quotient images is decided on its whole list
    (`HIPBackend._quotient_graphs`: no twin group in the call, no quotient),
    so two graphs without hydrogens passed as lists of their own would run
    on the full-image kernels, other instantiations that agree with the
    quotient ones to rounding only."""
    _, gs = graphs
    gs = gs[:3] + gs[9:16]                # ten graphs, 55 one-pair plans
    n = len(gs)
    i, j = np.triu_indices(n)
    jobs = np.column_stack((i, j)).astype(np.uint32).ravel().view(JOB_T)
    one = backend(record_iterations=record)
    k1 = kernel(one)
    P = np.zeros((n, n))
    for t in range(len(jobs)):
        v, plan = _packed(one, k1, gs, jobs[t:t + 1])
        assert plan.quotient
        P[i[t], j[t]] = P[j[t], i[t]] = v[0]
    be = backend(record_iterations=record)
    k = kernel(be)
    K, Kxy, d = k(gs), k(gs[:3], gs[3:]), k.diag(gs)
    out, plan = _packed(be, k, gs, jobs[::2])
    print('max |rel diff| to the pair-by-pair matrix: K',
          np.abs(K / P - 1).max(), 'Kxy', np.abs(Kxy / P[:3, 3:] - 1).max(),
          'diag', np.abs(d / np.diag(P) - 1).max(), 'packed',
          np.abs(out / P[i[::2], j[::2]] - 1).max())
    assert np.array_equal(K, P)
    assert np.array_equal(Kxy, P[:3, 3:])
    assert np.array_equal(d, np.diag(P))
    assert np.array_equal(out, P[i[::2], j[::2]])
    if record:
        assert be.iterations(plan).min() >= 1
