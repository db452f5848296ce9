"""The slot set-up of the quotient value kernels with its table loads ahead of
the slot loop (mgk_oc.h GPRE) on the device.  First on
the host: among the first-batch rows of the pairs that run, every degree pair
(d1, d2) in {1..4} x {1..4} occurs -- every valid / invalid combination of a
grid cell -- and some pair has fewer than 64 rows: dead lanes, all later
batches empty.  Then the values of the symmetric call, of a cross call in both
orders and of diag against the C oracle in double at 1e-13, a repeat bit for
bit, and the iteration counts against the full images."""
import numpy as np
import pytest

import cases
from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
from oracle import mgk as oracle
from test_quotient_gpu import ROUNDING_SAFE_FTOL
from test_quotient_layouts import layout_graphs, p_cells, quotients

pytestmark = pytest.mark.gpu

REALS = (np.float32, np.float64)
BOUND = {np.float32: 1e-5, np.float64: 1e-11}   # (test_quotient_layouts_gpu)


@pytest.fixture(scope='module')
def graphs():
    """The hand-built molecules, neopentane and trimethylamine, 30 of the
    QM7-like set; `lo` / `hi`: quotient of largest degree <= 3 / 4."""
    _, G = layout_graphs(30)
    md = np.array([int(q.adjacency_count.max()) for q in quotients(G)])
    return G, np.flatnonzero(md <= 3), np.flatnonzero(md == 4)


def first_batch_rows(be, real):
    """Of the plan that just ran: the set of degree pairs (d1, d2) among the
    first 64 rows of its pairs -- rows sorted by descending d1 d2, ties in
    row-major order of (d1, d2) as mgk_oc.h class_order lays them out, the
    graphs in the roles the kernel gives them -- and the row counts."""
    lay = be.last_plan.layout
    jobs = lay.jobs_host
    deg = [q.adjacency_count.astype(np.int64) for q in lay.dgraphs]
    seen, sizes = set(), []
    for v, _, t, flip, _ in p_cells(lay.launches, lay.order_host, jobs,
                                    lay.dgraphs):
        assert v.W == 1 and HIPBackend.grid_of(v.L, v.D) is not None, v
        for k, f in zip(t.tolist(), flip.tolist()):
            a, c = int(jobs['i'][k]), int(jobs['j'][k])
            if f:
                a, c = c, a
            d1, d2 = np.meshgrid(deg[a], deg[c], indexing='ij')
            rows = sorted(zip((-d1 * d2).ravel().tolist(), d1.ravel().tolist(),
                              d2.ravel().tolist()))[:64]
            seen |= {(x, y) for _, x, y in rows if x and y}
            sizes.append(d1.size)
    return seen, np.array(sizes)


@pytest.fixture(scope='module')
def results(graphs):
    G, lo, hi = graphs
    X, Y = [G[k] for k in lo], [G[k] for k in hi]
    knode, kedge, q = cases.config3_kernels()
    out = {}
    for real in REALS:
        be = HIPBackend(real=real, min_launch=0, record_iterations=True)
        full = HIPBackend(real=real, quotient=False, record_iterations=True)
        k = MarginalizedGraphKernel(knode, kedge, q=q, backend=be, ftol=1e-13)
        r = {'K': k(G)}
        r['quotient'] = be.last_plan.quotient
        r['rows'] = first_batch_rows(be, real)
        r['again'] = k(G)
        r['Kxy'], r['Kyx'], r['diag'] = k(X, Y), k(Y, X), k.diag(G)
        r['quotient'] &= be.last_plan.quotient
        for name, b in (('it', be), ('it_full', full)):
            MarginalizedGraphKernel(knode, kedge, q=q, backend=b,
                                    ftol=ROUNDING_SAFE_FTOL)(G)
            r[name] = b.iterations(b.last_plan).astype(np.int64)
        out[real] = r
    return out


@pytest.fixture(scope='module')
def reference(graphs):
    """The C oracle in double at 1e-13, as the full symmetric matrix."""
    G, _, _ = graphs
    knode, kedge, q = cases.config3_kernels()
    i, j = np.triu_indices(len(G))
    ref = np.zeros((len(G), len(G)))
    ref[i, j] = oracle.TensorProductBatch(G, knode, kedge).run(
        i, j, q=q, tol=1e-13, real='f64')[0]
    ref[j, i] = ref[i, j]
    return ref


def _rel(a, b):
    return float(np.max(np.abs(a / b - 1)))


@pytest.mark.parametrize('real', REALS)
def test_first_batches_run_every_cell_of_the_grid(results, real):
    assert results[real]['quotient']
    seen, sizes = results[real]['rows']
    want = {(a, b) for a in range(1, 5) for b in range(1, 5)}
    print(real.__name__, 'pairs', len(sizes), 'below 64 rows',
          int((sizes < 64).sum()), 'missing', sorted(want - seen))
    assert want <= seen, sorted(want - seen)
    assert (sizes < 64).any() and (sizes > 64).any()


@pytest.mark.parametrize('real', REALS)
def test_values_are_the_oracles(results, reference, graphs, real):
    _, lo, hi = graphs
    r = results[real]
    block = reference[np.ix_(lo, hi)]
    figures = {'K': _rel(r['K'], reference), 'Kxy': _rel(r['Kxy'], block),
               'Kyx': _rel(r['Kyx'], block.T),
               'diag': _rel(r['diag'], np.diag(reference))}
    print(real.__name__, figures)
    assert max(figures.values()) <= BOUND[real], figures


@pytest.mark.parametrize('real', REALS)
def test_a_repeat_is_equal_bit_for_bit(results, real):
    r = results[real]
    assert np.array_equal(r['K'], r['again'])
    assert np.array_equal(r['K'], r['K'].T)


@pytest.mark.parametrize('real', REALS)
def test_iteration_counts_are_those_of_the_full_images(results, real):
    """The rule of test_quotient_layouts_gpu at ROUNDING_SAFE_FTOL: at most
    one step apart, on at most 2 % of the pairs."""
    r = results[real]
    d = np.abs(r['it'] - r['it_full'])
    print(real.__name__, 'pairs', len(d), 'differ', int((d > 0).sum()),
          'max', int(d.max()))
    assert d.max() <= 1
    assert (d > 0).sum() <= 0.02 * len(d)
