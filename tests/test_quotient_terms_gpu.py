"""The quotient value kernels on the half-term records of the arena (mgk_oc.h
RECS) on the device: the hand-built molecules with
neopentane and trimethylamine and 30 graphs of the QM7-like set -- every valid
/ invalid combination of a cell of the 4 x 3 and 4 x 4 grids among the first
batches, as tests/test_quotient_setup_gpu.py establishes it -- against the
same backend on the full images by the rules of tests/test_quotient_gpu.py;
repeats, symmetry and a cross call with swapped roles bit for bit; and a
weighted tree against the oracle."""
import numpy as np
import pytest

import cases
from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
from oracle import mgk as oracle
from test_quotient_gpu import ROUNDING_SAFE_FTOL
from test_quotient_layouts import layout_graphs, quotients
from test_quotient_setup_gpu import first_batch_rows
from test_quotient_terms import weighted_tree

pytestmark = pytest.mark.gpu

REALS = (np.float32, np.float64)
BOUND = {np.float32: 1e-5, np.float64: 1e-11}      # (test_quotient_gpu, 1e-13)


@pytest.fixture(scope='module')
def graphs():
    """graphs; `lo` / `hi`: those whose quotient has largest degree <= 3 / 4"""
    _, G = layout_graphs(30)
    md = np.array([int(q.adjacency_count.max()) for q in quotients(G)])
    return G, np.flatnonzero(md <= 3), np.flatnonzero(md == 4)


@pytest.fixture(scope='module')
def results(graphs):
    G, lo, hi = graphs
    X, Y = [G[k] for k in lo], [G[k] for k in hi]
    knode, kedge, q = cases.config3_kernels()
    out = {}
    for real in REALS:
        on = HIPBackend(real=real, min_launch=0, record_iterations=True)
        off = HIPBackend(real=real, quotient=False, record_iterations=True)
        r = {}
        for name, be in (('on', on), ('off', off)):
            k = MarginalizedGraphKernel(knode, kedge, q=q, backend=be,
                                        ftol=1e-13)
            r[name] = {'K': k(G)}
            r[name]['quotient'] = [be.last_plan.quotient]
            if be is on:
                r['rows'] = first_batch_rows(be, real)
                r['again'] = k(G)
            r[name]['Kxy'], r[name]['diag'] = k(X, Y), k.diag(G)
            r[name]['quotient'].append(be.last_plan.quotient)
            MarginalizedGraphKernel(knode, kedge, q=q, backend=be,
                                    ftol=ROUNDING_SAFE_FTOL)(G)
            r[name]['it'] = be.iterations(be.last_plan).astype(np.int64)
        out[real] = r
    return out


def _rel(a, b):
    return float(np.max(np.abs(a / b - 1)))


@pytest.mark.parametrize('real', REALS)
def test_every_cell_of_both_grids_runs(results, graphs, real):
    _, lo, hi = graphs
    assert len(lo) and len(hi)
    assert all(results[real]['on']['quotient'])
    assert not any(results[real]['off']['quotient'])
    seen, sizes = results[real]['rows']
    want = {(a, b) for a in range(1, 5) for b in range(1, 5)}
    assert want <= seen, sorted(want - seen)
    assert (sizes < 64).any() and (sizes > 64).any()


@pytest.mark.parametrize('real', REALS)
def test_values_are_those_of_the_full_images(results, real):
    on, off = results[real]['on'], results[real]['off']
    figures = {name: _rel(on[name], off[name])
               for name in ('K', 'Kxy', 'diag')}
    print(real.__name__, figures)
    assert max(figures.values()) <= BOUND[real], figures


@pytest.mark.parametrize('real', REALS)
def test_iteration_counts_are_those_of_the_full_images(results, real):
    """At most one step apart, on at most 2 % of the pairs, at
    ROUNDING_SAFE_FTOL (test_quotient_gpu)."""
    d = np.abs(results[real]['on']['it'] - results[real]['off']['it'])
    print(real.__name__, 'pairs', len(d), 'differ', int((d > 0).sum()),
          'max', int(d.max()))
    assert d.max() <= 1
    assert (d > 0).sum() <= 0.02 * len(d)


@pytest.mark.parametrize('real', REALS)
def test_repeat_symmetry_and_swapped_roles_bit_for_bit(results, graphs, real):
    """The cross call has the graphs with a four-valent node second: the
    kernel of the 4 x 3 grid swaps the roles (mgk_oc.h ORIENT), as it does
    for the mirrored half of the symmetric call."""
    _, lo, hi = graphs
    r = results[real]
    K = r['on']['K']
    assert np.array_equal(K, r['again'])
    assert np.array_equal(K, K.T)
    assert np.array_equal(r['on']['Kxy'], K[np.ix_(lo, hi)])


@pytest.mark.parametrize('real', REALS)
def test_weighted_tree_against_the_oracle(real):
    """The edge weights multiply the table value ahead of the scales, as
    before; the tolerance is the one of tests/test_parity_gpu.py for weighted
    graphs."""
    G = weighted_tree() * 2
    knode, kedge, q = cases.config2b_kernels()
    be = HIPBackend(real=real)
    K = MarginalizedGraphKernel(knode, kedge, q=q, backend=be)(G)
    assert be.last_plan.quotient
    ref = oracle.gram(G, knode, kedge, q=q)
    print(real.__name__, _rel(K, ref))
    assert np.allclose(K, ref, rtol=1e-5)
    assert np.array_equal(K, K.T)
