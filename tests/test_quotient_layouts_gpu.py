"""The static layouts cut to quotient pairs (mgk_oc.h GRID with GU x GV slots,
ORIENT) on the device: every new layout runs, in both
orientations of a 4 x 3 pair, and gives the values and iteration counts of the
full images -- symmetric, cross and diagonal calls, float and double, merged
and unmerged launches."""
import numpy as np
import pytest

import cases
from graphdot_amd.graph import Graph
from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
from oracle import mgk as oracle
from test_quotient import hand_built
from test_quotient_gpu import ROUNDING_SAFE_FTOL
from test_quotient_layouts import extra_molecules, p_cells

pytestmark = pytest.mark.gpu

FTOLS = (1e-8, 1e-13, ROUNDING_SAFE_FTOL)


@pytest.fixture(scope='module')
def graphs():
    """The graphs of test_quotient_gpu plus neopentane and trimethylamine;
    `lo` / `hi`: those whose quotient has largest degree <= 3 / 4."""
    from graphdot_amd.kernel.marginalized._devicegraph import (
        pack_many, quotient_graph)
    named = {k: g for k, (g, _, _) in hand_built().items()}
    named.update(extra_molecules())
    G = Graph.unify_datatype([Graph.from_networkx(g) for g in named.values()]
                             + cases.config3_graphs(30))
    md = np.array([int(quotient_graph(dg).adjacency_count.max())
                   for dg in pack_many(G, real=np.float64)])
    lo, hi = np.flatnonzero(md <= 3), np.flatnonzero(md == 4)
    assert len(lo) >= 4 and len(hi) >= 4
    return G, lo, hi


def roles(be):
    """Of the plan that just ran: layout -> [pairs, pairs that ran with
    swapped roles, cells of p to spare below the dump cell]."""
    lay = be.last_plan.layout
    out = {}
    for v, cells, t, flip, top in p_cells(lay.launches, lay.order_host,
                                          lay.jobs_host, lay.dgraphs):
        out[v.L] = [len(t), int(flip.sum()), int(cells - 1 - top.max())]
    return out


@pytest.fixture(scope='module')
def results(graphs):
    """(real, ftol, mode) -> K, Kxy (low-degree graphs first), Kyx, diag,
    iteration counts and the layouts that ran; mode 'layouts': quotient
    images with unmerged launches, 'merged': default launches, 'full'."""
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    G, lo, hi = graphs
    X, Y = [G[k] for k in lo], [G[k] for k in hi]
    knode, kedge, q = cases.config3_kernels()
    out = {}
    for real in (np.float32, np.float64):
        for mode, kw in (('layouts', dict(min_launch=0)), ('merged', {}),
                         ('full', dict(quotient=False))):
            be = HIPBackend(real=real, record_iterations=True, **kw)
            for ftol in FTOLS:
                k = MarginalizedGraphKernel(knode, kedge, q=q, backend=be,
                                            ftol=ftol)
                r = {'K': k(G)}
                r['quotient'] = be.last_plan.quotient
                r['it'] = be.iterations(be.last_plan).astype(np.int64)
                r['ran'] = {L['variant'].L: L['count']
                            for L in be.last_plan.launches}
                if mode == 'merged':
                    r['again'] = k(G)
                else:
                    r['Kxy'] = k(X, Y)
                    r['quotient'] &= be.last_plan.quotient
                    r['Kyx'] = k(Y, X)
                    r['quotient'] &= be.last_plan.quotient
                    if mode == 'layouts':
                        k(X, Y)
                        r['ran_xy'] = roles(be)
                        k(Y, X)
                        r['ran_yx'] = roles(be)
                    r['diag'] = k.diag(G)
                    r['quotient'] &= be.last_plan.quotient
                out[(real, ftol, mode)] = r
    return out


@pytest.fixture(scope='module')
def reference(graphs):
    """real -> the C oracle's values at 1e-8 on the upper triangle."""
    G, _, _ = graphs
    knode, kedge, q = cases.config3_kernels()
    i, j = np.triu_indices(len(G))
    batch = oracle.TensorProductBatch(G, knode, kedge)
    return i, j, {real: batch.run(i, j, q=q, tol=1e-8, real=name)[0]
                  for real, name in ((np.float32, 'f32'), (np.float64, 'f64'))}


def _rel(a, b):
    return float(np.max(np.abs(a / b - 1)))


def test_every_new_layout_runs(results):
    from graphdot_amd.kernel.marginalized._backend_hip import (
        OC_QUOTIENT_LAYOUTS)
    for real in (np.float32, np.float64):
        r = results[(real, 1e-8, 'layouts')]
        assert r['quotient']
        for L in OC_QUOTIENT_LAYOUTS:
            assert r['ran'].get(L, 0) >= 1, (L, r['ran'])
        # the cross call puts the graph of degree <= 3 first on every pair:
        # its 12-first launches run with swapped roles, pair for pair, those
        # of the reverse call as the jobs have them; 16-first ones never swap
        print(real.__name__, 'X x Y', r['ran_xy'], 'Y x X', r['ran_yx'])
        for ran, swapped in ((r['ran_xy'], True), (r['ran_yx'], False)):
            first12 = {L: c for L, c in ran.items() if L[0] == 12}
            assert first12, ran
            assert all(c[1] == (c[0] if swapped else 0)
                       for c in first12.values()), ran
            assert all(c[1] == 0 for L, c in ran.items() if L[0] != 12), ran
            assert all(c[2] >= 0 for c in ran.values()), ran


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('ftol', [1e-8, 1e-13])
def test_values_are_those_of_the_full_images(results, reference, graphs, real,
                                             ftol):
    _, lo, hi = graphs
    on, off = results[(real, ftol, 'layouts')], results[(real, ftol, 'full')]
    merged = results[(real, ftol, 'merged')]
    assert on['quotient'] and merged['quotient'] and not off['quotient']
    figures = {name: _rel(on[name], off[name])
               for name in ('K', 'Kxy', 'Kyx', 'diag')}
    figures['orders'] = _rel(on['Kxy'], on['Kyx'].T)
    figures['merged'] = _rel(merged['K'], off['K'])
    print(real.__name__, ftol, figures)
    assert np.array_equal(on['K'], on['K'].T)
    assert np.array_equal(merged['K'], merged['K'].T)
    assert np.array_equal(merged['K'], merged['again'])
    if ftol == 1e-13:
        bound = 1e-5 if real is np.float32 else 1e-11
        assert max(figures.values()) <= bound, figures
    else:
        i, j, ref = reference
        rtol = 1e-5 if real is np.float32 else 2e-7
        for r in (on, off, merged):
            assert np.allclose(r['K'][i, j], ref[real], rtol=rtol), \
                _rel(r['K'][i, j], ref[real])
        for r in (on, off):
            block = r['K'][np.ix_(lo, hi)]
            assert np.allclose(r['Kxy'], block, rtol=rtol)
            assert np.allclose(r['Kyx'].T, block, rtol=rtol)
            assert np.allclose(r['Kxy'], r['Kyx'].T, rtol=rtol)
            assert np.allclose(r['diag'], np.diag(r['K']), rtol=rtol)


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('mode', ['layouts', 'merged'])
def test_iteration_counts_are_those_of_the_full_images(results, real, mode):
    """The rule of test_quotient_gpu: the counts differ by at most one step on
    at most 2 % of the pairs, at ROUNDING_SAFE_FTOL on the default builds."""
    on = results[(real, ROUNDING_SAFE_FTOL, mode)]
    off = results[(real, ROUNDING_SAFE_FTOL, 'full')]
    d = np.abs(on['it'] - off['it'])
    print(real.__name__, mode, 'pairs', len(d), 'differ', int((d > 0).sum()),
          'max', int(d.max()), 'mean iterations', on['it'].mean(),
          off['it'].mean())
    assert d.max() <= 1
    assert (d > 0).sum() <= 0.02 * len(d)


@pytest.mark.parametrize('real', [np.float32, np.float64])
def test_a_swapped_pair_that_sizes_its_launch(graphs, real):
    """One pair per call, so that it is its launch's largest: a graph of
    largest degree <= 3 with an even number of quotient nodes against one of
    degree 4 with an odd number.  In the job's order p has n_lo n_hi cells, in
    the swapped roles the kernel runs it in n_hi (n_lo + 1): the launch must
    be sized for those.  Values: those of the full images and of the reverse
    order, within the bounds of test_values_are_those_of_the_full_images at
    1e-13."""
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    G, lo, hi = graphs
    knode, kedge, q = cases.config3_kernels()
    on = HIPBackend(real=real, min_launch=0)
    off = HIPBackend(real=real, quotient=False)
    kon = MarginalizedGraphKernel(knode, kedge, q=q, backend=on, ftol=1e-13)
    koff = MarginalizedGraphKernel(knode, kedge, q=q, backend=off, ftol=1e-13)
    from graphdot_amd.kernel.marginalized._devicegraph import (
        pack_many, quotient_graph)
    n = np.array([quotient_graph(dg).n_node
                  for dg in pack_many(G, real=np.float64)])
    bound = 1e-5 if real is np.float32 else 1e-11
    tried = 0
    for a in [g for g in lo if n[g] % 2 == 0][-2:]:
        for c in sorted((g for g in hi if n[g] % 2 == 1),
                        key=lambda g: n[g])[-2:]:
            Kxy = kon([G[a]], [G[c]])
            ran = roles(on)
            if not all(L[0] == 12 for L in ran):
                continue      # (a profile beyond the 12-first layouts)
            tried += 1
            (count, swapped, spare), = ran.values()
            assert (count, swapped) == (1, 1) and spare >= 0, ran
            # (the job's own order would have been too small for it)
            assert n[c] * (n[a] | 1) > n[a] * (n[c] | 1)
            Kyx = kon([G[c]], [G[a]])
            assert [c_[1] for c_ in roles(on).values()] == [0]
            ref = koff([G[a]], [G[c]])
            figures = (_rel(Kxy, ref), _rel(Kyx.T, ref), _rel(Kxy, Kyx.T))
            print(real.__name__, int(n[a]), int(n[c]), ran, figures)
            assert max(figures) <= bound, figures
    assert tried >= 1
