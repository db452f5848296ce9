"""The static layouts cut to the degrees of twin-leaf quotient pairs
(_backend_hip.OC_QUOTIENT_LAYOUTS, mgk_oc.h GRID / ORIENT, DESIGN.md section
4a): which layout a pair takes, that the first batch's grid holds it, that the
native and the numpy classification agree, that merged launches keep both, and
that the menu is really used on the QM7-like set.  Host only."""
import numpy as np
import pytest

import cases
from graphdot_amd.graph import Graph
from graphdot_amd.kernel.marginalized._backend_hip import (
    CallShape, HIPBackend, OCVariant, OC_QUOTIENT_LAYOUTS)
from graphdot_amd.kernel.marginalized._devicegraph import (
    pack_many, quotient_graph)
from test_quotient import hand_built, molecule

job_t = np.dtype([('i', np.uint32), ('j', np.uint32)])


def extra_molecules():
    """Quotients of largest degree 4 with no other node above 2 (neopentane)
    and of largest degree 3 (trimethylamine)."""
    star = [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1)]
    return {'neopentane': molecule([6] * 5, star, [0, 3, 3, 3, 3]),
            'trimethylamine': molecule([7, 6, 6, 6], star[:3], [0, 3, 3, 3])}


def layout_graphs(n_set):
    named = {k: g for k, (g, _, _) in hand_built().items()}
    named.update(extra_molecules())
    graphs = Graph.unify_datatype(
        [Graph.from_networkx(g) for g in named.values()]
        + cases.config3_graphs(n_set))
    return list(named), graphs


def quotients(graphs, real=np.float64):
    return [quotient_graph(dg) for dg in pack_many(graphs, real=real)]


def triu_jobs(n):
    i, j = np.triu_indices(n)
    return np.column_stack((i, j)).astype(np.uint32).ravel().view(job_t)


def profiles(qs, i, j):
    """oc_trips of every pair (i, j) of the quotient images."""
    hist = np.array([np.bincount(q.adjacency_count, minlength=5)[:5]
                     for q in qs], dtype=np.int64)
    return HIPBackend.oc_trips(hist[i], hist[j], 4, HIPBackend.TRIP_BATCHES)


def assert_holds(v, trips, md_i, md_j, what):
    """Static layout v dominates the profile and its grid fits the pair."""
    assert isinstance(v, OCVariant) and v.L, (what, v)
    cap = np.zeros(len(trips), dtype=np.int64)
    cap[:v.R] = v.L
    assert np.all(trips <= cap), (what, v.L, trips)
    grid = HIPBackend.grid_of(v.L, v.D)
    if grid is not None:
        assert max(md_i, md_j) <= grid[0] and min(md_i, md_j) <= grid[1], \
            (what, v.L, md_i, md_j)


def p_cells(launches, order, jobs, qs):
    """Per launch: (variant, cells of p below the dump cell, job indices,
    which of them run with swapped roles, highest cell of p each writes) --
    the kernel's own layout of p: n1 rows of stride n2 | 1 in the roles it
    gives the graphs (mgk_oc.h ORIENT), the dump cell at u_capacity - 1."""
    n = np.array([q.n_node for q in qs], dtype=np.int64)
    md = np.array([int(q.adjacency_count.max()) for q in qs])
    i, j = jobs['i'].astype(np.int64), jobs['j'].astype(np.int64)
    for L in launches:
        t = np.asarray(order[L['offset']:L['offset'] + L['count']],
                       dtype=np.int64)
        flip = HIPBackend.swaps_roles(L['variant'], md[j[t]])
        n1 = np.where(flip, n[j[t]], n[i[t]])
        n2 = np.where(flip, n[i[t]], n[j[t]])
        yield (L['variant'], L['ucap'] - 1, t, flip,
               (n1 - 1) * (n2 | 1) + n2 - 1)


@pytest.fixture(scope='module')
def small():
    names, graphs = layout_graphs(60)
    qs = quotients(graphs)
    maxdeg = np.array([int(q.adjacency_count.max()) for q in qs])
    return names, qs, maxdeg


def test_grids_of_the_first_segments():
    assert HIPBackend.grid_of((16, 4, 1), 4) == (4, 4)
    assert HIPBackend.grid_of((12, 3), 4) == (4, 3)
    assert HIPBackend.grid_of((9, 3), 4) == (3, 3)
    assert HIPBackend.grid_of((8, 2), 4) is None
    assert HIPBackend.grid_of(None, 4) is None


def test_every_pair_takes_a_layout_that_holds_it(small):
    names, qs, maxdeg = small
    i, j = np.triu_indices(len(qs))
    trips = profiles(qs, i, j)
    out = []
    for native in (True, False):
        b = HIPBackend(real=np.float64, native=native)
        choice = b.classify(i, j, qs, 1, gtab=True)[0]
        for t, k in enumerate(choice.tolist()):
            assert_holds(b.variants[k], trips[t], maxdeg[i[t]], maxdeg[j[t]],
                         (int(i[t]), int(j[t])))
        out.append(choice)
    assert np.array_equal(*out)
    # the layouts cut for quotients are in use, for 4 x 3 pairs in both orders
    b = HIPBackend(real=np.float64)
    taken = {b.variants[k].L for k in out[0].tolist()}
    assert taken & set(OC_QUOTIENT_LAYOUTS)
    first12 = np.array([b.variants[k].L[0] == 12 for k in out[0].tolist()])
    assert np.any(first12 & (maxdeg[i] == 3) & (maxdeg[j] == 4))
    assert np.any(first12 & (maxdeg[i] == 4) & (maxdeg[j] == 3))
    # largest degrees (4, 2): eight terms, inside the 4 x 3 grid
    a, e = names.index('neopentane'), names.index('ethane')
    t = int(np.flatnonzero((i == min(a, e)) & (j == max(a, e)))[0])
    assert (maxdeg[a], maxdeg[e]) == (4, 2) and trips[t][0] == 8
    assert b.variants[out[0][t]].L[0] == 12


def test_full_images_keep_their_menu(small):
    """The new layouts are offered to quotient images only: gradient plans and
    full images are classified as before."""
    _, graphs = layout_graphs(20)
    dgs = pack_many(graphs, real=np.float64)
    b = HIPBackend(real=np.float64)
    for C, gs in ((1, dgs), (2, dgs), (2, small[1])):
        i, j = np.triu_indices(len(gs))
        choice = b.classify(i, j, gs, C, gtab=True)[0]
        assert not {b.variants[k].L for k in choice.tolist()} \
            & set(OC_QUOTIENT_LAYOUTS)


@pytest.mark.parametrize('min_launch', [8192, 300, 0])
def test_merged_launches_hold_their_pairs(small, min_launch):
    _, qs, maxdeg = small
    jobs = triu_jobs(len(qs))
    trips = profiles(qs, jobs['i'].astype(np.int64), jobs['j'].astype(np.int64))
    out = []
    for native in (True, False):
        b = HIPBackend(real=np.float64, native=native, min_launch=min_launch)
        _, used, order, launches = b._partition(
                qs, jobs, CallShape(1, quot=True, gtab=True))
        seen = 0
        for L in launches:
            for t in order[L['offset']:L['offset'] + L['count']].tolist():
                a, c = int(jobs['i'][t]), int(jobs['j'][t])
                assert_holds(L['variant'], trips[t], maxdeg[a], maxdeg[c],
                             (a, c))
            seen += L['count']
        assert seen == len(jobs)
        out.append((used, [(L['variant'], L['offset'], L['count'])
                           for L in launches], order))
    assert out[0][:2] == out[1][:2] and np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize('min_launch', [8192, 0])
@pytest.mark.parametrize('seed', [1, 2, 3, 4])
def test_p_holds_every_pair_in_the_roles_the_kernel_gives_it(small, seed,
                                                             min_launch):
    """n1 (n2 | 1) is not symmetric (8 x 9: 72 cells, 9 x 8: 81): a launch
    whose kernel swaps the roles of some pairs sizes p for the order that
    runs.  Small cross lists, five graphs of largest degree <= 3 against five
    of degree 4 in both orders, so that a few pairs of mixed parity decide the
    size of every launch."""
    _, qs, maxdeg = small
    rng = np.random.default_rng(seed)
    lo = rng.choice(np.flatnonzero(maxdeg <= 3), 5, replace=False)
    hi = rng.choice(np.flatnonzero(maxdeg == 4), 5, replace=False)
    swapped = {}
    for name, (X, Y) in (('lo x hi', (lo, hi)), ('hi x lo', (hi, lo))):
        a, c = np.meshgrid(X, Y, indexing='ij')
        jobs = np.column_stack((a.ravel(), c.ravel())).astype(np.uint32) \
            .ravel().view(job_t)
        plans = []
        for native in (True, False):
            b = HIPBackend(real=np.float64, native=native,
                           min_launch=min_launch)
            _, _, order, launches = b._partition(
                qs, jobs, CallShape(1, quot=True, gtab=True))
            swapped[name] = 0
            for v, cells, t, flip, top in p_cells(launches, order, jobs, qs):
                assert np.all(top < cells), (name, v, cells, int(top.max()))
                swapped[name] += int(flip.sum())
            plans.append([(L['variant'], L['ucap'], L['count'])
                          for L in launches])
        assert plans[0] == plans[1]
    if min_launch == 0:
        # (every 4 x 3 pair of the order that puts the degree-4 graph second)
        assert swapped['lo x hi'] > 0 and swapped['hi x lo'] == 0


def test_a_narrow_launch_never_rides_in_a_narrower_grid():
    v = {L: HIPBackend(real=np.float64).variants[k] for k, L in
         ((k, x.L) for k, x in enumerate(HIPBackend(real=np.float64).variants)
          if getattr(x, 'L', None))}
    takes = HIPBackend._grid_takes
    assert takes(v[(16, 3)], v[(12, 3)]) and takes(v[(16, 4)], v[(12, 3)])
    assert takes(v[(12, 3, 1)], v[(12, 3)])
    assert not takes(v[(12, 3, 1)], v[(16,)])
    assert not takes(v[(12, 3)], v[(16, 3)])


def test_the_qm7_like_set_uses_the_menu():
    """All 500 500 quotient pairs of the 1000-graph set find a static layout,
    at no more than 17.8 slots per lane on average (the menu before the
    quotient layouts: 20.47; with them: 17.53)."""
    qs = quotients(cases.config3_graphs(1000))
    i, j = np.triu_indices(len(qs))
    b = HIPBackend(real=np.float64)
    choice = b.classify(i, j, qs, 1, gtab=True)[0]
    variants = [b.variants[k] for k in sorted(set(choice.tolist()))]
    assert all(isinstance(v, OCVariant) and v.L for v in variants), variants
    slots = np.array([getattr(v, 'S', 0) for v in b.variants])[choice]
    print('mean slots per lane', slots.mean())
    assert slots.mean() <= 17.8
