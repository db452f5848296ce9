"""The fixtures of tests/menu_edges.py against the host rules, without a
device: every claimed edge pair is the variant's under its one-variant
backend, every claimed edge is an equality recomputed from the public host
functions (`classify` through the host plan, `oc_slots_needed`, `oc_trips`,
`slots_needed`, `grid_of`, `lds_bytes`), the next pair up of a capacity edge
is refused, and the menu is covered: an entry without a fixture is in
`menu_edges.UNREACHABLE` with the rule that excludes it, an edge without a
pair in `menu_edges.NOT_REACHED` -- and what can be evaluated of either is."""
import numpy as np
import pytest

import menu_edges as me
from graphdot_amd.kernel.marginalized._backend_hip import (
    GENERAL, LDS_LIMIT, OC_QUOTIENT_LAYOUTS, OC_VARIANTS, VARIANTS)

FIXTURES = list(me.fixtures())
RNAME = {real: name for name, real in me.REALS.items()}
IDS = [f'{me.variant_id(v)}-{RNAME[real]}-C{C}' for v, real, C, _, _ in FIXTURES]


def _plan(v, real, C, graphs):
    b = me.one_variant_backend(v, real)
    k = me.kernel_on(b, real)
    traits = k.traits(symmetric=True, eval_gradient=C == 2)
    jobs = me.triu_jobs(len(graphs))
    at = {(int(i), int(j)): t for t, (i, j) in enumerate(jobs.tolist())}
    return b, k, traits, jobs, at


@pytest.mark.parametrize('v,real,C,graphs,edges', FIXTURES, ids=IDS)
def test_edge_pairs_are_the_variants_and_sit_on_their_edges(v, real, C,
                                                            graphs, edges):
    b, k, traits, jobs, at = _plan(v, real, C, graphs)
    assert b.variants == [v, GENERAL]
    assert len(graphs) <= 12
    which = me.assignment(b, k, graphs, jobs, traits)
    assert set(which.tolist()) <= {0, 1}
    m = me.pair_metrics(b, k, graphs, v, jobs['i'], jobs['j'], traits)
    cap = 64 * v.W * v.R
    assert edges, 'a fixture without an edge'
    assert set(edges) | set(edges.cross) <= set(me.edges_of(v))
    assert not set(edges) & set(edges.cross)
    for name, (i, j) in edges.items():
        t = at[(i, j)]
        # index 0: the variant, not GENERAL
        assert which[t] == 0, (name, i, j)
        assert me.edge_holds(name, v, m, t), (name, i, j)
    # the equalities once more, spelled out
    e = {name: at[p] for name, p in edges.items()}
    assert int(m['N'][e['full']]) == edges.N_full <= cap
    assert int(m['N'][which == 0].max()) == edges.N_full
    if 'one_row' in e:
        assert m['N'][e['one_row']] == 64 * v.W * (v.R - 1) + 1
    if 'no_last' in e:
        assert m['N'][e['no_last']] == 64 * v.W * (v.R - 1)
    if 'slots_full' in e:
        assert m['slots'][e['slots_full']] == v.S
    if 'max_degree' in e:
        assert m['deg_hi'][e['max_degree']] == v.D
    if 'trips_full' in e:
        assert m['trips'][e['trips_full']][:v.R].tolist() == list(v.L)
    if 'trips_first' in e:
        tr = m['trips'][e['trips_first']]
        assert tr[0] == v.L[0] and tr[v.R - 1] == 0
    if 'grid' in e:
        t = e['grid']
        assert (m['deg_hi'][t], m['deg_lo'][t]) == b.grid_of(v.L, v.D)
    if 'smallest' in e:
        assert m['N'][e['smallest']] == m['N'][which == 0].min()
    if 'stride' in e:
        i, j = edges['stride']
        assert m['n1'][e['stride']] % 2 == 0 and m['n2'][e['stride']] % 2 == 1
        assert m['NP'][e['stride']] != m['n2'][e['stride']] * (
            m['n1'][e['stride']] | 1)
        both = me.assignment(b, k, graphs, me.cross_jobs([(i, j), (j, i)]),
                             k.traits(eval_gradient=C == 2))
        assert both.tolist() == [0, 0]
    # the edges taken as a call k([a], [b]) of their own
    for name, pair in edges.cross.items():
        assert name in ('one_row', 'no_last', 'slots_full')
        tr = k.traits(eval_gradient=C == 2)
        one = me.cross_jobs([(0, 1)])
        assert me.assignment(b, k, list(pair), one, tr).tolist() == [0], name
        m2 = me.pair_metrics(b, k, list(pair), v, [0], [1], tr)
        if name == 'slots_full':
            assert m2['slots'][0] == v.S
        else:
            assert m2['N'][0] == me.row_target(v, name)


@pytest.mark.parametrize('v,real,C,graphs,edges', FIXTURES, ids=IDS)
def test_the_next_pair_up_is_refused(v, real, C, graphs, edges):
    """Both sides of the boundary: one node more than the full pair, one
    slot more than the full slot walk -- not the variant's."""
    b, k, traits, jobs, at = _plan(v, real, C, graphs)
    cap = 64 * v.W * v.R
    # every fixture names the next pair up of its full pair, and of a full
    # slot walk
    assert 'full' in edges.beyond
    if 'slots_full' in edges:
        assert 'slots_full' in edges.beyond
    m = me.pair_metrics(b, k, graphs, v, jobs['i'], jobs['j'], traits)
    for name, recipes in edges.beyond.items():
        g2 = me.make_graphs(recipes)
        one = me.cross_jobs([(0, 1)])
        assert me.assignment(b, k, g2, one, traits).tolist() == [1], name
        m2 = me.pair_metrics(b, k, g2, v, [0], [1], traits)
        if name == 'full':
            # the full pair with one graph grown by one node (two where the
            # generator has no graph of that size, or where the padded row
            # n2 | 1 makes one more node the same pair to the rules)
            t = at[edges['full']]
            grown = sorted((int(m2['n1'][0]) - int(m['n1'][t]),
                            int(m2['n2'][0]) - int(m['n2'][t])))
            assert grown in ([0, 1], [0, 2]), grown
            if edges.N_full == cap:
                assert m2['N'][0] > cap
        if name == 'slots_full':
            # refused by the slot rule alone: N and the degrees would fit.
            # One slot more where the walks of the pool come that close
            # (menu_edges.SLOT_STEP: the smallest walk above S otherwise)
            assert m2['N'][0] <= cap
            step = me.SLOT_STEP.get(me.variant_id(v), 1)
            assert m2['slots'][0] == v.S + step
            if me.kind_of(v) == 'dynamic':
                assert m2['deg_hi'][0] <= v.D


def test_the_menu_is_covered():
    """Every entry of OC_VARIANTS + VARIANTS but the quotient layouts has a
    fixture for every (real, C) -- or stands in UNREACHABLE, and then the
    rule named there does exclude every pair."""
    have = {(me.variant_id(v), RNAME[r], C) for v, r, C, _, _ in FIXTURES}
    want = set()
    for rname, real in me.REALS.items():
        for C in (1, 2):
            entries = me.menu(real, C)
            assert set(OC_VARIANTS + VARIANTS) - set(entries) == {
                v for v in OC_VARIANTS if v.L in OC_QUOTIENT_LAYOUTS}
            want |= {(me.variant_id(v), rname, C) for v in entries}
    assert have | set(me.UNREACHABLE) == want
    assert not have & set(me.UNREACHABLE), 'listed as unreachable, yet reached'
    by_id = {me.variant_id(v): v for v in OC_VARIANTS + VARIANTS}
    for (vid, rname, C), rule in me.UNREACHABLE.items():
        v = by_id[vid]
        b = me.one_variant_backend(v, me.REALS[rname])
        assert rule == 'lds'
        # the LDS of a workgroup without any pair in it is over the limit
        assert b.lds_bytes(v, C, 0, 0) > LDS_LIMIT, (vid, rname, C)


def test_every_edge_is_claimed_or_recorded_as_not_reached():
    """An edge a fixture does not sit on is a recorded finding
    (menu_edges.NOT_REACHED), not a silent gap; every static layout has its
    pair with trips == L in every batch; and a row edge (`one_row`,
    `no_last`) is recorded only where the variant takes not even the
    sparsest pair of any factorisation of that row count -- evaluated here,
    so the table cannot absorb an edge the rules reach."""
    for v, real, C, graphs, edges in FIXTURES:
        key = (me.variant_id(v), RNAME[real], C)
        missing = set(me.edges_of(v)) - set(edges) - set(edges.cross)
        assert missing == set(me.NOT_REACHED.get(key, ())), key
        assert {'full', 'smallest'} <= set(edges)
        assert missing <= {'one_row', 'no_last'}, key
        for name in missing:
            # (a composite row count always has pairs to offer)
            target = me.row_target(v, name)
            if any(target % d == 0 for d in range(2, int(target ** .5) + 1)):
                assert me.factor_pairs(v, target), (key, name)
            for ra, rb in me.factor_pairs(v, me.row_target(v, name)):
                assert not me.cross_pair_taken(v, real, C, name, ra, rb), \
                    (key, name, ra, rb)


def test_sources_are_one_variant_translation_units():
    """`sources()` without compiling: labelled translation units of one
    entry point each -- the variant, the general solver or the table kernel
    -- for every call of every (variant, real): value, gradient, the two
    roles, the cross calls, nodal for the representatives."""
    labels = set()
    for label, flags, src in me.sources():
        assert label.startswith('menu_edges/') and isinstance(flags, tuple)
        assert src.count('extern "C" __global__') == 1
        labels.add(tuple(label.split('/')[1:4]))
    for v, real, C, graphs, edges in FIXTURES:
        what = 'value' if C == 1 else 'gradient'
        assert (RNAME[real], what, me.variant_id(v)) in labels
        if C == 1 and 'stride' in edges:
            assert (RNAME[real], 'roles_yx', me.variant_id(v)) in labels
        for name in edges.cross:
            assert (RNAME[real], f'cross_{name}_C{C}',
                    me.variant_id(v)) in labels
    for v in me.nodal_representatives():
        assert ('f32', 'nodal', me.variant_id(v)) in labels
