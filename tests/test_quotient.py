"""Twin-leaf quotient images: detection of the twin
groups, the quotient image of the native packer against its numpy
specification, and the exactness of the rescaled quotient system -- solved
densely in float64 against the full system of the oracle's assembly."""
import itertools
import networkx as nx
import numpy as np
import pytest

import cases
from graphdot_amd.graph import Graph
from graphdot_amd.kernel.marginalized._devicegraph import (
    GraphArena, pack_many, quotient_graph, twin_groups)
from oracle import mgk as oracle


def _atom(g, v, Z, hcount=0, aromatic=False, **extra):
    g.add_node(v, atomic_number=Z, charge=0, hcount=hcount, hybridization=4,
               aromatic=aromatic, chiral=0, **extra)


def _bond(g, u, v, order=1.0, **extra):
    g.add_edge(u, v, order=float(order), aromatic=False,
               conjugated=bool(order > 1), stereo=0, ring_stereo=0.0, **extra)


def molecule(heavy, bonds, hydrogens):
    """nx graph: heavy atoms [Z], bonds [(u, v, order)], hydrogens per heavy
    atom [count]; attributes as cases.qm7_like_molecule gives them."""
    g = nx.Graph()
    for u, Z in enumerate(heavy):
        _atom(g, u, Z, hcount=hydrogens[u])
    h = len(heavy)
    for u, k in enumerate(hydrogens):
        for _ in range(k):
            _atom(g, h, 1)
            _bond(g, u, h)
            h += 1
    for u, v, o in bonds:
        _bond(g, u, v, o)
    return g


def hand_built():
    """name -> (nx graph, nodes of the quotient, largest multiplicity)"""
    out = {}
    out['methane'] = (molecule([6], [], [4]), 2, 4)
    out['ethane'] = (molecule([6, 6], [(0, 1, 1)], [3, 3]), 4, 3)
    out['water'] = (molecule([8], [], [2]), 2, 2)
    out['ammonia'] = (molecule([7], [], [3]), 2, 3)
    out['methanol'] = (molecule([6, 8], [(0, 1, 1)], [3, 1]), 4, 3)
    h2 = nx.Graph()
    _atom(h2, 0, 1)
    _atom(h2, 1, 1)
    _bond(h2, 0, 1)
    out['h2'] = (h2, 2, 1)
    out['no_hydrogens'] = (molecule([6, 8, 6, 7], [(0, 1, 2), (0, 2, 1),
                                                   (2, 3, 3)], [0] * 4), 4, 1)
    # a carbon between a carbon and an oxygen, with two hydrogens that differ
    # in one node attribute: not twins
    odd = molecule([6, 6, 8], [(0, 1, 1), (1, 2, 1)], [0, 2, 0])
    odd.nodes[4]['charge'] = 1
    out['differing_hydrogens'] = (odd, 5, 1)
    # a self loop on one of two otherwise equal leaves: it has two adjacency
    # entries and is no leaf
    loop = molecule([6, 6], [(0, 1, 1)], [2, 0])
    _bond(loop, 3, 3)
    out['self_loop'] = (loop, 4, 1)
    return out


def weighted_pair():
    """Two weighted stars: leaf edges of equal weight (merged) and of
    different weights (not merged)."""
    gs = []
    for w in ((1.0, 1.0), (1.0, 0.5)):
        g = nx.Graph()
        for v in range(4):
            g.add_node(v, category=1 + int(v == 0))
        g.add_edge(0, 1, w=w[0], length=1.0)
        g.add_edge(0, 2, w=w[1], length=1.0)
        g.add_edge(0, 3, w=2.0, length=2.0)
        gs.append(Graph.from_networkx(g, weight='w'))
    return Graph.unify_datatype(gs)


def hand_graphs():
    """The nine unweighted hand-built molecules as graphs of one type (the
    weighted tenth case lives in a set of its own: `weighted_pair`)."""
    cases_ = hand_built()
    return list(cases_), Graph.unify_datatype(
        [Graph.from_networkx(g) for g, _, _ in cases_.values()])


@pytest.fixture(scope='module')
def hand():
    names, graphs = hand_graphs()
    return names, graphs, hand_built()


@pytest.mark.parametrize('real', [np.float32, np.float64])
def test_twin_groups_of_hand_built_graphs(hand, real):
    names, graphs, spec = hand
    for name, dg in zip(names, pack_many(graphs, real=real)):
        keep, mult = twin_groups(dg)
        _, n_q, m_max = spec[name]
        assert len(keep) == n_q, name
        assert mult.max() == m_max, name
        assert mult.sum() == dg.n_node, name
        q = quotient_graph(dg, native=False)
        assert (q.n_node, q.n_orig) == (n_q, dg.n_node), name
        assert np.array_equal(q.scale, np.sqrt(np.round(q.scale**2))), name
        # descending adjacency count of the quotient, degrees of the full graph
        assert np.all(np.diff(q.adjacency_count) <= 0), name
        full_degree = dict(zip(dg.perm.tolist(), dg.degree.tolist()))
        assert [full_degree[v] for v in q.perm.tolist()] == q.degree.tolist()
        # the nonzeros are those of the full graph between the nodes kept
        new_of = {int(v): k for k, v in enumerate(q.perm)}
        oi, oj = dg.perm[dg.nz['i']], dg.perm[dg.nz['j']]
        want = sorted((new_of[a], new_of[b]) for a, b in zip(oi, oj)
                      if a in new_of and b in new_of)
        assert want == list(zip(q.nz['i'].tolist(), q.nz['j'].tolist())), name


def test_weighted_leaves_merge_only_at_equal_weight():
    equal, different = pack_many(weighted_pair(), real=np.float64)
    q = quotient_graph(equal, native=False)
    assert (q.n_node, q.scale.max()) == (3, np.sqrt(2.0))
    q = quotient_graph(different, native=False)
    assert q.n_node == 4 and np.all(q.scale == 1)


@pytest.mark.parametrize('real', [np.float32, np.float64])
def test_native_quotient_is_the_numpy_one(hand, real):
    _, graphs, _ = hand
    sets = [graphs, weighted_pair(), cases.config3_graphs(30)]
    for gs in sets:
        for dg in pack_many(gs, real=real):
            a = quotient_graph(dg, native=True)
            b = quotient_graph(dg, native=False)
            assert a.offsets == b.offsets
            assert (a.n_node, a.n_nz, a.n_orig) == (b.n_node, b.n_nz, b.n_orig)
            assert a.image_bytes == b.image_bytes
            assert np.array_equal(a.blob, b.blob)


def test_header_keeps_its_fields_and_carries_the_full_node_count(hand):
    _, graphs, _ = hand
    dgs = pack_many(graphs, real=np.float64)
    qs = [quotient_graph(dg) for dg in dgs]
    arena = GraphArena(qs, classes=True)
    n_node = arena._hdr['n_node'].astype(np.int64)
    assert (n_node & 0xFFFF).tolist() == [q.n_node for q in qs]
    assert (n_node >> 16).tolist() == [dg.n_node for dg in dgs]
    assert arena.n_node.tolist() == [q.n_node for q in qs]
    full = GraphArena(dgs, classes=True)
    assert (full._hdr['n_node'] >> 16).tolist() == [0] * len(dgs)


def quotient_value(g1, g2, q1, q2, knode, kedge, q):
    """K of the pair from the rescaled quotient system, dense in float64:
    rows and columns of the representatives of the full matrix (the oracle's
    assembly), off-diagonal entries times s(I) s(J), the diagonal as it is,
    right-hand side and starting probability times s."""
    s1, s2 = oracle._side(g1), oracle._side(g2)
    V = oracle.node_table(knode, s1, s2)
    E = oracle.edge_table(kedge, s1, s2)
    A, Dx = oracle.assemble(s1, s2, V, E, q)
    K_full = np.linalg.solve(A, Dx).sum()
    rows = (q1.perm.astype(np.int64)[:, None] * s2.n
            + q2.perm.astype(np.int64)[None, :]).ravel()
    s = np.outer(q1.scale, q2.scale).ravel()
    Aq = A[np.ix_(rows, rows)] * np.outer(s, s)
    np.fill_diagonal(Aq, A[rows, rows])
    x = np.linalg.solve(Aq, s * Dx[rows])
    return K_full, float((s * x).sum())


def test_quotient_system_gives_the_value_of_the_full_one(hand):
    names, graphs, _ = hand
    knode, kedge, q = cases.config3_kernels()
    qs = [quotient_graph(dg) for dg in pack_many(graphs, real=np.float64)]
    assert sum(g.n_node for g in qs) < sum(len(g.nodes) for g in graphs)
    for a, b in itertools.combinations_with_replacement(range(len(graphs)), 2):
        full, quot = quotient_value(graphs[a], graphs[b], qs[a], qs[b],
                                    knode, kedge, q)
        assert quot == pytest.approx(full, rel=1e-12), (names[a], names[b])


def test_weighted_quotient_system_gives_the_value_of_the_full_one():
    graphs = weighted_pair()
    knode, kedge, q = cases.config2b_kernels()
    qs = [quotient_graph(dg) for dg in pack_many(graphs, real=np.float64)]
    for a, b in ((0, 0), (0, 1), (1, 1)):
        full, quot = quotient_value(graphs[a], graphs[b], qs[a], qs[b],
                                    knode, kedge, q)
        assert quot == pytest.approx(full, rel=1e-12)

