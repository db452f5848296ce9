"""Graph.from_ase, the adjacency rules and the M3 metric against values
recorded from the reference (golden/m3.json, make_golden_m3.py), on the CPU:
M3's nodal similarities come from the dense fp64 oracle here."""
import json
import os
import numpy as np
import pytest
from graphdot_amd.graph import Graph
from graphdot_amd.graph.adjacency import (AtomicAdjacency, Tent, Gaussian,
                                          CompactBell)
from graphdot_amd.graph._from_ase import hill_formula
from graphdot_amd.experimental.metric import M3
from graphdot_amd.experimental.metric.m3 import m3_from_nodal

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), 'golden',
                                     'm3.json')))


class Atoms:
    """The members Graph.from_ase reads, and nothing else."""

    def __init__(self, numbers, positions, cell=None, pbc=False,
                 charges=None, formula=None):
        self._numbers = np.asarray(numbers, dtype=np.int64)
        self._positions = np.asarray(positions, dtype=np.float64)
        self.cell = np.zeros((3, 3)) if cell is None else np.asarray(
            cell, dtype=np.float64)
        self.pbc = np.broadcast_to(np.asarray(pbc, dtype=bool), 3).copy()
        self._charges = None if charges is None else np.asarray(charges)
        if formula is not None:
            self.get_chemical_formula = lambda: formula

    def __len__(self):
        return len(self._numbers)

    def get_atomic_numbers(self):
        return self._numbers.copy()

    def get_positions(self):
        return self._positions.copy()

    def get_initial_charges(self):
        return (np.zeros(len(self)) if self._charges is None
                else self._charges.copy())


def atoms(name, formula=True):
    s = GOLDEN['structures'][name]
    return Atoms(s['numbers'], s['positions'], s.get('cell'),
                 s.get('pbc', False), s.get('charges'),
                 s['formula'] if formula else None)


class OracleM3(M3):
    """M3 whose nodal similarities come from the dense fp64 oracle."""

    def _fused(self, GX, GY):
        return None

    def _nodal(self, GX, GY):
        from oracle import mgk
        kw = dict(q=self.q, nodal=True, mode='dense', tol=1e-14)
        K = mgk.gram(GX, self.node_kernel, self.edge_kernel, Y=GY, **kw)

        def diag(G):
            return np.concatenate([np.diagonal(mgk.gram(
                [g], self.node_kernel, self.edge_kernel, **kw)) for g in G])
        k1 = diag(GX)
        k2 = k1 if GY is None else diag(GY)
        return K, k1, k2


def _ulp32(a, b):
    a = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# -- adjacency rules ---------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(GOLDEN['shapes']))
def test_shapes_scalar_and_array(name):
    case = GOLDEN['shapes'][name]
    shape = AtomicAdjacency._parse_shape(name)
    d = np.array(case['d'])
    ls = case['length_scale']
    got = [shape(float(x), ls) for x in d]
    assert np.array_equal(got, case['w'])
    assert np.array_equal(shape(d, ls), case['w'])
    assert shape.cutoff(ls) == case['cutoff']


def test_shape_classes():
    assert isinstance(AtomicAdjacency._parse_shape('tent3'), Tent)
    assert isinstance(AtomicAdjacency._parse_shape('gaussian'), Gaussian)
    b = AtomicAdjacency._parse_shape('compactbell6,3')
    assert isinstance(b, CompactBell) and (b.a, b.b) == (6, 3)
    with pytest.raises(ValueError):
        AtomicAdjacency(shape='triangle')
    assert Tent(2)(10.0, 1.0) == 0


@pytest.mark.parametrize('key', sorted(GOLDEN['adjacency']))
def test_atomic_adjacency(key):
    case = GOLDEN['adjacency'][key]
    A = AtomicAdjacency(**case['kwargs'])
    rows = np.array(case['rows'])
    n1, n2 = rows[:, 0].astype(int), rows[:, 1].astype(int)
    for a, b, r, w in case['rows']:
        assert A(int(a), int(b), r) == w
    assert np.array_equal(A(n1, n2, rows[:, 2]), rows[:, 3])
    assert A.cutoff(np.array([1, 6, 7, 8, 16])) == case['cutoff_CHNOS']
    assert A.cutoff(np.array([11, 17])) == case['cutoff_NaCl']


def test_radii_table_matches_fixture_radii():
    from cases import _VDW
    A = AtomicAdjacency()
    assert A.ltable.shape == (119,)
    for z, r in _VDW.items():
        assert A.ltable[z] == pytest.approx(r, rel=1e-15)


def test_length_scale_forms_and_errors():
    base = AtomicAdjacency(shape='tent1')
    m = AtomicAdjacency(shape='tent1', length_scale={1: 1.1, 6: 1.7})
    arr = np.full(119, np.nan)
    arr[[1, 6]] = [1.1, 1.7]
    a = AtomicAdjacency(shape='tent1', length_scale=arr, zoom=2.0)
    for r in (0.4, 1.3, 3.9):
        assert m(1, 6, r) == pytest.approx(base(1, 6, r), rel=1e-14)
    assert a.cutoff([1, 6]) == pytest.approx(2 * base.cutoff([1, 6]))
    with pytest.raises(ValueError, match='Fe'):
        base.cutoff([6, 26])
    with pytest.raises(ValueError, match='Fe'):
        base(26, 6, 1.0)
    with pytest.raises(ValueError, match='N'):
        m(7, 6, 1.0)
    with pytest.raises(ValueError, match='covalent_radius_pyykko'):
        AtomicAdjacency(length_scale='covalent_radius_pyykko')


# -- importer ----------------------------------------------------------------------
def _variant_kwargs(vname):
    return {
        'default': {},
        'tent2_zoom': dict(adjacency=AtomicAdjacency(shape='tent2',
                                                     zoom=0.75)),
        'gaussian_numeric': dict(adjacency=AtomicAdjacency(
            shape='gaussian', length_scale=0.6)),
        'compactbell': dict(adjacency=AtomicAdjacency(
            shape='compactbell4,2')),
        'nopbc': dict(use_pbc=False),
        'charge': dict(use_charge=True),
    }[vname]


@pytest.mark.parametrize('key', sorted(GOLDEN['graphs']))
def test_from_ase_matches_reference(key):
    ref = GOLDEN['graphs'][key]
    vname, name = key.split('/')
    g = Graph.from_ase(atoms(name), **_variant_kwargs(vname))
    assert {c: str(np.asarray(g.nodes[c]).dtype)
            for c in g.nodes.columns} == ref['node_dtypes']
    assert {c: str(np.asarray(g.edges[c]).dtype)
            for c in g.edges.columns} == ref['edge_dtypes']
    for c, v in ref['nodes'].items():
        assert np.array_equal(np.asarray(g.nodes[c]), v)
    e = g.edges
    assert np.array_equal(np.asarray(e['!i']), ref['edges']['!i'])
    assert np.array_equal(np.asarray(e['!j']), ref['edges']['!j'])
    for c in ('!w', 'length'):
        assert _ulp32(e[c], ref['edges'][c]).max() <= 1
    prefix = ' '.join(ref['title'].split()[:2]) + ' '
    assert g.title.startswith(prefix)
    assert len(g.title) == len(ref['title'])


def test_from_ase_without_formula_method_uses_hill():
    g = Graph.from_ase(atoms('CH5NOS', formula=False))
    assert g.title.startswith('Molecule CH5NOS ')
    assert hill_formula([8, 1, 1]) == 'H2O'
    assert hill_formula([17, 11, 11, 17]) == 'Cl2Na2'
    assert hill_formula([6, 6, 1, 8]) == 'C2HO'


def test_from_ase_without_edges_raises():
    far = Atoms([1, 1], [[0, 0, 0], [0, 0, 50.0]])
    with pytest.raises(ValueError):
        Graph.from_ase(far)


def test_from_ase_kdtree_path_agrees(monkeypatch):
    import importlib
    _from_ase = importlib.import_module('graphdot_amd.graph._from_ase')
    a = atoms('NaCl')
    dense = Graph.from_ase(a)
    monkeypatch.setattr(_from_ase, '_DENSE_LIMIT', 0)
    tree = Graph.from_ase(a)
    for c in ('!i', '!j', '!w', 'length'):
        assert np.array_equal(np.asarray(dense.edges[c]),
                              np.asarray(tree.edges[c]))


# -- M3 ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', GOLDEN['m3'],
                         ids=lambda c: f"{c['a']}-{c['b']}-{c['use_charge']}")
def test_m3_vs_reference(case):
    m = OracleM3(use_charge=case['use_charge'])
    a = atoms(case['a'])
    b = a if case['a'] == case['b'] else atoms(case['b'])
    d = m(a, b)
    assert d == pytest.approx(case['tight'], abs=1e-5)
    assert d == pytest.approx(case['shipped'], abs=1e-4)


def test_m3_self_distance_is_zero_and_perturbation_is_not():
    """The reference's test_m3 / test_m3_charge on methane."""
    a = atoms('CH4')
    assert OracleM3()(a, a) <= 1e-7
    assert OracleM3(use_charge=True)(a, a) <= 1e-7
    s = GOLDEN['structures']['CH4']
    p = np.array(s['positions'])
    p[1] += [0.05, -0.02, 0.03]
    b = Atoms(s['numbers'], p)
    assert OracleM3()(a, b) > 1e-7


def test_pairwise_equals_calls():
    m = OracleM3()
    X = [atoms(n) for n in ('CH4', 'H2O', 'CH5NOS', 'C2H6O')]
    D = m.pairwise(X)
    assert D.shape == (4, 4)
    for i in range(4):
        for j in range(4):
            assert D[i, j] == pytest.approx(m(X[i], X[j]), abs=1e-12)
    Y = [atoms('NaCl'), X[1]]
    DY = m.pairwise(X, Y)
    assert DY.shape == (4, 2)
    for i in range(4):
        for j in range(2):
            assert DY[i, j] == pytest.approx(m(X[i], Y[j]), abs=1e-12)
    # graphs already built are taken as they are
    G = [Graph.from_ase(x, adjacency=m.adjacency) for x in X]
    assert np.allclose(m.pairwise(G), D, atol=1e-12, rtol=0)


def test_m3_from_nodal_uses_own_diagonal_for_self_pairs():
    K = np.array([[2.0, 0.5], [0.5, 1.0]])
    D = m3_from_nodal(K, [9.0, 9.0], [9.0, 9.0], [0, 2], [0, 2], True)
    assert D.shape == (1, 1) and D[0, 0] == 0.0


def test_default_adjacency():
    m = M3()
    assert isinstance(m.adjacency.shape, Tent) and m.adjacency.shape.ord == 2
    assert m.adjacency.ltable[6] == pytest.approx(1.7 * 0.75)
