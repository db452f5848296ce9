#!/usr/bin/env python
"""Golden vectors that pin Graph.from_ase, the adjacency rules and the M3
metric to the reference.  Runs only where the reference tree exists.

The reference's own `Graph.from_ase`, `AtomicAdjacency`, `Tent`, `Gaussian`,
`CompactBell` and `M3` run under the shims of make_golden.py, with

* a stand-in atoms class that exposes exactly the members the importer here
  reads (len, get_atomic_numbers, get_positions, pbc, cell,
  get_initial_charges, get_chemical_formula) plus the ``atoms[i].number`` the
  reference's importer uses;
* mendeleev's `fetch_table` returning this package's shipped van der Waals
  radii, so that both sides read the same table.

M3 is recorded twice: with the reference's CG as shipped (atol 1e-7, scipy's
default rtol) and with the CG tightened to rtol 1e-13 as the other generators
do.  Writes m3.json.
"""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402


class Atom:
    def __init__(self, number):
        self.number = number


class Atoms:
    """Numbers, positions, cell, pbc and charges; nothing else."""

    def __init__(self, numbers, positions, cell=None, pbc=False,
                 charges=None, formula=None):
        self.numbers = np.asarray(numbers, dtype=np.int64)
        self.positions = np.asarray(positions, dtype=np.float64)
        self.cell = np.zeros((3, 3)) if cell is None else np.asarray(
            cell, dtype=np.float64)
        self.pbc = np.broadcast_to(np.asarray(pbc, dtype=bool), 3).copy()
        self.charges = np.zeros(len(self.numbers)) if charges is None \
            else np.asarray(charges, dtype=np.float64)
        self.formula = formula

    def __len__(self):
        return len(self.numbers)

    def __getitem__(self, i):
        return Atom(int(self.numbers[i]))

    def get_atomic_numbers(self):
        return self.numbers.copy()

    def get_positions(self):
        return self.positions.copy()

    def get_initial_charges(self):
        return self.charges.copy()

    def get_chemical_formula(self):
        return self.formula


def structures():
    """name -> dict(numbers, positions, cell, pbc, charges, formula)."""
    rng = np.random.RandomState(2024)
    out = {}
    # methane, hand-typed (the reference's test_m3 fixture geometry)
    out['CH4'] = dict(
        numbers=[6, 1, 1, 1, 1],
        positions=[[0.0, 0.0, 0.0], [0.629118, 0.629118, 0.629118],
                   [-0.629118, -0.629118, 0.629118],
                   [0.629118, -0.629118, -0.629118],
                   [-0.629118, 0.629118, -0.629118]],
        formula='CH4')
    out['H2O'] = dict(
        numbers=[8, 1, 1],
        positions=[[0.0, 0.0, 0.119262], [0.0, 0.763239, -0.477047],
                   [0.0, -0.763239, -0.477047]],
        formula='H2O')
    # methanethiol-like, with an amine and an alcohol group: C, H, N, O, S
    out['CH5NOS'] = dict(
        numbers=[6, 16, 7, 8, 1, 1, 1, 1, 1],
        positions=[[0.0, 0.0, 0.0], [1.82, 0.0, 0.0], [-0.5, 1.35, 0.0],
                   [-0.48, -0.70, 1.15], [-0.36, -0.52, -0.89],
                   [2.10, 1.32, 0.0], [-1.51, 1.38, 0.05],
                   [-0.18, 1.86, 0.82], [-1.44, -0.73, 1.14]],
        formula='CH5NOS')
    # ethanol-like with random jitter: a less symmetric molecule
    base = np.array([[0.0, 0.0, 0.0], [1.52, 0.0, 0.0], [2.0, 1.35, 0.0],
                     [-0.38, -1.02, 0.0], [-0.38, 0.51, 0.89],
                     [-0.38, 0.51, -0.89], [1.9, -0.51, 0.89],
                     [1.9, -0.51, -0.89], [2.95, 1.30, 0.0]])
    out['C2H6O'] = dict(
        numbers=[6, 6, 8, 1, 1, 1, 1, 1, 1],
        positions=(base + 0.05 * rng.normal(size=base.shape)).tolist(),
        formula='C2H6O')
    # rocksalt-like periodic cell (conventional, 8 atoms, a = 5.64 A)
    a = 5.64
    na = [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]]
    cl = [[.5, .5, .5], [.5, 0, 0], [0, .5, 0], [0, 0, .5]]
    out['NaCl'] = dict(
        numbers=[11] * 4 + [17] * 4,
        positions=(a * np.array(na + cl)).tolist(),
        cell=(a * np.eye(3)).tolist(), pbc=True, formula='Cl4Na4')
    # a slab: periodic along x and y only
    out['slab'] = dict(
        numbers=[6, 6, 1, 1],
        positions=[[0.0, 0.0, 0.0], [1.4, 0.0, 0.0], [0.0, 1.0, 0.0],
                   [1.4, 1.0, 0.0]],
        cell=[[2.8, 0, 0], [0, 2.0, 0], [0, 0, 10.0]],
        pbc=[True, True, False], formula='C2H2')
    # charged species
    out['OH-'] = dict(numbers=[8, 1], positions=[[0, 0, 0], [0, 0, 0.97]],
                      charges=[-1.2, 0.2], formula='HO')
    out['NH4+'] = dict(
        numbers=[7, 1, 1, 1, 1],
        positions=[[0.0, 0.0, 0.0], [0.59, 0.59, 0.59],
                   [-0.59, -0.59, 0.59], [0.59, -0.59, -0.59],
                   [-0.59, 0.59, -0.59]],
        charges=[-0.4, 0.35, 0.35, 0.35, 0.35], formula='H4N')
    return out


def make(spec):
    return Atoms(spec['numbers'], spec['positions'], spec.get('cell'),
                 spec.get('pbc', False), spec.get('charges'),
                 spec.get('formula'))


class ElementTable:
    """What the reference reads of mendeleev's element table: the
    `atomic_number` attribute and column access by name."""

    def __init__(self, columns):
        self.columns = columns
        self.atomic_number = columns['atomic_number']

    def __getitem__(self, name):
        return self.columns[name]


def main():
    import scipy.sparse.linalg as spla
    shipped_cg = spla.cg
    mg.install_shims()
    sys.path.insert(0, mg.REF)
    sys.path.insert(1, ROOT)
    from graphdot_amd.graph.adjacency.atomic import VDW_RADIUS_PM

    z = np.arange(1, 119)
    table = ElementTable({
        'atomic_number': z,
        'vdw_radius': np.array([VDW_RADIUS_PM.get(int(k), np.nan)
                                for k in z], dtype=np.float64),
    })
    sys.modules['mendeleev.fetch'].fetch_table = lambda *a, **k: table

    from graphdot import Graph
    from graphdot.graph.adjacency.atomic import AtomicAdjacency
    from graphdot.graph.adjacency.euclidean import (
        Tent, Gaussian, CompactBell)
    from graphdot.experimental.metric.m3 import M3

    S = structures()
    out = dict(structures=S)

    # -- shapes and adjacency --------------------------------------------------
    d = np.linspace(0.0, 7.0, 29)
    shapes = {}
    for name, f in (('tent1', Tent(1)), ('tent2', Tent(2)),
                    ('gaussian', Gaussian()),
                    ('compactbell4,2', CompactBell(4, 2)),
                    ('compactbell5,3', CompactBell(5, 3))):
        shapes[name] = dict(
            d=d.tolist(), length_scale=1.3,
            w=[float(f(x, 1.3)) for x in d],
            cutoff=float(f.cutoff(1.3)))
    out['shapes'] = shapes
    adj = {}
    pairs = [(1, 1), (1, 6), (6, 8), (7, 16), (11, 17), (8, 8)]
    for key, kw in (('tent1', dict(shape='tent1')),
                    ('tent2_zoom', dict(shape='tent2', zoom=0.75)),
                    ('gaussian', dict(shape='gaussian')),
                    ('compactbell4,2', dict(shape='compactbell4,2')),
                    ('tent1_numeric', dict(shape='tent1', length_scale=1.1))):
        A = AtomicAdjacency(**kw)
        rows = []
        for n1, n2 in pairs:
            for r in (0.5, 1.0, 2.0, 3.5, 5.0):
                rows.append([n1, n2, r, float(A(n1, n2, r))])
        adj[key] = dict(kwargs=kw, rows=rows,
                        cutoff_CHNOS=float(A.cutoff(np.array([1, 6, 7, 8, 16]))),
                        cutoff_NaCl=float(A.cutoff(np.array([11, 17]))))
    out['adjacency'] = adj

    # -- graphs --------------------------------------------------------------------
    graphs = {}
    variants = [
        ('default', {}, S.keys()),
        ('tent2_zoom', dict(adjacency=AtomicAdjacency(shape='tent2',
                                                      zoom=0.75)), S.keys()),
        ('gaussian_numeric', dict(adjacency=AtomicAdjacency(
            shape='gaussian', length_scale=0.6)), ['CH4', 'H2O', 'OH-']),
        ('compactbell', dict(adjacency=AtomicAdjacency(
            shape='compactbell4,2')), ['CH5NOS', 'NaCl']),
        ('nopbc', dict(use_pbc=False), ['NaCl', 'slab']),
        ('charge', dict(use_charge=True), ['OH-', 'NH4+', 'H2O']),
    ]
    for vname, kw, names in variants:
        for name in names:
            g = Graph.from_ase(make(S[name]), **kw)
            e = g.edges
            order = np.lexsort((np.asarray(e['!j']), np.asarray(e['!i'])))
            rec = dict(
                title=g.title,
                node_dtypes={c: str(np.asarray(g.nodes[c]).dtype)
                             for c in g.nodes.columns},
                edge_dtypes={c: str(np.asarray(e[c]).dtype)
                             for c in e.columns},
                nodes={c: np.asarray(g.nodes[c]).tolist()
                       for c in g.nodes.columns},
                edges={c: np.asarray(e[c])[order].tolist()
                       for c in e.columns})
            graphs[f'{vname}/{name}'] = rec
    out['graphs'] = graphs

    # -- M3 ------------------------------------------------------------------------
    tight_cg = spla.cg
    mpairs = [('CH4', 'CH4'), ('CH4', 'H2O'), ('CH4', 'CH5NOS'),
              ('H2O', 'C2H6O'), ('CH5NOS', 'C2H6O'), ('C2H6O', 'C2H6O'),
              ('NaCl', 'NaCl'), ('NaCl', 'CH4')]
    cpairs = [('OH-', 'NH4+'), ('H2O', 'OH-'), ('NH4+', 'NH4+')]
    m3 = []
    for charge, plist in ((False, mpairs), (True, cpairs)):
        for a, b in plist:
            rec = dict(a=a, b=b, use_charge=charge)
            for key, cg in (('tight', tight_cg), ('shipped', shipped_cg)):
                spla.cg = cg
                A = make(S[a])
                B = A if a == b else make(S[b])
                rec[key] = float(M3(use_charge=charge)(A, B))
            spla.cg = tight_cg
            m3.append(rec)
    out['m3'] = m3

    with open(os.path.join(HERE, 'm3.json'), 'w') as f:
        json.dump(mg.jsonable(out), f)


if __name__ == '__main__':
    main()
