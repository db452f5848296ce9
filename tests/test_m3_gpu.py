"""M3 on the HIP backend: the fused double epilogue (mgk_oc.h, MAXIMIN == 2)
against the host composition on the same backend and against values recorded
from the reference."""
import numpy as np
import pytest
from test_m3 import GOLDEN, atoms, Atoms

pytestmark = pytest.mark.gpu


class Spy:
    """Counts the backend's fused M3 launches and the ones it declined."""

    def __init__(self, backend):
        from graphdot_amd.kernel.marginalized._backend_hip import \
            NotOwnerComputes
        self.fused, self.declined = 0, 0
        inner = backend.m3_distance

        def wrapped(*args, **kwargs):
            try:
                out = inner(*args, **kwargs)
            except NotOwnerComputes:
                self.declined += 1
                raise
            self.fused += 1
            return out
        backend.m3_distance = wrapped


def _m3(**kw):
    from graphdot_amd.experimental.metric import M3
    m = M3(**kw)
    spy = Spy(m.kernel.backend)
    return m, spy


def _composition(m, X, Y=None):
    GX, GY, _ = m._graphs(X, Y)
    return m._composition(GX, GY)


def test_backend_is_double():
    m, _ = _m3()
    assert np.dtype(m.kernel.backend.real) == np.float64


def test_fused_matches_golden_and_composition():
    for charge in (False, True):
        cases = [c for c in GOLDEN['m3'] if c['use_charge'] == charge]
        m, spy = _m3(use_charge=charge)
        for c in cases:
            a = atoms(c['a'])
            b = a if c['a'] == c['b'] else atoms(c['b'])
            d = m(a, b)
            assert d == pytest.approx(c['tight'], abs=1e-5)
            assert d == pytest.approx(c['shipped'], abs=1e-4)
            D = _composition(m, [a], [b] if b is not a else None)
            assert d == pytest.approx(D[0, 0], abs=1e-6)
        assert spy.fused == len(cases) and spy.declined == 0


def test_self_distance_zero_on_fused_path():
    """The reference's test_m3 / test_m3_charge on methane, fused."""
    a = atoms('CH4')
    for charge in (False, True):
        m, spy = _m3(use_charge=charge)
        assert m(a, a) <= 1e-7
        assert spy.fused == 1
    s = GOLDEN['structures']['CH4']
    p = np.array(s['positions'])
    p[1] += [0.05, -0.02, 0.03]
    m, _ = _m3()
    assert m(a, Atoms(s['numbers'], p)) > 1e-7


def test_pairwise_symmetric_and_cross():
    names = ['CH4', 'H2O', 'CH5NOS', 'C2H6O', 'NaCl', 'slab', 'NH4+']
    X = [atoms(n) for n in names]
    m, spy = _m3()
    D = m.pairwise(X)
    assert spy.fused == 1
    assert np.all(np.diagonal(D) <= 1e-7)
    assert np.array_equal(D, D.T)
    assert np.allclose(D, _composition(m, X), atol=1e-6, rtol=0)
    # 1 x N and N x 1 (LDS capacity of the reduction cells), periodic items
    for A, B in (([X[1]], X), (X, [X[4]]), ([X[4]], [X[0]])):
        DC = m.pairwise(A, B)
        assert DC.shape == (len(A), len(B))
        assert np.allclose(DC, _composition(m, A, B), atol=1e-6, rtol=0)
    # element by element
    for i in range(len(X)):
        for j in range(len(X)):
            assert D[i, j] == pytest.approx(m(X[i], X[j]), abs=1e-6)


def test_tang2019_batch():
    import cases
    G = cases.tang2019_graphs(72, seed=5)
    m, spy = _m3()
    D = m.pairwise(G)
    assert spy.fused == 1 and spy.declined == 0
    assert D.shape == (72, 72)
    assert np.all(np.diagonal(D) <= 1e-7)
    assert np.allclose(D, _composition(m, G), atol=1e-6, rtol=0)
    DC = m.pairwise(G[:5], G[5:])
    assert np.allclose(DC, D[:5, 5:], atol=1e-6, rtol=0)


def test_large_graphs_take_the_composition():
    import cases
    P = cases.protein_like_graphs(n_graphs=2, nmin=150, nmax=200, seed=7)
    T = cases.tang2019_graphs(2, seed=9)
    m, spy = _m3()
    D = m.pairwise(P + T)
    assert spy.declined == 1 and spy.fused == 0
    # (the host normalisation is not bitwise symmetric: (r_i k_ij) r_j)
    assert np.all(np.isfinite(D)) and np.allclose(D, D.T, atol=1e-12, rtol=0)
    assert np.all(np.diagonal(D) <= 1e-6)
    # the small pairs agree with their fused evaluation
    m2, spy2 = _m3()
    assert np.allclose(m2.pairwise(T), D[2:, 2:], atol=1e-6, rtol=0)
    assert spy2.fused == 1
