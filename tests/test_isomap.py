"""KernelIsomap without a GPU: the definition of the model in numpy on the
stored matrix widened to double, the data, the ``*_torch`` restatements of
model/manifold/_geodesic.py on CPU tensors against the definition, the
definition against SciPy's shortest paths and scikit-learn's Isomap, the model's
interface, and the kernels' unit.  tests/test_isomap_gpu.py takes the
definition, the data and the bounds from here.

The bounds.  A geodesic is the minimum over the same paths of sums of at most
n - 1 non-negative terms, added in an order that differs between the
implementations: two of them differ by ``2 (n - 1) u G`` at the most, ``u =
2**-53`` (`path_bound`).  The embeddings are compared with scikit-learn's
within 100 times the difference that tests/golden/make_golden_isomap.py
recorded between the definition and scikit-learn (tests/golden/
isomap_bands.json): room for another eigensolver and the device's arithmetic.
Eigenvalues come from a backward-stable solver: ``16 n u |w_0|``."""
import functools
import json
import os
import warnings

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -53
#: (n, n_neighbors): below a wave; one tile; a tile plus one; two tiles plus
#: one (geo_fw_rest has four workgroups, one of them 1 x 1); an interior tile
SHAPES = [(5, 2), (64, 5), (65, 5), (129, 6), (200, 8)]
#: the seed of the points of each shape: its neighbourhood graph is connected
SEEDS = {5: 2, 64: 1, 65: 1, 129: 0, 200: 0}
#: components kept per shape: a clear gap behind the last one
COMPONENTS = {5: 2, 64: 2, 65: 2, 129: 3, 200: 3}
DTYPES = [np.float32, np.float64]
#: held-out samples of a case
N_NEW = 7


def _torch():
    import torch
    import graphdot_amd.model.manifold  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.array(a, order='C'))


# -- the data --------------------------------------------------------------------------
def points(n, seed):
    """n seeded random points of the unit cube, one of them twice."""
    P = np.random.RandomState(seed).rand(n, 3)
    P[n // 2] = P[1]
    return P


def gaussian(P, Q=None):
    Q = P if Q is None else Q
    return np.exp(-0.5 * ((P[:, None, :] - Q[None, :, :]) ** 2).sum(2))


# -- the definition --------------------------------------------------------------------
def define_lists(Ks, dq, dt, k, exclude_self=False):
    """(d2 (b, k), idx (b, k)): the k first columns of every row in the
    order (d2, column)."""
    d2 = np.maximum((dq[:, None] + dt[None, :])
                    - 2.0 * np.asarray(Ks, dtype=np.float64), 0.0)
    if exclude_self:
        d2 = d2.copy()
        np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind='stable')[:, :k]
    return np.take_along_axis(d2, idx, 1), idx


def define_graph(K, k):
    """(W, idx): the edge lengths of the neighbourhood graph of the stored
    matrix K and the lists they come from."""
    K = np.asarray(K, dtype=np.float64)
    n = len(K)
    d = np.diag(K).copy()
    D2 = np.maximum((d[:, None] + d[None, :]) - 2.0 * K, 0.0)
    _, idx = define_lists(K, d, d, k, exclude_self=True)
    E = np.zeros((n, n), dtype=bool)
    E[np.arange(n)[:, None], idx] = True
    E |= E.T
    W = np.where(E, np.sqrt(np.minimum(D2, D2.T)), np.inf)
    np.fill_diagonal(W, 0.0)
    return W, idx


def define_paths(W):
    """All-pairs shortest paths: the n steps of Floyd and Warshall."""
    G = W.copy()
    for m in range(len(G)):
        G = np.minimum(G, G[:, m:m + 1] + G[m:m + 1, :])
    return G


def blocked_paths(W, T=64):
    """The same in the order of the device: R rounds of the pivot tile, the
    tiles of its row and column, and the min-plus products of the rest, on
    the matrix padded with inf to whole tiles."""
    n = len(W)
    R = -(-n // T)
    G = np.full((R * T, R * T), np.inf)
    G[:n, :n] = W

    def tile(i, j):
        return G[i * T:(i + 1) * T, j * T:(j + 1) * T]
    for p in range(R):
        X = tile(p, p)
        for m in range(T):
            X[...] = np.minimum(X, X[:, m:m + 1] + X[m:m + 1, :])
        for t in range(R):
            if t == p:
                continue
            X = tile(p, t)
            for m in range(T):
                X[...] = np.minimum(X, tile(p, p)[:, m:m + 1] + X[m:m + 1, :])
            X = tile(t, p)
            for m in range(T):
                X[...] = np.minimum(X, X[:, m:m + 1] + tile(p, p)[m:m + 1, :])
        for i in range(R):
            for j in range(R):
                if i == p or j == p:
                    continue
                A, B = tile(i, p), tile(p, j)
                tile(i, j)[...] = np.minimum(
                    tile(i, j), (A[:, :, None] + B[None, :, :]).min(1))
    return G[:n, :n].copy()


def path_bound(n, G):
    return 2.0 * (n - 1) * U * G


def close_paths(got, G, n=None):
    """Whether `got` is within the path bound of the finite G, inf where G
    is (n: the most vertices of a path, the rows of G unless given)."""
    n = len(G) if n is None else n
    fin = np.isfinite(G)
    return bool(np.array_equal(np.isfinite(got), fin) and
                (np.abs(got[fin] - G[fin]) <= path_bound(n, G[fin])).all())


def centre(B):
    return B - B.mean(0)[None, :] - B.mean(1)[:, None] + B.mean()


def define_embedding(G, c):
    """(eigenvalues (c,), eigenvectors (n, c) signed as KernelPCA signs
    them, |H B H|_F^2, B)"""
    B = -0.5 * (G * G)
    Bc = centre(B)
    w, V = np.linalg.eigh(0.5 * (Bc + Bc.T))
    w, V = w[::-1][:c].copy(), V[:, ::-1][:, :c].copy()
    lead = np.argmax(np.abs(V), axis=0)
    V = V * np.where(V[lead, np.arange(c)] < 0, -1.0, 1.0)
    return w, V, float((Bc * Bc).sum()), B


def define_extension(Kq, dq, d, k, G):
    """Gq (b, n) of new samples with the cross matrix Kq."""
    d2, idx = define_lists(Kq, dq, d, k)
    return (np.sqrt(d2)[:, :, None] + G[idx]).min(1)


def define_transform(Gq, B, w, V):
    Bq = -0.5 * (Gq * Gq)
    Bqc = Bq - Bq.mean(1)[:, None] - B.mean(0)[None, :] + B.mean()
    return Bqc @ (V / np.sqrt(w))


def define_error(norm2, w, n):
    return np.sqrt(norm2 - (w ** 2).sum()) / n


class Case:
    """Everything the tests of one (n, k, storage) share, computed once and
    left unchanged."""

    def __init__(self, n, k, dtype):
        self.n, self.k, self.c = n, k, COMPONENTS[n]
        P = points(n, SEEDS[n])
        Q = np.random.RandomState(SEEDS[n] + 1000).rand(N_NEW, 3)
        Q[0] = P[2]                               # (a training sample again)
        self.K = gaussian(P).astype(dtype)
        self.Kq = gaussian(Q, P).astype(dtype)
        self.dq = np.ones(N_NEW)
        self.d = np.diag(self.K).astype(np.float64)
        self.W, self.idx = define_graph(self.K, k)
        self.G = define_paths(self.W)
        self.w, self.V, self.norm2, self.B = define_embedding(self.G, self.c)
        self.Y = self.V * np.sqrt(self.w)
        self.Gq = define_extension(self.Kq, self.dq, self.d, k, self.G)
        self.Yq = define_transform(self.Gq, self.B, self.w, self.V)
        self.error = define_error(self.norm2, self.w, n)
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(n, k, dtype):
    return Case(n, k, dtype)


def close_edges(got, W):
    """Whether `got` has the edges of W, each within an ulp (torch's square
    root on a CPU is not rounded correctly; numpy's and the device's are)."""
    fin = np.isfinite(W)
    return bool(np.array_equal(np.isfinite(got), fin)
                and np.array_equal(got, got.T)
                and (np.abs(got[fin] - W[fin]) <= 2 * U * W[fin]).all())


def align(Y, ref):
    """Y with every column signed as that of `ref`."""
    return Y * np.where((Y * ref).sum(0) < 0, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def bands():
    with open(os.path.join(GOLDEN, 'isomap_bands.json')) as f:
        return json.load(f)['cases']


def band(n, k, what):
    """100 times what the golden file recorded for the double case."""
    return 100.0 * bands()[f'{n}-{k}'][what]


def error_bound(c):
    """On n^2 times the squared reconstruction error: it is a difference of
    sums of n^2 squares of the size of |B|_F^2, each sum within n u of its
    value whatever its order, and the model forms |H B H|_F^2 from three
    such."""
    return 8.0 * c.n * U * float((c.B * c.B).sum())


def check_model(model, c, factor=1.0):
    """The fitted `model` against the definition of the case."""
    n = c.n
    assert model.n_components_ == c.c
    assert np.abs(model.eigenvalues_ - c.w).max() <= 16 * n * U * c.w[0]
    assert close_paths(model.dist_matrix_, c.G)
    assert np.array_equal(model.dist_matrix_, model.dist_matrix_.T)
    Y = model.embedding_
    assert Y.shape == (n, c.c) and Y.dtype == np.float64
    worst = np.abs(align(Y, c.Y) - c.Y).max()
    assert worst <= factor * band(n, c.k, 'embedding'), worst
    got = (model.reconstruction_error() * n) ** 2
    assert abs(got - (c.error * n) ** 2) <= error_bound(c)
    return worst


# -- 1. the data -----------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_neighbourhood_graphs_are_connected(n, k, dtype):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    c = case(n, k, dtype)
    A = csr_matrix(np.isfinite(c.W) & ~np.eye(n, dtype=bool))
    assert connected_components(A, directed=False)[0] == 1
    assert np.isfinite(c.G).all()
    # a duplicated sample: an edge of length 0
    assert c.W[1, n // 2] == 0.0 and c.G[1, n // 2] == 0.0
    # a clear gap behind the last component kept
    w = np.linalg.eigvalsh(centre(c.B))[::-1]
    assert w[c.c] < 0.7 * w[c.c - 1] and w[c.c - 1] > 0


# -- 2. the geodesics ------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_definition_against_scipy(n, k, dtype):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    c = case(n, k, dtype)
    W = np.where(np.isfinite(c.W), c.W, 0.0)
    # (explicit zeros are edges of length 0 for a csr matrix built from its
    # coordinates: the duplicate's)
    i, j = np.nonzero(np.isfinite(c.W) & ~np.eye(n, dtype=bool))
    A = csr_matrix((W[i, j], (i, j)), shape=(n, n))
    ref = shortest_path(A, method='D', directed=False)
    assert close_paths(c.G, ref)
    assert np.array_equal(c.G, c.G.T)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_blocked_order_against_the_plain_one(n, k, dtype):
    c = case(n, k, dtype)
    G = blocked_paths(c.W)
    assert close_paths(G, c.G)
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_twins_against_the_definition(n, k, dtype):
    torch = _torch()
    from graphdot_amd.model.manifold import _geodesic
    c = case(n, k, dtype)
    for K in (_t(c.K), _t(c.K).t().contiguous().t()):
        W = _geodesic.graph_torch(K, _t(c.d), _t(c.idx))
        assert close_edges(W.numpy(), c.W)
    G = _geodesic.shortest_paths_torch(W)
    assert close_paths(G.numpy(), c.G)
    assert torch.equal(G, G.T)
    B, label, count = _geodesic.finish_torch(G)
    assert np.array_equal(B.numpy(), -0.5 * (G.numpy() * G.numpy()))
    assert int(count.sum()) == 1 and not label.any()
    d2, idx = define_lists(c.Kq, c.dq, c.d, k)
    Bq, Gq = _geodesic.extend_torch(_t(d2), _t(idx), _t(c.G), True)
    # (one square root within an ulp and one sum)
    assert (np.abs(Gq.numpy() - c.Gq) <= 4 * U * c.Gq).all()
    assert np.array_equal(Bq.numpy(), -0.5 * (Gq.numpy() * Gq.numpy()))
    assert _geodesic.extend_torch(_t(d2), _t(idx), _t(c.G))[1] is None


def test_an_asymmetric_matrix_gives_a_symmetric_graph():
    from graphdot_amd.model.manifold import _geodesic
    c = case(65, 5, np.float64)
    K = np.array(c.K)
    r = np.random.RandomState(3)
    K += 1e-3 * r.rand(*K.shape) * ~np.eye(65, dtype=bool)
    assert not np.array_equal(K, K.T)
    W, idx = define_graph(K, 5)
    assert np.array_equal(W, W.T)
    got = _geodesic.graph_torch(_t(K), _t(np.diag(K).copy()), _t(idx))
    assert close_edges(got.numpy(), W)


def test_device_lists_is_the_search():
    torch = _torch()
    from graphdot_amd.model.neighbors import _knn, device_lists
    c = case(65, 5, np.float32)
    K, d = _t(c.K), _t(c.d)
    for kw in ({}, {'exclude_self': True}):
        (d2, idx, flag), fused = device_lists(K, d, d, 5, **kw)
        (r2, ridx, rflag), rfused = _knn.search(K, d, d, 5, **kw)
        assert fused is rfused is False
        assert torch.equal(d2, r2) and torch.equal(idx, ridx)
        assert torch.equal(flag, rflag) and int(flag) == 0
    assert np.array_equal(idx.numpy(), c.idx)


# -- 3. the definition and the model against scikit-learn --------------------------------
def sklearn_isomap(c):
    from sklearn.manifold import Isomap
    D = np.sqrt(np.maximum((c.d[:, None] + c.d[None, :])
                           - 2.0 * c.K.astype(np.float64), 0.0))
    m = Isomap(n_neighbors=c.k, n_components=c.c, metric='precomputed',
               eigen_solver='dense')
    Y = m.fit_transform(D)
    Dq = np.sqrt(np.maximum((c.dq[:, None] + c.d[None, :])
                            - 2.0 * c.Kq.astype(np.float64), 0.0))
    return m, Y, m.transform(Dq)


def sklearn_differences(c):
    """How far the definition of the case is from scikit-learn's Isomap on
    this machine: what the golden file records."""
    m, Y, Yq = sklearn_isomap(c)
    sign = np.where((Y * c.Y).sum(0) < 0, -1.0, 1.0)
    return {'paths': bool(close_paths(m.dist_matrix_, c.G)),
            'embedding': float(np.abs(Y * sign - c.Y).max()),
            'transform': float(np.abs(Yq * sign - c.Yq).max()),
            'reconstruction_error': float(m.reconstruction_error()),
            'scale': float(np.abs(c.Y).max())}


@pytest.mark.parametrize('n, k', SHAPES)
def test_model_against_scikit_learn(n, k):
    from graphdot_amd.model.manifold import KernelIsomap
    c = case(n, k, np.float64)
    m, Y, Yq = sklearn_isomap(c)
    model = KernelIsomap('precomputed', k, c.c, device='cpu').fit(
        np.array(c.K))
    assert model.last_timing['fused'] is False
    assert model.last_timing['adopted'] is False
    assert close_paths(model.dist_matrix_, m.dist_matrix_)
    sign = np.where((Y * model.embedding_).sum(0) < 0, -1.0, 1.0)
    worst = np.abs(Y * sign - model.embedding_).max()
    assert worst <= band(n, k, 'embedding'), worst
    got = model.transform(np.array(c.Kq), diag=c.dq)
    worst_q = np.abs(Yq * sign - got).max()
    assert worst_q <= band(n, k, 'transform'), worst_q
    assert abs((model.reconstruction_error() * n) ** 2
               - (m.reconstruction_error() * n) ** 2) <= error_bound(c)
    # ... and the recorded run of scikit-learn said the same of the definition
    rec = bands()[f'{n}-{k}']
    assert rec['paths'] is True
    assert rec['embedding'] <= 1e-12 * rec['scale']
    assert abs((rec['reconstruction_error'] * n) ** 2
               - (c.error * n) ** 2) <= error_bound(c)
    print(f'n = {n}: embedding within {worst:.1e}, transform within '
          f'{worst_q:.1e} of scikit-learn')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_model_against_the_definition(n, k, dtype):
    from graphdot_amd.model.manifold import KernelIsomap
    c = case(n, k, dtype)
    K = _t(c.K)
    bits = np.array(c.K).tobytes()
    model = KernelIsomap('precomputed', k, c.c, device='cpu')
    Y = model.fit_transform(K if n % 2 else np.array(c.K))
    assert Y is model.embedding_
    check_model(model, c)
    assert K.numpy().tobytes() == bits and c.K.tobytes() == bits
    # held-out rows: the definition, column signs as the training map's
    sign = np.where((Y * c.Y).sum(0) < 0, -1.0, 1.0)
    Gq = model.geodesic_distances(np.array(c.Kq), diag=c.dq)
    assert Gq.dtype == np.float64 and close_paths(Gq, c.Gq, n + 1)
    Yq = model.transform(_t(c.Kq), diag=_t(c.dq))
    assert Yq.shape == (N_NEW, c.c)
    worst = np.abs(Yq * sign - c.Yq).max()
    assert worst <= band(n, k, 'transform'), worst
    # a training sample is its own nearest neighbour at distance 0: its
    # geodesics are its row of G, up to the rounding of a detour through
    # another neighbour (its coordinates are *not* its row of the embedding:
    # the projection differs by the discarded spectrum)
    assert close_paths(Gq[:1], c.G[2:3], n + 1)
    assert set(model.last_timing) == {'kernel', 'paths', 'linalg', 'adopted',
                                      'fused'}


# -- 4. the ring -----------------------------------------------------------------------
def ring():
    a = 2.0 * np.pi * np.arange(96) / 96
    P = np.column_stack((np.cos(a), np.sin(a)))
    return P @ P.T + 1.0


def pairwise(Y):
    return np.sqrt(((Y[:, None, :] - Y[None, :, :]) ** 2).sum(2))


def test_the_ring_needs_the_algebraically_largest_eigenvalues():
    """H B H of a ring is indefinite, and its most negative eigenvalue is
    larger in magnitude than the third and fourth largest: the eigenvalues
    of largest magnitude are not the ones Isomap keeps."""
    from graphdot_amd.model.manifold import KernelIsomap
    K = ring()
    n = 96
    W, _ = define_graph(K, 2)
    assert (np.isfinite(W).sum(1) == 3).all()
    G = define_paths(W)
    w, V, _, B = define_embedding(G, 4)
    every = np.linalg.eigvalsh(centre(B))
    assert w[0] == pytest.approx(96.0, rel=1e-3)
    assert w[2] == pytest.approx(10.697, rel=1e-4)
    assert every[0] == pytest.approx(-24.03, rel=1e-3) and -every[0] > w[2]
    gap = w[3] - every[-5]
    assert gap > 5.0
    model = KernelIsomap('precomputed', 2, 4, device='cpu').fit(K)
    assert (model.eigenvalues_ > 0).all() and model.n_components_ == 4
    assert np.abs(model.eigenvalues_ - w).max() <= 16 * n * U * w[0]
    # the eigenvalues come in pairs: the distances of the map are what the
    # pairs agree on, whichever basis a solver picks in each plane.  The
    # planes turn by n u |w_0| / gap at the most under a backward-stable
    # solver; the map has the size of its diameter
    ref = pairwise(V * np.sqrt(w))
    tol = 64 * n * U * w[0] / gap * ref.max()
    assert np.abs(pairwise(model.embedding_) - ref).max() <= tol


# -- 5. a graph that is not connected ----------------------------------------------------
def clusters():
    r = np.random.RandomState(5)
    P = np.vstack((r.rand(10, 3), r.rand(7, 3) + 100.0))
    return gaussian(P)


def test_a_graph_that_is_not_connected_is_an_error():
    from graphdot_amd.model.manifold import KernelIsomap, _geodesic
    K = clusters()
    with pytest.raises(ValueError, match=r'2 components of sizes \[10, 7\].*'
                                         'larger n_neighbors'):
        KernelIsomap('precomputed', 3, 2, device='cpu').fit(K)
    W, idx = define_graph(K, 3)
    G = _geodesic.shortest_paths_torch(
        _geodesic.graph_torch(_t(K), _t(np.diag(K).copy()), _t(idx)))
    assert not G.isnan().any()
    assert np.array_equal(np.isinf(G.numpy()),
                          np.arange(17)[:, None] // 10
                          != np.arange(17)[None, :] // 10)
    B, label, count = _geodesic.finish_torch(G)
    assert int(count.sum()) == 2
    assert label.tolist() == [0] * 10 + [10] * 7
    assert _geodesic.component_sizes(label.numpy()) == [10, 7]
    # scikit-learn's meaning, which this model declines: it goes on
    KernelIsomap('precomputed', 10, 2, device='cpu').fit(K)


# -- 6. the interface --------------------------------------------------------------------
def test_errors():
    from graphdot_amd.model.manifold import KernelIsomap
    K = np.array(case(5, 2, np.float64).K)
    for k in (0, 1.5, True, -1):
        with pytest.raises(ValueError, match='n_neighbors'):
            KernelIsomap('precomputed', n_neighbors=k)
    for c in (0, 17, 2.5):
        with pytest.raises(ValueError, match='n_components'):
            KernelIsomap('precomputed', n_components=c)
    with pytest.raises(ValueError, match='n_neighbors = 5 with 5 samples'):
        KernelIsomap('precomputed', 5, 2, device='cpu').fit(K)
    with pytest.raises(ValueError, match='n_components = 5 with 5 samples'):
        KernelIsomap('precomputed', 2, 5, device='cpu').fit(K)
    KernelIsomap('precomputed', 4, 4, device='cpu')
    with pytest.raises(ValueError, match='square'):
        KernelIsomap('precomputed', device='cpu').fit(K[:4])
    model = KernelIsomap('precomputed', 2, 2, device='cpu')
    for call in (lambda: model.transform(K), lambda: model.dist_matrix_,
                 model.reconstruction_error):
        with pytest.raises(RuntimeError, match='before fit'):
            call()
    model.fit(K)
    with pytest.raises(ValueError, match='diag'):
        model.transform(K[:2])
    with pytest.raises(ValueError, match=r'diag: \(2,\)'):
        model.transform(K[:2], diag=np.ones(3))
    with pytest.raises(ValueError, match='shape'):
        model.transform(K[:2, :4], diag=np.ones(2))
    bad = np.array(K)
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        KernelIsomap('precomputed', 2, 2, device='cpu').fit(bad)
    with pytest.raises(ValueError, match='not finite'):
        model.transform(bad[:2], diag=np.ones(2))


def test_components_without_weight_are_dropped_with_the_warning():
    """Four points on a line at unit steps, chained: the geodesics are
    Euclidean distances on a line, H B H has rank 1."""
    from graphdot_amd.model.manifold import KernelIsomap
    x = np.arange(4.0)
    K = -0.5 * (x[:, None] - x[None, :]) ** 2       # (d2 = (x_i - x_j)^2)
    with pytest.warns(UserWarning, match='dropped'):
        model = KernelIsomap('precomputed', 1, 2, rcond=1e-8,
                             device='cpu').fit(K)
    assert model.n_components_ == 1 and model.embedding_.shape == (4, 1)
    assert model.eigenvalues_ == pytest.approx([5.0])
    assert np.abs(model.embedding_[:, 0]) == pytest.approx(
        np.abs(x - 1.5))
    assert model.reconstruction_error() <= 1e-6


def test_model_on_graphs_leaves_the_kernel_alone():
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.model.manifold import KernelIsomap
    graphs = np.asarray(cases.config3_graphs(12, seed=3), dtype=object)
    knode, kedge, q = cases.config3_kernels()
    kernel = MarginalizedGraphKernel(knode, kedge, q=q,
                                     backend=OracleBackend())
    # (the oracle backend solves pairs only: the self-similarities of Z as
    # the diagonal of its Gram matrix, as in test_neighbors.py)
    kernel.diag = lambda Z: kernel(Z).diagonal()
    theta0 = np.array(kernel.theta)
    K = np.asarray(kernel(graphs), dtype=np.float64)
    model = KernelIsomap(kernel, 6, 2, device='cpu')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        Y = model.fit_transform(graphs)
    assert np.array_equal(kernel.theta, theta0)
    assert model.last_timing['adopted'] is False
    assert model.last_timing['fused'] is False
    pre = KernelIsomap('precomputed', 6, 2, device='cpu').fit(K)
    assert np.array_equal(Y, pre.embedding_)
    assert np.array_equal(model.dist_matrix_, pre.dist_matrix_)
    new = graphs[:3]
    Ks = np.asarray(kernel(new, graphs), dtype=np.float64)
    dq = np.asarray(kernel.diag(new), dtype=np.float64)
    assert np.array_equal(model.transform(new), pre.transform(Ks, diag=dq))
    assert np.array_equal(model.geodesic_distances(new),
                          pre.geodesic_distances(Ks, diag=dq))
    assert np.array_equal(kernel.theta, theta0)


# -- 7. the kernels' unit ----------------------------------------------------------------
def test_model_unit_compiles_for_gfx950():
    from graphdot_amd.hip import jit, source_module
    from graphdot_amd.model.manifold import _geodesic
    assert 'geodesic' in source_module.MODEL_UNITS
    for older in (source_module.STATIC, source_module.TEXT_UNITS,
                  source_module.FILE_UNITS):
        assert 'geodesic' not in older
    module = source_module.MODEL_UNITS['geodesic']
    path = os.path.join(os.path.dirname(source_module.__file__), '..',
                        'model', 'manifold', 'geodesic.h')
    with open(path) as f:
        assert module.path is None and module.source == f.read()
    assert module.flags == source_module.DENSE_FLAGS
    assert '#include "dense_reduce.h"' in module.source
    assert 'atomic' not in module.source.replace('no atomics', '')
    assert _geodesic._module is module
    image = jit.load_image(module.precompile())
    names = jit.entry_points(module.source)
    assert sorted(names) == sorted(_geodesic.ENTRY_POINTS) and len(names) == 7
    for kernel in names:
        assert kernel.encode() in image, kernel


def test_the_file_keys_its_own_unit_alone(tmp_path, monkeypatch):
    """An edit of model/manifold/geodesic.h gives its unit a new cache key
    and no other source: the file is no header of csrc/device."""
    import shutil
    from graphdot_amd.hip import jit, source_module
    from graphdot_amd.hip.source_module import (FILE_UNITS, MODEL_UNITS,
                                                STATIC, TEXT_UNITS)
    geo, tsne = MODEL_UNITS['geodesic'], FILE_UNITS['tsne']
    knn, mmd = TEXT_UNITS['knn'], STATIC['mmd.hip']
    relative = source_module.MODEL_UNIT_SOURCES['geodesic']
    assert relative == 'model/manifold/geodesic.h'
    assert not os.path.exists(os.path.join(jit.DEVICE_INCLUDE, 'geodesic.h'))

    def keys():
        monkeypatch.setattr(jit, '_hdr_digest', None)
        unit = source_module.SourceModule(source=source_module._text(relative))
        other = source_module.SourceModule(source=source_module._text(
            source_module.FILE_UNIT_SOURCES['tsne']))
        return (unit.key, other.key, jit.cache_key(knn.source, knn.flags),
                jit.cache_key(mmd.source, mmd.flags))
    before = keys()
    assert before == (geo.key, tsne.key, knn.key, mmd.key)
    copy = tmp_path / 'package'
    os.makedirs(copy / 'model')
    shutil.copytree(os.path.join(source_module._PACKAGE, 'model', 'manifold'),
                    copy / 'model' / 'manifold')
    monkeypatch.setattr(source_module, '_PACKAGE', str(copy))
    assert keys() == before
    with open(copy / relative, 'a') as f:
        f.write('// edited\n')
    edited = keys()
    assert edited[0] != before[0] and edited[1:] == before[1:]


def test_the_older_lists_are_what_they_were():
    from graphdot_amd.hip import jit, source_module
    assert list(source_module.FILE_UNITS) == ['tsne']
    assert list(source_module.TEXT_UNITS) == ['knn']
    assert len(source_module.STATIC_SOURCES) == 13
    assert all(p.endswith('.hip') for p in source_module.STATIC_SOURCES)
    assert jit.UNIT_HEADERS == ('knn.h',)
    from graphdot_amd.model.manifold import _geodesic
    assert _geodesic.rounds(64) == 1 and _geodesic.rounds(65) == 2
    assert _geodesic.rounds(129) == 3 and _geodesic.rounds(200) == 4
