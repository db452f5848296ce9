"""KernelKMeans without a GPU: the host chain (the ``*_torch`` restatements
of lloyd.hip) against an independent Lloyd iteration on explicit features
written here in numpy, and against scikit-learn's; the definitions of the
inertia, the medoids and the distances; the restarts, the two seedings on
their defining properties, the warnings, the value errors and the cadence of
the host's looks.

The inputs are Gram matrices ``K = X X^T`` of Gaussian blobs in five
dimensions, so that every quantity has an explicit counterpart.  Across all
rounds of these runs the gap between the best and the second-best d2 is at
least 4.4e-7 max|K|, far above the differences between two orders of
summation (n eps |K|, about 1e-13 |K|): the labels of the Gram form and of the
explicit form must be identical."""
import warnings
import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
#: (n, k): the smallest problems, a cluster count on either side of a register
#: chunk of 16 and of a block of 256 samples, and the size of the timings
NK = [(2, 1), (3, 2), (65, 9), (257, 16), (257, 17), (1000, 8)]
SEEDS = [0, 1, 2]
DIM = 5


def _torch():
    import torch
    import graphdot_amd.model.clustering  # noqa: F401 (torch first)
    return torch


_cases = {}


def blobs(n, k, seed):
    """(X, K, labels0): computed once and left unchanged."""
    if (n, k, seed) not in _cases:
        rng = np.random.default_rng(seed)
        cen = rng.normal(size=(k, DIM)) * 3
        X = cen[rng.integers(0, k, n)] + rng.normal(size=(n, DIM))
        K = X @ X.T
        assert np.array_equal(K, K.T)
        labels0 = rng.integers(0, k, n)
        labels0[:k] = np.arange(k)
        _cases[n, k, seed] = (X, K, labels0)
    return _cases[n, k, seed]


def lloyd(X, lab, k, max_iter=300):
    """Lloyd's iteration on explicit features: (labels the last round used,
    its number, the inertia of the labels each round used)."""
    n = len(X)
    history = []
    for it in range(1, max_iter + 1):
        cnt = np.bincount(lab, minlength=k)
        cen = np.zeros((k, X.shape[1]))
        np.add.at(cen, lab, X)
        cen[cnt > 0] /= cnt[cnt > 0, None]
        d = ((X[:, None, :] - cen[None, :, :]) ** 2).sum(-1)
        d[:, cnt == 0] = np.inf
        history.append(d[np.arange(n), lab].sum())
        new = d.argmin(1)
        if np.array_equal(new, lab):
            break
        lab = new if it < max_iter else lab
    return lab, it, history


def inertia_of(K, lab, k):
    """The definition, from the Gram matrix."""
    total = np.trace(K)
    for c in range(k):
        m = lab == c
        if m.any():
            total -= K[np.ix_(m, m)].sum() / m.sum()
    return total


def model(k, **kwargs):
    from graphdot_amd.model.clustering import KernelKMeans
    kwargs.setdefault('device', 'cpu')
    return KernelKMeans('precomputed', k, **kwargs)


def check_fit(km, X, K, lab, it, history):
    """The assertions of a fit from start labels (the GPU file's too)."""
    k = km.n_clusters
    assert np.array_equal(km.labels_, lab)
    assert km.n_iter_ == it
    assert abs(km.inertia_ - history[-1]) <= 1e-9 * abs(history[-1])
    assert abs(km.inertia_ - inertia_of(K, lab, k)) \
        <= 1e-9 * abs(history[-1])
    assert np.array_equal(km.cluster_sizes_, np.bincount(lab, minlength=k))
    check_medoids(X, K, lab, k, km.medoid_indices_)


def check_medoids(X, K, lab, k, got):
    """The member nearest to its cluster's mean; where two members are as
    near as the rounding of d2 can tell (a sum of n products of the size of K:
    ``8 n eps max|K|``), either (n = 2, k = 1 is an exact tie)."""
    bound = 8 * len(X) * EPS * np.abs(K).max()
    assert got.shape == (k,)
    for c in range(k):
        m = np.flatnonzero(lab == c)
        if not len(m):
            assert got[c] == -1
            continue
        d = ((X[m] - X[m].mean(0)) ** 2).sum(1)
        assert got[c] in m
        assert d[list(m).index(got[c])] <= d.min() + bound
        if np.ptp(np.sort(d)[:2]) > bound if len(m) > 1 else True:
            assert got[c] == m[np.argmin(d)]


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n,k', NK)
def test_against_lloyd_on_explicit_features(n, k, seed):
    X, K, labels0 = blobs(n, k, seed)
    lab, it, history = lloyd(X, labels0, k)
    assert it <= 40
    km = model(k)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # (empty clusters: tested below)
        km.fit(K, labels0=labels0)
    check_fit(km, X, K, lab, it, history)
    assert km.seed_indices_ is None and km.best_restart_ == 0


@pytest.mark.parametrize('n,k', NK)
def test_against_scikit_learn(n, k):
    cluster = pytest.importorskip('sklearn.cluster')
    X, K, _ = blobs(n, k, 0)
    seeds = np.random.default_rng(n + k).choice(n, k, replace=False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref = cluster.KMeans(n_clusters=k, init=X[seeds], n_init=1,
                             algorithm='lloyd', tol=0).fit(X)
        km = model(k, init=seeds).fit(K)
    assert np.array_equal(km.seed_indices_, seeds[None, :])
    assert np.array_equal(km.labels_, ref.labels_)
    assert abs(km.inertia_ - ref.inertia_) <= 1e-9 * ref.inertia_


@pytest.mark.parametrize('n,k', [(65, 9), (257, 16), (1000, 8)])
def test_inertia_does_not_increase(n, k):
    X, K, labels0 = blobs(n, k, 1)
    _, it, history = lloyd(X, labels0, k)
    got = []
    for rounds in range(1, it + 1):
        km = model(k, max_iter=rounds)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            km.fit(K, labels0=labels0)
        got.append(km.inertia_)
        assert abs(km.inertia_ - inertia_of(K, km.labels_, k)) \
            <= 1e-9 * history[0]
    assert np.all(np.diff(got) <= 1e-12 * history[0])
    np.testing.assert_allclose(got, history, rtol=1e-9)


def test_restarts():
    from graphdot_amd.model.clustering import _lloyd
    torch = _torch()
    n, k, R = 257, 6, 5
    X, K, _ = blobs(n, k, 3)
    Kt = torch.from_numpy(K)
    u = np.random.default_rng(11).random((R, k))
    for init in _lloyd.INITS:
        whole = _lloyd.iterate(Kt, k, init=init, u=u)
        assert whole.labels.shape == (R, n)
        for r in range(R):
            one = _lloyd.iterate(Kt, k, init=init, u=u[r:r + 1])
            assert torch.equal(one.labels[0], whole.labels[r])
            assert one.inertia[0] == whole.inertia[r]
            assert one.n_iter[0] == whole.n_iter[r]
            assert torch.equal(one.seeds[0], whole.seeds[r])
        assert whole.best == int(np.argmin(whole.inertia))
        for r in range(R):
            lab = whole.labels[r].numpy()
            assert abs(whole.inertia[r] - inertia_of(K, lab, k)) \
                <= 1e-9 * whole.inertia[r]
    # the model reports the best restart of the u it draws from random_state
    km = model(k, n_init=R, random_state=11).fit(K)
    whole = _lloyd.iterate(Kt, k, u=u)
    assert km.best_restart_ == whole.best
    assert np.array_equal(km.labels_, whole.labels[whole.best].numpy())
    assert km.inertia_ == whole.inertia.min()
    assert np.array_equal(km.restart_inertia_, whole.inertia)
    assert np.array_equal(km.seed_indices_, whole.seeds.numpy())


def check_seeding(K, k, init, u, seeds, labels, mind):
    """The defining properties of a seeding, given what it returned (numpy
    arrays; K as float64, the stored values).  ``mind`` before each step is
    recomputed here: its arithmetic, ``(K_ii + K_jj) - 2 K_ij`` clamped at 0
    and a minimum, is exact to reproduce.  The chosen index i of 'k-means++'
    must satisfy ``cum[i - 1] <= u total < cum[i]`` for numpy's cumulative
    sum, with a slack of ``n eps total`` on either side: two orders of
    summation of n non-negative terms differ by less."""
    n = len(K)
    d = np.diagonal(K)
    for r in range(len(seeds)):
        m = lab = None
        for t in range(k):
            j = int(seeds[r, t])
            assert 0 <= j < n
            if init == 'given':
                pass
            elif t == 0:
                assert j == min(n - 1, int(u[r, 0] * n))
            elif init == 'farthest':
                assert j == int(np.argmax(m))
            else:
                cum = np.cumsum(m)
                total = cum[-1]
                if total == 0:
                    assert j == min(set(range(n)) - set(seeds[r, :t].tolist()))
                else:
                    slack = n * EPS * total
                    below = cum[j - 1] if j else 0.0
                    assert below - slack <= u[r, t] * total < cum[j] + slack
                    assert m[j] > 0
            dist = np.maximum((d + d[j]) - 2.0 * K[j], 0.0)
            if t == 0:
                m, lab = dist, np.zeros(n, dtype=np.int64)
            else:
                lab = np.where(dist < m, t, lab)
                m = np.minimum(m, dist)
        assert np.array_equal(mind[r], m)
        assert np.array_equal(labels[r], lab)


@pytest.mark.parametrize('init', ['k-means++', 'farthest'])
@pytest.mark.parametrize('n,k', NK + [(64, 64)])
def test_seeding(n, k, init):
    from graphdot_amd.model.clustering import _lloyd
    torch = _torch()
    K = blobs(n, min(k, 17), 4)[1]
    u = np.random.default_rng(n).random((3, k))
    seeds, lab, mind = _lloyd.seed_torch(torch.from_numpy(K), k, init, u)
    assert all(len(set(row)) == k for row in seeds.tolist())
    check_seeding(K, k, init, u, seeds.numpy(), lab.numpy(), mind.numpy())


def test_seeding_of_coincident_samples():
    """All distances vanish: 'k-means++' takes the lowest index not chosen."""
    from graphdot_amd.model.clustering import _lloyd
    torch = _torch()
    n, k = 7, 3
    K = np.ones((n, n))
    u = np.array([[0.5, 0.9, 0.1]])
    seeds, lab, mind = _lloyd.seed_torch(torch.from_numpy(K), k, 'k-means++', u)
    assert seeds.tolist() == [[3, 0, 1]]
    check_seeding(K, k, 'k-means++', u, seeds.numpy(), lab.numpy(),
                  mind.numpy())
    with pytest.warns(UserWarning, match='empty'):
        km = model(k, n_init=1).fit(K)
    assert km.cluster_sizes_.tolist() == [n, 0, 0]


def test_predict_and_transform():
    n, k = 257, 6
    X, K, labels0 = blobs(n, k, 5)
    km = model(k, n_init=3).fit(K)
    assert km.n_iter_ < 300 and km.cluster_sizes_.min() > 0
    assert np.array_equal(km.predict(K), km.labels_)
    assert np.array_equal(model(k).fit_predict(K, labels0),
                          lloyd(X, labels0, k)[0])
    rng = np.random.default_rng(6)
    Z = rng.normal(size=(9, DIM)) * 3
    cen = np.stack([X[km.labels_ == c].mean(0) for c in range(k)])
    want = ((Z[:, None, :] - cen[None, :, :]) ** 2).sum(-1)
    got = km.transform(Z @ X.T, diag=(Z * Z).sum(1))
    assert got.shape == (9, k)
    # d2 is a sum of n products of the size of K on either side
    size = max(np.abs(K).max(), (Z * Z).sum(1).max())
    assert np.abs(got ** 2 - want).max() <= 8 * n * EPS * size
    assert np.array_equal(km.predict(Z @ X.T), want.argmin(1))
    with pytest.raises(ValueError, match='diag'):
        km.transform(Z @ X.T)


def test_empty_cluster_and_max_iter_warnings():
    n, k = 65, 4
    X, K, _ = blobs(n, 3, 6)
    labels0 = np.arange(n) % 3             # (cluster 3 is and stays empty)
    with pytest.warns(UserWarning, match='1 of 4 clusters are empty'):
        km = model(k).fit(K, labels0=labels0)
    lab, it, history = lloyd(X, labels0, k)
    check_fit(km, X, K, lab, it, history)
    assert km.cluster_sizes_[3] == 0 and km.medoid_indices_[3] == -1
    assert np.isinf(km.transform(K[:2], diag=np.diagonal(K)[:2])[:, 3]).all()
    # unconverged: the attributes describe the labels the last round used
    X, K, labels0 = blobs(257, 16, 0)
    for rounds in (1, 2, 5):
        with pytest.warns(UserWarning, match='not converged'):
            km = model(16, max_iter=rounds).fit(K, labels0=labels0)
        lab, it, history = lloyd(X, labels0, 16, max_iter=rounds)
        assert it == rounds
        check_fit(km, X, K, lab, it, history)


def test_value_errors():
    from graphdot_amd.model.clustering import KernelKMeans
    X, K, labels0 = blobs(65, 9, 0)
    for k in (0, 65, 2.5):
        with pytest.raises(ValueError):
            KernelKMeans('precomputed', k)
    with pytest.raises(ValueError):
        KernelKMeans('precomputed', 3, init='random')
    with pytest.raises(ValueError, match='n_clusters'):
        model(9).fit(K[:8, :8])
    with pytest.raises(ValueError, match='square'):
        model(3).fit(K[:8])
    for init in ([0, 1, 1], [0, 1, 65], [0, 1], [[0, 1, -1]], [0.0, 1.0, 2.0]):
        with pytest.raises(ValueError, match='init'):
            model(3, init=np.array(init)).fit(K)
    for bad in (labels0[:-1], np.full(65, 9), np.full(65, -1),
                labels0.astype(float), np.zeros((2, 2, 65), dtype=int)):
        with pytest.raises(ValueError, match='labels0'):
            model(9).fit(K, labels0=bad)
    for name in ('n_init', 'max_iter'):
        with pytest.raises(ValueError, match=name):
            model(3, **{name: 0}).fit(K)
    with pytest.raises(ValueError, match='before fit'):
        model(3).predict(K)
    with pytest.raises(ValueError, match='before fit'):
        model(3).transform(K, diag=np.diagonal(K))
    km = model(3).fit(K)
    with pytest.raises(ValueError):
        km.predict(K[:, :-1])
    bad = K.copy()
    bad[3, 5] = bad[5, 3] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        model(3).fit(bad)


def test_precomputed_accepts_numpy_and_torch():
    torch = _torch()
    n, k = 65, 9
    X, K, labels0 = blobs(n, k, 0)
    want = model(k).fit(K, labels0=labels0)
    for given in (torch.from_numpy(K), K.astype(np.float32),
                  torch.from_numpy(K.astype(np.float32)),
                  torch.from_numpy(K).t().contiguous().t()):
        km = model(k).fit(given, labels0=labels0)
        assert np.array_equal(km.labels_, want.labels_)
        assert abs(km.inertia_ - want.inertia_) <= 1e-5 * want.inertia_
        assert np.array_equal(km.predict(given), want.labels_)
    km = model(k).fit(K, labels0=np.stack((labels0, want.labels_)))
    assert np.array_equal(km.labels_, want.labels_)
    assert km.restart_n_iter_.tolist() == [want.n_iter_, 1]


def test_repeats_are_identical():
    X, K, _ = blobs(257, 16, 2)
    a, b = (model(16, n_init=4, random_state=3).fit(K) for _ in range(2))
    assert np.array_equal(a.labels_, b.labels_)
    assert a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_
    assert np.array_equal(a.medoid_indices_, b.medoid_indices_)
    assert np.array_equal(a.transform(K[:5], diag=np.diagonal(K)[:5]),
                          b.transform(K[:5], diag=np.diagonal(K)[:5]))


def test_cadence_of_the_looks():
    from graphdot_amd.model.clustering import _lloyd
    torch = _torch()
    assert _lloyd.CHECK_EVERY == 4
    for n, k in ((65, 9), (257, 16), (1000, 8)):
        X, K, labels0 = blobs(n, k, 0)
        it = lloyd(X, labels0, k)[1]
        r = _lloyd.iterate(torch.from_numpy(K), k, labels0)
        assert r.n_iter[0] == it
        assert r.rounds == -(-it // 4) * 4 and r.looks == r.rounds // 4
        r = _lloyd.iterate(torch.from_numpy(K), k, labels0, max_iter=it + 1)
        assert r.rounds == min(it + 1, -(-it // 4) * 4)
        assert r.looks == -(-r.rounds // 4) and r.n_iter[0] == it
        assert r.converged[0]
    assert _lloyd.grid(1000, 8) == (8, 1, 63, 4)
    assert _lloyd.grid(257, 17) == (16, 2, 17, 2)


def test_graph_kernel_without_a_device_path():
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.model.clustering import KernelKMeans
    G = np.asarray(cases.config3_graphs(12, seed=3), dtype=object)
    knode, kedge, q = cases.config3_kernels()
    mgk = MarginalizedGraphKernel(knode, kedge, q=q, backend=OracleBackend())
    # (the oracle backend solves pairs only: the self-similarities of Z as
    # the diagonal of its Gram matrix)
    mgk.diag = lambda Z: mgk(Z).diagonal()
    X, Z = G[:9], G[9:]
    k = 3
    labels0 = np.arange(9) % k
    for kernel in (mgk, Normalization(mgk)):
        K = np.asarray(kernel(X), dtype=np.float64)
        Ks = np.asarray(kernel(Z, X), dtype=np.float64)
        want = model(k).fit(K, labels0=labels0)
        km = KernelKMeans(kernel, k, device='cpu').fit(X, labels0=labels0)
        assert km.last_timing['adopted'] is False
        assert np.array_equal(km.labels_, want.labels_)
        assert km.inertia_ == want.inertia_ and km.n_iter_ == want.n_iter_
        assert np.array_equal(km.medoid_indices_, want.medoid_indices_)
        assert np.array_equal(km.predict(Z), want.predict(Ks))
        assert np.array_equal(
            km.transform(Z), want.transform(Ks, diag=kernel.diag(Z)))
        seeded = KernelKMeans(kernel, k, n_init=3, device='cpu').fit(X)
        assert seeded.inertia_ <= seeded.restart_inertia_.min()
        assert abs(seeded.inertia_ - inertia_of(K, seeded.labels_, k)) \
            <= 1e-9 * np.trace(K)
