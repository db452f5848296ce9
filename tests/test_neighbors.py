"""The neighbour models without a GPU: the host chain (`_knn.topk_torch` and
its siblings, the restatement of csrc/device/knn.h) against the definition of
the lists in numpy -- ``np.lexsort((arange(n), d2_row))[:k]``, the k smallest
in the total order (d2, column) -- with equal indices and equal bits; the four
models against scikit-learn with ``metric='precomputed'`` on sqrt(d2); the
zero-distance rule of ``weights='distance'``; the interface; and the text unit
of the kernels.

The data.  `tied`: integer-valued matrices and self-similarities with few
distinct values, so that most d2 of a row are equal and the column decides.
`duplicated`: an RBF matrix of points of which some are exact copies, so that
``d2 == 0.0`` exactly between them (2 a - 2 a).  `continuous`: RBF matrices
of points around three centres, positive definite and without ties (asserted:
scikit-learn breaks ties differently), with labels that follow the centres
but for a share of random ones.

Rounding bounds.  EPS = 2^-53; a sum of k terms in any order carries at most
k - 1 roundings per term.

* A weighted mean ``sum_r w_r t_r / sum_r w_r``: a weight 1 / sqrt(d2) has 2
  roundings, a product 1, the sum k - 1: the numerator is within ``(k + 2)
  EPS sum_r w_r |t_r|`` of the exact one, the denominator within ``(k + 1) EPS
  sum_r w_r``, the quotient adds 1: a computed mean is within ``2 (k + 2)
  EPS max |T|`` of the exact one, and two computed means within ``C_MEAN (k +
  2) EPS max |T|`` of each other, ``C_MEAN = 4``.
* ``lrd = 1 / (mean_r max(kdist, d) + 1e-10)``: a square root 1, the sum k -
  1, the division by k, the addition and the reciprocal 1 each: k + 3
  relative roundings.  ``lof = mean_r (lrd_train[j] / lrd)``, all terms
  positive: a quotient 2 (k + 3) + 1, the sum k - 1, the division 1: ``(3 k +
  7) EPS <= 4 (k + 2) EPS`` relative, and two computed scores within ``C_LOF
  (k + 2) EPS |score|`` of each other, ``C_LOF = 8``.

(First order in EPS, as in test_two_sample.py.)"""
import warnings
import numpy as np
import pytest

from graphdot_amd.hip.source_module import TEXT_UNITS

EPS = 2.0 ** -53
C_MEAN = 4
C_LOF = 8
KS = [1, 5, 20]
SEEDS = [0, 1, 2]
#: (seed, n) of the comparisons with scikit-learn: seeds for which no two
#: classes of a row have the same vote (asserted where it matters)
CASES = [(4, 30), (7, 115), (16, 200)]


def bound(k, c, scale):
    """``c (k + 2) 2^-53 scale``: see the module's docstring."""
    return c * (k + 2) * EPS * scale


def _torch():
    import torch
    import graphdot_amd.model.neighbors  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


# -- the definition --------------------------------------------------------------------
def define_d2(K, dq, dt):
    """The (b, n) squared distances of the stored matrix widened to double:
    two roundings, no contraction (numpy has none)."""
    d2 = (dq[:, None] + dt[None, :]) - 2.0 * K.astype(np.float64)
    return np.where(d2 < 0.0, 0.0, d2)


def define_topk(K, dq, dt, k, exclude_self=False):
    """(d2 (b, k), idx (b, k)): per row the k smallest (d2, column)."""
    d2 = define_d2(K, dq, dt)
    b, n = d2.shape
    val, idx = np.empty((b, k)), np.empty((b, k), dtype=np.int64)
    for i in range(b):
        order = np.lexsort((np.arange(n), d2[i]))
        if exclude_self:
            order = order[order != i]
        idx[i] = order[:k]
        val[i] = d2[i, idx[i]]
    return val, idx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 \
        and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# -- the data --------------------------------------------------------------------------
def tied(b, n, seed, dtype=np.float64):
    """(K (b, n), dq (b,), dt (n,)): integers with few distinct values."""
    rng = np.random.default_rng(seed)
    K = rng.integers(0, 3, size=(b, n)).astype(dtype)
    if b == n:
        K = np.triu(K) + np.triu(K, 1).T
    dt = rng.integers(4, 6, size=n).astype(np.float64)
    dq = dt.copy() if b == n else rng.integers(4, 6, size=b).astype(
        np.float64)
    return K, dq, dt


def points(n, seed, dim=4):
    """(points around three centres (n, dim), the centre of each)"""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, 3, size=n)
    centres = 3.0 * rng.normal(size=(3, dim))
    return centres[centre] + rng.normal(size=(n, dim)), centre


def rbf(A, B, gamma=0.05):
    return np.exp(-gamma * ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))


def duplicated(n, seed, dtype=np.float64):
    """(K (n, n), diagonal): every third point is a copy of its left
    neighbour; scaled by 1.5, so that the diagonal is not one."""
    A, _ = points(n, seed)
    A[2::3] = A[1:-1:3][:len(A[2::3])]
    K = (1.5 * rbf(A, A)).astype(dtype)
    return K, np.diag(K).astype(np.float64)


def continuous(n, b, seed, dtype=np.float64):
    """(K (n, n), Ks (b, n), dt, dq, labels, targets (n, 3)): the training
    matrix, the cross matrix of b new points and the self-similarities, as
    stored in `dtype`; labels of three classes: the centres, one in six drawn
    at random; targets: smooth functions of the points plus noise."""
    A, centre = points(n + b, seed)
    rng = np.random.default_rng(1000 + seed)
    lab = np.where(rng.random(n) < 1 / 6, rng.integers(0, 3, size=n),
                   centre[:n])
    T = np.stack((A[:n, 0], np.sin(A[:n, 1]), A[:n, 2] * A[:n, 3]), axis=1) \
        + 0.1 * rng.normal(size=(n, 3))
    K = (2.0 * rbf(A[:n], A[:n])).astype(dtype)
    Ks = (2.0 * rbf(A[n:], A[:n])).astype(dtype)
    dt = np.diag(K).astype(np.float64)
    dq = np.full(b, 2.0)
    return K, Ks, dt, dq, lab, T


def smallest_gap(d2):
    """The smallest difference of two consecutive sorted d2 of a row."""
    return float(np.min(np.diff(np.sort(d2, axis=1), axis=1)))


# -- 1. the restatement against the definition -------------------------------------------
def _check_topk(K, dq, dt, k, exclude_self):
    from graphdot_amd.model.neighbors import _knn
    want2, want = define_topk(K, dq, dt, k, exclude_self)
    d2, idx, flag = _knn.topk_torch(_t(K), _t(dq), _t(dt), k, exclude_self)
    assert idx.dtype == _torch().int64 and int(flag) == 0
    assert np.array_equal(idx.numpy(), want), (K.shape, k, exclude_self)
    assert same_bits(d2.numpy(), want2), (K.shape, k, exclude_self)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restatement_on_tied_data(dtype):
    for b, n in ((7, 40), (40, 40), (3, 130)):
        K, dq, dt = tied(b, n, seed=b + n, dtype=dtype)
        # most of a row's d2 are equal: the column decides
        assert len(np.unique(define_d2(K, dq, dt))) <= 7
        for k in (1, 5, min(n - 1, 64)):
            _check_topk(K, dq, dt, k, False)
            if b == n:
                _check_topk(K, dq, dt, k, True)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restatement_on_duplicated_samples(dtype):
    K, d = duplicated(50, seed=5, dtype=dtype)
    d2 = define_d2(K, d, d)
    assert (d2[np.arange(2, 50, 3), np.arange(1, 49, 3)] == 0.0).all()
    for k in (1, 2, 20):
        _check_topk(K, d, d, k, False)
        _check_topk(K, d, d, k, True)
    # a sample's nearest is itself or its copy, whichever has the lower index
    _, idx = define_topk(K, d, d, 1)
    assert idx[2, 0] == 1 and idx[1, 0] == 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('seed', SEEDS)
def test_restatement_on_continuous_data(seed, dtype):
    K, Ks, dt, dq, _, _ = continuous(70, 33, seed, dtype)
    for k in KS:
        _check_topk(Ks, dq, dt, k, False)
        _check_topk(K, dt, dt, k, True)


# -- 2. against scikit-learn -----------------------------------------------------------
def _distances(K, dq, dt):
    d2 = define_d2(K, dq, dt)
    assert smallest_gap(d2) > 0.0
    return np.sqrt(d2)


def _models(cls, K, k, *fit, **kwargs):
    return cls('precomputed', n_neighbors=k, device='cpu', **kwargs).fit(
        K, *fit)


@pytest.mark.parametrize('seed, n', CASES)
def test_search_against_scikit_learn(seed, n):
    sk = pytest.importorskip('sklearn.neighbors')
    from graphdot_amd.model.neighbors import KernelNearestNeighbors
    K, Ks, dt, dq, _, _ = continuous(n, 21, seed)
    D, Ds = _distances(K, dt, dt), _distances(Ks, dq, dt)
    for k in KS:
        ref = sk.NearestNeighbors(n_neighbors=k, metric='precomputed').fit(D)
        m = _models(KernelNearestNeighbors, K, k)
        for want, got in ((ref.kneighbors(Ds), m.kneighbors(Ks, diag=dq)),
                          (ref.kneighbors(), m.kneighbors())):
            assert np.array_equal(got[1], want[1])
            assert got[1].dtype == np.int64 and got[0].dtype == np.float64
            assert np.array_equal(got[0], want[0])
        assert np.array_equal(m.kneighbors(Ks, diag=dq,
                                           return_distance=False),
                              ref.kneighbors(Ds)[1])
        assert np.array_equal(m.kneighbors(Ks, 2, diag=dq)[1],
                              ref.kneighbors(Ds, 2)[1])


@pytest.mark.parametrize('weights', ['uniform', 'distance'])
@pytest.mark.parametrize('seed, n', CASES)
def test_classifier_against_scikit_learn(seed, n, weights):
    sk = pytest.importorskip('sklearn.neighbors')
    from graphdot_amd.model.neighbors import KernelKNeighborsClassifier
    K, Ks, dt, dq, lab, _ = continuous(n, 21, seed)
    D, Ds = _distances(K, dt, dt), _distances(Ks, dq, dt)
    for k in KS:
        ref = sk.KNeighborsClassifier(n_neighbors=k, weights=weights,
                                      metric='precomputed').fit(D, lab)
        m = _models(KernelKNeighborsClassifier, K, k, lab, weights=weights)
        assert np.array_equal(m.classes_, ref.classes_)
        want, got = ref.predict_proba(Ds), m.predict_proba(Ks, diag=dq)
        assert np.all(np.abs(got - want) <= bound(k, C_MEAN, 1.0))
        # no row's two largest probabilities within the bound of each other
        top = np.sort(want, axis=1)
        assert np.all(top[:, -1] - top[:, -2] > bound(k, C_MEAN, 1.0))
        assert np.array_equal(m.predict(Ks, diag=dq), ref.predict(Ds))
        assert m.score(Ks, lab[:21], diag=dq) == ref.score(Ds, lab[:21])


@pytest.mark.parametrize('weights', ['uniform', 'distance'])
@pytest.mark.parametrize('seed, n', CASES)
def test_regressor_against_scikit_learn(seed, n, weights):
    sk = pytest.importorskip('sklearn.neighbors')
    from graphdot_amd.model.neighbors import KernelKNeighborsRegressor
    K, Ks, dt, dq, _, T = continuous(n, 21, seed)
    D, Ds = _distances(K, dt, dt), _distances(Ks, dq, dt)
    for k in KS:
        for y in (T, T[:, 1]):
            ref = sk.KNeighborsRegressor(n_neighbors=k, weights=weights,
                                         metric='precomputed').fit(D, y)
            m = _models(KernelKNeighborsRegressor, K, k, y, weights=weights)
            want, got = ref.predict(Ds), m.predict(Ks, diag=dq)
            assert got.shape == want.shape == (21,) + y.shape[1:]
            assert np.all(np.abs(got - want)
                          <= bound(k, C_MEAN, np.abs(y).max()))


@pytest.mark.parametrize('seed, n', CASES)
def test_outlier_factor_against_scikit_learn(seed, n):
    sk = pytest.importorskip('sklearn.neighbors')
    from graphdot_amd.model.neighbors import KernelLocalOutlierFactor
    K, Ks, dt, dq, _, _ = continuous(n, 21, seed)
    D, Ds = _distances(K, dt, dt), _distances(Ks, dq, dt)
    for k in KS:
        for contamination in ('auto', 0.1):
            ref = sk.LocalOutlierFactor(
                n_neighbors=k, metric='precomputed', novelty=True,
                contamination=contamination).fit(D)
            m = KernelLocalOutlierFactor(
                'precomputed', n_neighbors=k, contamination=contamination,
                device='cpu').fit(K)
            want, got = ref.negative_outlier_factor_, \
                m.negative_outlier_factor_
            assert np.all(np.abs(got - want)
                          <= bound(k, C_LOF, np.abs(want)))
            assert abs(m.offset_ - ref.offset_) \
                <= bound(k, C_LOF, abs(ref.offset_))
            want, got = ref.score_samples(Ds), m.score_samples(Ks, diag=dq)
            assert np.all(np.abs(got - want)
                          <= bound(k, C_LOF, np.abs(want)))
            # (no decision value within the bound of zero)
            assert np.all(np.abs(want - ref.offset_)
                          > 2 * bound(k, C_LOF, np.abs(want)))
            assert np.array_equal(m.predict(Ks, diag=dq), ref.predict(Ds))
            assert np.allclose(m.decision_function(Ks, diag=dq),
                               ref.decision_function(Ds), rtol=0, atol=1e-12)
        plain = sk.LocalOutlierFactor(n_neighbors=k, metric='precomputed')
        assert np.array_equal(
            KernelLocalOutlierFactor('precomputed', k,
                                     device='cpu').fit_predict(K),
            plain.fit_predict(D))


# -- 3. the zero-distance rule ---------------------------------------------------------
def test_distance_weights_of_duplicated_samples():
    from graphdot_amd.model.neighbors import (
        KernelKNeighborsClassifier, KernelKNeighborsRegressor, _knn)
    n = 50
    K, d = duplicated(n, seed=9)
    rng = np.random.default_rng(3)
    y = rng.normal(size=n)
    lab = rng.integers(0, 3, size=n)
    k = 4
    d2, idx = define_topk(K, d, d, k)
    # the queries are the training samples themselves: every list starts at
    # d == 0 -- with one entry, or with two for a sample and its copy
    zeros = (d2 == 0.0).sum(1)
    assert set(zeros) == {1, 2} and (zeros == 2).sum() == 2 * len(d2[2::3])
    w = _knn.weights_torch(_t(d2), 'distance').numpy()
    assert np.array_equal(w, (d2 == 0.0).astype(np.float64))
    want = np.array([y[idx[i, :zeros[i]]].sum() / zeros[i] for i in range(n)])
    got = KernelKNeighborsRegressor('precomputed', k, 'distance',
                                    device='cpu').fit(K, y).predict(K, diag=d)
    assert np.all(np.abs(got - want) <= bound(k, C_MEAN, np.abs(y).max()))
    proba = KernelKNeighborsClassifier(
        'precomputed', k, 'distance', device='cpu').fit(K, lab).predict_proba(
            K, diag=d)
    for i in range(n):
        votes = np.bincount(lab[idx[i, :zeros[i]]], minlength=3) / zeros[i]
        assert np.array_equal(proba[i], votes)
    # without zeros in a list: 1 / d
    w = _knn.weights_torch(_t(np.array([[0.25, 4.0]])), 'distance').numpy()
    assert np.array_equal(w, [[2.0, 0.5]])
    w = _knn.weights_torch(_t(np.array([[0.0, 4.0]])), 'uniform').numpy()
    assert np.array_equal(w, [[1.0, 1.0]])


# -- 4. the interface --------------------------------------------------------------------
def test_errors():
    from graphdot_amd.model.neighbors import (
        KernelKNeighborsClassifier, KernelKNeighborsRegressor,
        KernelLocalOutlierFactor, KernelNearestNeighbors)
    K, Ks, dt, dq, lab, T = continuous(12, 3, seed=0)
    m = KernelNearestNeighbors('precomputed', 12, device='cpu').fit(K)
    assert m.kneighbors(Ks, diag=dq)[1].shape == (3, 12)
    with pytest.raises(ValueError, match='exceeds'):
        m.kneighbors()                       # 11 candidates with Z=None
    with pytest.raises(ValueError, match='exceeds'):
        m.kneighbors(Ks, 13, diag=dq)
    assert m.kneighbors(n_neighbors=11)[1].shape == (12, 11)
    with pytest.raises(ValueError, match='diag'):
        m.kneighbors(Ks)
    with pytest.raises(ValueError, match='diag'):
        m.kneighbors(Ks, diag=dq[:2])
    with pytest.raises(ValueError, match='shape'):
        m.kneighbors(Ks[:, :5], diag=dq)
    with pytest.raises(ValueError, match='n_neighbors'):
        KernelNearestNeighbors('precomputed', 0)
    with pytest.raises(ValueError, match='weights'):
        KernelKNeighborsRegressor('precomputed', weights='rank')
    with pytest.raises(ValueError, match='contamination'):
        KernelLocalOutlierFactor('precomputed', contamination=0.7)
    for model, call in (
            (KernelNearestNeighbors('precomputed'), 'kneighbors'),
            (KernelKNeighborsClassifier('precomputed'), 'predict'),
            (KernelKNeighborsClassifier('precomputed'), 'predict_proba'),
            (KernelKNeighborsRegressor('precomputed'), 'predict'),
            (KernelLocalOutlierFactor('precomputed'), 'score_samples'),
            (KernelLocalOutlierFactor('precomputed'), 'predict')):
        with pytest.raises(ValueError, match='before fit'):
            getattr(model, call)(Ks, diag=dq)
    with pytest.raises(ValueError, match='rows'):
        KernelKNeighborsRegressor('precomputed', 3, device='cpu').fit(
            K, T[:5])


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_entries_that_are_not_finite(bad):
    from graphdot_amd.model.neighbors import (
        KernelKNeighborsRegressor, KernelLocalOutlierFactor,
        KernelNearestNeighbors)
    K, Ks, dt, dq, lab, T = continuous(12, 3, seed=0)
    m = KernelNearestNeighbors('precomputed', 3, device='cpu').fit(K)
    Kb = Ks.copy()
    Kb[1, 7] = bad
    with pytest.raises(ValueError, match='not finite'):
        m.kneighbors(Kb, diag=dq)
    db = dq.copy()
    db[2] = bad
    with pytest.raises(ValueError, match='not finite'):
        m.kneighbors(Ks, diag=db)
    Kb = K.copy()
    Kb[3, 8] = Kb[8, 3] = bad
    with pytest.raises(ValueError, match='not finite'):
        KernelNearestNeighbors('precomputed', 3, device='cpu').fit(
            Kb).kneighbors()
    with pytest.raises(ValueError, match='not finite'):
        KernelLocalOutlierFactor('precomputed', 3, device='cpu').fit(Kb)
    Kb = K.copy()
    Kb[5, 5] = bad                           # a training self-similarity
    with pytest.raises(ValueError, match='not finite'):
        KernelKNeighborsRegressor('precomputed', 3, device='cpu').fit(
            Kb, T).predict(Ks, diag=dq)


def test_outlier_factor_clips_its_neighbours():
    from graphdot_amd.model.neighbors import KernelLocalOutlierFactor
    K, _, _, _, _, _ = continuous(12, 3, seed=0)
    with pytest.warns(UserWarning, match='n_neighbors'):
        m = KernelLocalOutlierFactor('precomputed', device='cpu').fit(K)
    assert m.n_neighbors_ == 11 and m.n_neighbors == 20
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = KernelLocalOutlierFactor('precomputed', 11, device='cpu').fit(K)
    assert m.n_neighbors_ == 11 and m.offset_ == -1.5
    low = KernelLocalOutlierFactor('precomputed', 5, contamination=0.25,
                                   device='cpu').fit(K)
    assert low.offset_ == np.percentile(low.negative_outlier_factor_, 25.0)
    assert (low.fit_predict(K) == -1).sum() == 3


def test_hashable_labels_of_mixed_order():
    from graphdot_amd.model.neighbors import KernelKNeighborsClassifier
    K, Ks, dt, dq, lab, _ = continuous(40, 9, seed=1)
    plain = KernelKNeighborsClassifier('precomputed', 5, device='cpu').fit(
        K, lab)
    for names in (['pear', 'apple', 'fig'], [('b', 2), ('a', 7), ('a', 1)],
                  [2.5, -1.0, 0.0]):
        m = KernelKNeighborsClassifier('precomputed', 5, device='cpu').fit(
            K, [names[c] for c in lab])
        assert m.classes_.tolist() == sorted(names)
        order = np.argsort(np.argsort([sorted(names).index(x)
                                       for x in names]))
        assert np.array_equal(m.predict_proba(Ks, diag=dq)[:, order],
                              plain.predict_proba(Ks, diag=dq))
        got = m.predict(Ks, diag=dq).tolist()
        assert got == [names[c] for c in plain.predict(Ks, diag=dq)]
        assert m.score(Ks, got, diag=dq) == 1.0


def test_leave_one_out_scores():
    """`loo_score` against a loop that really leaves each sample out: a model
    fitted on the other n - 1 samples predicts the one."""
    from graphdot_amd.model.neighbors import (
        KernelKNeighborsClassifier, KernelKNeighborsRegressor)
    n, k = 30, 4
    K, _, dt, _, lab, T = continuous(n, 1, seed=2)
    for weights in ('uniform', 'distance'):
        for y in (T, T[:, 0]):
            got = np.empty_like(y)
            for i in range(n):
                rest = np.arange(n) != i
                m = KernelKNeighborsRegressor(
                    'precomputed', k, weights, device='cpu').fit(
                        K[np.ix_(rest, rest)], y[rest])
                got[i] = m.predict(K[i:i + 1, rest], diag=dt[i:i + 1])[0]
            r2 = 1.0 - ((y - got) ** 2).sum() / ((y - y.mean(0)) ** 2).sum()
            m = KernelKNeighborsRegressor('precomputed', k, weights,
                                          device='cpu').fit(K, y)
            assert m.loo_score() == pytest.approx(r2, rel=1e-12)
        hits = 0
        for i in range(n):
            rest = np.arange(n) != i
            m = KernelKNeighborsClassifier(
                'precomputed', k, weights, device='cpu').fit(
                    K[np.ix_(rest, rest)], lab[rest])
            hits += m.predict(K[i:i + 1, rest], diag=dt[i:i + 1])[0] == lab[i]
        m = KernelKNeighborsClassifier('precomputed', k, weights,
                                       device='cpu').fit(K, lab)
        assert m.loo_score() == hits / n


def test_models_on_graphs_leave_the_kernel_alone():
    """The four models with a graph kernel on the host: the results are those
    of the precomputed matrices of the same kernel, and the kernel object is
    unchanged after every call."""
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.model.neighbors import (
        KernelKNeighborsClassifier, KernelKNeighborsRegressor,
        KernelLocalOutlierFactor, KernelNearestNeighbors)
    G = np.asarray(cases.config3_graphs(10, seed=3), dtype=object)
    knode, kedge, q = cases.config3_kernels()
    kernel = MarginalizedGraphKernel(knode, kedge, q=q,
                                     backend=OracleBackend())
    # (the oracle backend solves pairs only: the self-similarities of Z as
    # the diagonal of its Gram matrix, as in test_kkmeans.py)
    kernel.diag = lambda Z: kernel(Z).diagonal()
    size = np.array([float(len(g.nodes)) for g in G])
    lab = (size > np.median(size)).astype(int)
    theta0 = np.array(kernel.theta)
    X, Z = G[:7], G[7:]
    K = np.asarray(kernel(X), dtype=np.float64)
    Ks = np.asarray(kernel(Z, X), dtype=np.float64)
    dq = np.asarray(kernel.diag(Z), dtype=np.float64)
    k = 3

    def unchanged():
        assert np.array_equal(kernel.theta, theta0)

    m = KernelNearestNeighbors(kernel, k, device='cpu').fit(X)
    p = KernelNearestNeighbors('precomputed', k, device='cpu').fit(K)
    assert m.last_timing['adopted'] is False
    assert m.last_timing['fused'] is False
    unchanged()
    for got, want in ((m.kneighbors(Z), p.kneighbors(Ks, diag=dq)),
                      (m.kneighbors(), p.kneighbors())):
        unchanged()
        assert np.array_equal(got[1], want[1])
        assert np.array_equal(got[0], want[0])
    assert set(m.last_timing) == {'kernel', 'linalg', 'adopted', 'fused'}
    c = KernelKNeighborsClassifier(kernel, k, 'distance',
                                   device='cpu').fit(X, lab[:7])
    pc = KernelKNeighborsClassifier('precomputed', k, 'distance',
                                    device='cpu').fit(K, lab[:7])
    unchanged()
    assert np.array_equal(c.predict_proba(Z), pc.predict_proba(Ks, diag=dq))
    assert np.array_equal(c.predict(Z), pc.predict(Ks, diag=dq))
    assert c.score(Z, lab[7:]) == pc.score(Ks, lab[7:], diag=dq)
    assert c.loo_score() == pc.loo_score()
    unchanged()
    r = KernelKNeighborsRegressor(kernel, k, device='cpu').fit(X, size[:7])
    pr = KernelKNeighborsRegressor('precomputed', k,
                                   device='cpu').fit(K, size[:7])
    assert np.array_equal(r.predict(Z), pr.predict(Ks, diag=dq))
    assert r.score(Z, size[7:]) == pr.score(Ks, size[7:], diag=dq)
    assert r.loo_score() == pr.loo_score()
    unchanged()
    o = KernelLocalOutlierFactor(kernel, k, device='cpu').fit(X)
    po = KernelLocalOutlierFactor('precomputed', k, device='cpu').fit(K)
    unchanged()
    assert np.array_equal(o.negative_outlier_factor_,
                          po.negative_outlier_factor_)
    assert np.array_equal(o.score_samples(Z), po.score_samples(Ks, diag=dq))
    assert np.array_equal(o.predict(Z), po.predict(Ks, diag=dq))
    unchanged()


# -- 5. the kernels' text unit ---------------------------------------------------------
def test_text_unit_compiles_for_gfx950():
    from graphdot_amd.hip import jit
    from graphdot_amd.hip.source_module import STATIC
    from graphdot_amd.model.neighbors import _knn
    assert list(TEXT_UNITS) == ['knn'] and 'knn' not in STATIC
    module = TEXT_UNITS['knn']
    assert module.path is None and '#include "knn.h"' in module.source
    path = module.precompile()
    names = jit.entry_points(module.source)
    assert sorted(names) == ['knn_average', 'knn_lrd', 'knn_merge',
                             'knn_ratio', 'knn_topk_f32', 'knn_topk_f64']
    image = jit.load_image(path)
    for kernel in names:
        assert kernel.encode() in image, kernel
    assert _knn.K_MOST == 64


def test_the_header_keys_its_own_unit_alone(tmp_path, monkeypatch):
    """csrc/device/knn.h is a `jit.UNIT_HEADERS` header: an edit of it gives
    the text unit that includes it a new cache key and no other source (the
    recorded keys of tests/golden/host_plans.json stay what they are); an edit
    of a shared header gives every source a new key, this unit included."""
    import shutil
    from graphdot_amd.hip import jit
    from graphdot_amd.hip.source_module import STATIC
    assert jit.UNIT_HEADERS == ('knn.h',)
    knn, mmd = TEXT_UNITS['knn'], STATIC['mmd.hip']
    assert '"knn.h"' not in mmd.source

    def keys():
        monkeypatch.setattr(jit, '_hdr_digest', None)
        return (jit.cache_key(knn.source, knn.flags),
                jit.cache_key(mmd.source, mmd.flags))
    before = keys()
    assert before == (knn.key, mmd.key)
    copy = tmp_path / 'device'
    shutil.copytree(jit.DEVICE_INCLUDE, copy)
    monkeypatch.setattr(jit, 'DEVICE_INCLUDE', str(copy))
    assert keys() == before
    with open(copy / 'knn.h', 'a') as f:
        f.write('// edited\n')
    edited = keys()
    assert edited[0] != before[0] and edited[1] == before[1]
    with open(copy / 'dense_reduce.h', 'a') as f:
        f.write('// edited\n')
    both = keys()
    assert both[0] != edited[0] and both[1] != before[1]


def test_the_split_of_the_columns_is_a_function_of_the_shape():
    from graphdot_amd.model.neighbors import _knn
    assert _knn.parts_for(1000, 1000) == 16         # 32 strips, 16 tiles
    assert _knn.parts_for(1, 64) == 1 and _knn.parts_for(1, 65) == 2
    assert _knn.parts_for(64, 100000) == _knn.PARTS_MOST
    assert _knn.parts_for(1000, 20000) == 16        # 32 strips
    assert _knn.parts_for(100000, 1000) == 1
    assert _knn.parts_for(5, 5, 7) == 7
    with pytest.raises(ValueError, match='parts'):
        _knn.parts_for(5, 5, 0)
    with pytest.raises(ValueError, match='parts'):
        _knn.parts_for(5, 5, _knn.PARTS_MOST + 1)
