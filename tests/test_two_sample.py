"""KernelTwoSampleTest without a GPU: the host chain (`_mmd.forms_torch`, the
restatement of mmd.hip) and `_mmd.statistics` against the definition of the
maximum mean discrepancy as block means over ``np.ix_`` index sets in numpy
double; the generator of the splits; the p-value, exactly, against the
definition's own; ties; the witness; the errors; and the model on a handful of
graphs with the host kernel.

The matrices are the RBF matrices of test_svc.py.  Nothing here is compared
with a second copy of the code under test.

Rounding bounds.  A double sum of M terms in any order is within ``M eps
sum |terms|`` of the exact one.  ``q = z^T K z`` is a sum of at most N^2
terms, and the code under test may count the pairs (i, j) and (j, i) once
with weight 2: ``|dq| <= 2 N^2 eps sum_ij z_i |K_ij| z_j``.  ``u = z^T r``
and ``dz = z^T d`` are sums over at most N indices: ``|du| <= N eps sum_i
z_i sum_j |K_ij|`` and ``|ddz| <= N eps sum_i z_i |K_ii|``; ``t`` and ``dt``,
the same with z = 1.  The statistic is linear in the sums, with ``S_xx
= q``, ``S_xy = u - q``, ``S_yy = t - 2 u + q``: its bound is the first-order
propagation of these through the formula, times two for the roundings of the
formula itself (as test_alignment_gpu.py allows for its quotients)."""
import numpy as np
import pytest

import test_svc as svc

EPS = svc.EPS
GAMMA = 0.05
SIZES = [2, 3, 65, 257]
ESTIMATORS = ['biased', 'unbiased']


def _torch():
    import torch
    import graphdot_amd.model.two_sample  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


# -- the data and the definition -----------------------------------------------------
def stored(n, dtype=np.float64):
    """The matrix of test_svc.data rounded to `dtype` and widened again
    (what the code under test reads), and the labels."""
    K, _, lab, _ = svc.data(n, GAMMA)
    return K.astype(dtype).astype(np.float64), lab


def restated_splits(z0, B, seed):
    """The generator of the splits as the issue fixes it."""
    z0 = np.asarray(z0, dtype=np.uint8)
    Z = np.empty((B + 1, len(z0)), dtype=np.uint8)
    Z[0] = z0
    Z[1:] = np.random.default_rng(seed).permuted(np.tile(z0, (B, 1)), axis=1)
    return Z


def first_sizes(n):
    """First-sample sizes 1, n / 2 and n - 1."""
    return sorted({1, max(1, n // 2), n - 1})


def define_sums(K, Z):
    """(sums (rows, 3), their bounds, t, dt, bounds of t and dt) by numpy
    double on index sets."""
    N = len(K)
    A = np.abs(K)
    sums, bound = np.empty((len(Z), 3)), np.empty((len(Z), 3))
    r, d = K.sum(1), np.diag(K).copy()
    for b, z in enumerate(Z):
        x = np.flatnonzero(z)
        xx = np.ix_(x, x)
        sums[b] = K[xx].sum(), r[x].sum(), d[x].sum()
        bound[b] = (2 * N * N * EPS * A[xx].sum(),
                    N * EPS * A[x].sum(),
                    N * EPS * np.abs(d[x]).sum())
    return (sums, bound, K.sum(), d.sum(),
            (N * EPS * A.sum(), N * EPS * np.abs(d).sum()))


def define_mmd(K, z, estimator):
    """The squared MMD of one split: block means over index sets."""
    x, y = np.flatnonzero(z), np.flatnonzero(np.asarray(z) == 0)
    n, m = len(x), len(y)
    Kxx, Kyy, Kxy = K[np.ix_(x, x)], K[np.ix_(y, y)], K[np.ix_(x, y)]
    if estimator == 'biased':
        return Kxx.mean() + Kyy.mean() - 2 * Kxy.mean()
    return (Kxx.sum() - np.trace(Kxx)) / (n * (n - 1)) \
        + (Kyy.sum() - np.trace(Kyy)) / (m * (m - 1)) - 2 * Kxy.mean()


def statistic_bound(bound, tb, n, m, estimator):
    """The bound of the statistic of each split from the bounds (rows, 3) of
    its sums and `tb` of t and dt: first order, times two."""
    dq, du, ddz = bound[:, 0], bound[:, 1], bound[:, 2]
    dt, ddt = tb
    dxy, dyy = du + dq, dt + 2 * du + dq
    if estimator == 'biased':
        return 2 * (dq / n ** 2 + dyy / m ** 2 + 2 * dxy / (n * m))
    return 2 * ((dq + ddz) / (n * (n - 1)) + (dyy + ddt + ddz) / (m * (m - 1))
                + 2 * dxy / (n * m))


def worst(got, want, bound):
    """The largest share of its bound any value is off by (0 / 0 = 0)."""
    err = np.abs(np.asarray(got) - want)
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300),
                                 0.0), initial=0.0))


def check_sums(out, K, Z, s):
    """`forms` / `forms_torch` output against the definition; the worst share
    of a bound."""
    sums, r, d, w = (x.cpu().numpy() for x in out)
    want, bound, _, _, _ = define_sums(K, Z)
    N = len(K)
    assert sums.shape == (len(Z), 3)
    assert np.all(np.abs(sums - want) <= bound)
    A = np.abs(K)
    assert np.all(np.abs(r - K.sum(1)) <= N * EPS * A.sum(1))
    assert np.array_equal(d, np.diag(K))
    assert np.all(np.abs(w - K @ s) <= 2 * N * EPS * (A @ np.abs(s)))
    return worst(sums, want, bound)


def negative_strides():
    """A tensor class that reports negative strides (torch itself makes no
    such view): for the check of the launches' host side."""
    torch = _torch()

    class Reversed(torch.Tensor):
        def stride(self, *args):
            return (-self.shape[1], 1)
    return Reversed


def weights(z0):
    z0 = np.asarray(z0, dtype=bool)
    return np.where(z0, 1.0 / z0.sum(), -1.0 / (len(z0) - z0.sum()))


# -- the two forms of the issue agree with the definition ----------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', SIZES)
def test_restatement_against_the_definition(n, dtype):
    from graphdot_amd.model.two_sample import _mmd
    K, lab = stored(n, dtype)
    share = 0.0
    for n1 in first_sizes(n):
        z0 = np.arange(n) < n1
        Z = restated_splits(z0, 7, seed=n + n1)
        s = weights(z0)
        for layout in ('row-major', 'column-major'):
            A = _t(K.astype(dtype))
            if layout == 'column-major':
                A = A.t().contiguous().t()
            out = _mmd.forms_torch(A, _t(Z), _t(s))
            share = max(share, check_sums(out, K, Z, s))
        sums, bound, t, dt, tb = define_sums(K, Z)
        got = out[0].numpy()
        for estimator in ESTIMATORS:
            if estimator == 'unbiased' and (n1 < 2 or n - n1 < 2):
                with pytest.raises(ValueError, match='two points'):
                    _mmd.statistics(got, t, dt, n1, n - n1, estimator)
                continue
            stat = _mmd.statistics(got, out[1].sum().item(),
                                   out[2].sum().item(), n1, n - n1, estimator)
            want = np.array([define_mmd(K, z, estimator) for z in Z])
            sb = statistic_bound(bound, tb, n1, n - n1, estimator)
            assert stat.shape == (len(Z),)
            assert np.all(np.abs(stat - want) <= sb), (n1, estimator)
    print(f'n {n} {np.dtype(dtype).name}: the sums are off by at most '
          f'{share:.3g} of their bounds')


def test_splits():
    from graphdot_amd.model.two_sample import _mmd
    z0 = np.arange(65) % 3 == 0
    Z = _mmd.splits(z0, 50, seed=4)
    assert Z.dtype == np.uint8 and Z.shape == (51, 65)
    assert np.array_equal(Z[0], z0)
    assert np.all(Z.sum(1) == z0.sum()) and Z.max() == 1
    assert np.array_equal(Z, restated_splits(z0, 50, 4))
    assert np.array_equal(Z, _mmd.splits(z0.astype(np.uint8), 50, seed=4))
    assert not np.array_equal(Z, _mmd.splits(z0, 50, seed=5))
    assert len({z.tobytes() for z in Z}) > 45
    only = _mmd.splits(z0, 0, seed=4)
    assert only.shape == (1, 65) and np.array_equal(only[0], z0)


# -- the model on precomputed matrices -----------------------------------------------
def _model(**kwargs):
    from graphdot_amd.model.two_sample import KernelTwoSampleTest
    kwargs.setdefault('device', 'cpu')
    return KernelTwoSampleTest('precomputed', **kwargs)


def define_test(K, z0, B, seed, estimator):
    """(statistic, null, p-value) from the definition."""
    Z = restated_splits(z0, B, seed)
    stat = np.array([define_mmd(K, z, estimator) for z in Z])
    return stat[0], stat[1:], (1 + int(np.sum(stat[1:] >= stat[0]))) / (1 + B)


@pytest.mark.parametrize('estimator', ESTIMATORS)
@pytest.mark.parametrize('n', [65, 257])
def test_pvalue_of_the_label_split(n, estimator):
    """The split by the labels is as far from its null as a test of 999
    permutations can say: the p-value is 1 / 1000, and the nearest null value
    is 4e-2 away from the observed one -- no rounding decides a comparison."""
    K, lab = stored(n)
    m = _model(n_permutations=999, random_state=5, estimator=estimator)
    m.fit(K, lab == 0)
    stat, null, p = define_test(K, lab == 0, 999, 5, estimator)
    assert m.seed_ == 5 and m.null_.shape == (999,)
    assert m.n_ == (lab == 0).sum() and m.m_ == (lab != 0).sum()
    assert m.pvalue_ == (1 + np.sum(m.null_ >= m.statistic_)) / 1000
    assert p == 1 / 1000 and m.pvalue_ == p
    assert m.statistic_ == pytest.approx(stat, rel=1e-10)
    assert np.allclose(m.null_, null, rtol=0, atol=1e-10)
    assert m.reject() is True and m.reject(alpha=1e-4) is False
    assert m.last_timing['fused'] is False
    assert m.last_timing['adopted'] is False


def test_pvalue_of_the_half_split():
    """First half against second half of one sample, N = 257: p = 0.968 with
    the nearest null value 1.9e-5 from the observed one, against a bound near
    1e-11: the p-value equals the definition's exactly."""
    n = 257
    K, _ = stored(n)
    for Y in (n // 2, np.arange(n) < n // 2):
        m = _model(n_permutations=999, random_state=5).fit(K, Y)
        stat, null, p = define_test(K, np.arange(n) < n // 2, 999, 5,
                                    'unbiased')
        assert np.abs(null - stat).min() > 1e-6
        assert m.pvalue_ == p == 0.968
        assert m.pvalue_ == (1 + np.sum(m.null_ >= m.statistic_)) / 1000
        assert m.reject() is False
        assert m.statistic(K, Y) == m.statistic_
    # a tensor is worked on as it is, float storage included
    m32 = _model(n_permutations=99, random_state=5).fit(
        _t(K.astype(np.float32)), n // 2)
    assert m32.statistic_ == pytest.approx(stat, abs=1e-6)


def test_ties_count_as_greater_or_equal():
    """At N = 5 permutations reproduce the observed split: their statistics
    tie with it exactly, and count."""
    K, _ = stored(65)
    K = np.ascontiguousarray(K[:5, :5])
    z0 = np.array([1, 1, 0, 0, 0], dtype=bool)
    Z = restated_splits(z0, 99, 3)
    same = np.all(Z[1:] == Z[0], axis=1)
    assert same.sum() >= 3
    for estimator in ESTIMATORS:
        m = _model(n_permutations=99, random_state=3,
                   estimator=estimator).fit(K, z0)
        assert np.all(m.null_[same] == m.statistic_)
        _, _, p = define_test(K, z0, 99, 3, estimator)
        assert m.pvalue_ == (1 + np.sum(m.null_ >= m.statistic_)) / 100
        assert m.pvalue_ >= (1 + same.sum()) / 100
        # the distinct values of the null are far apart at this size
        assert m.pvalue_ == p


@pytest.mark.parametrize('n', [3, 65])
def test_witness(n):
    K, lab = stored(n)
    Ks = svc.data(n, GAMMA)[1]
    z0 = lab == 0
    s = weights(z0)
    m = _model(n_permutations=9, random_state=0, estimator='biased')
    m.fit(K, z0)
    A = np.abs(K)
    assert m.witness_.shape == (n,)
    assert np.all(np.abs(m.witness_ - K @ s)
                  <= 2 * n * EPS * (A @ np.abs(s)))
    # the biased statistic is the mean witness difference of the samples
    assert m.statistic_ == pytest.approx(s @ (K @ s), rel=1e-10)
    new = m.witness(Ks)
    assert new.shape == (svc.NEW,)
    assert np.all(np.abs(new - Ks @ s)
                  <= 2 * n * EPS * (np.abs(Ks) @ np.abs(s)))
    assert np.array_equal(m.witness(_t(Ks)), new)
    with pytest.raises(ValueError, match='shape'):
        m.witness(Ks[:, :-1])


def test_no_permutations_and_reject():
    K, lab = stored(65)
    m = _model(n_permutations=0).fit(K, lab == 0)
    assert m.pvalue_ is None and m.null_.shape == (0,)
    assert m.statistic_ == pytest.approx(
        define_mmd(K, lab == 0, 'unbiased'), rel=1e-10)
    assert m.witness_.shape == (65,)
    with pytest.raises(ValueError, match='reject'):
        m.reject()
    with pytest.raises(ValueError, match='reject'):
        _model().reject()
    # a seed is drawn once and kept where none is given
    a = _model(n_permutations=19).fit(K, lab == 0)
    b = _model(n_permutations=19, random_state=a.seed_).fit(K, lab == 0)
    assert np.array_equal(a.null_, b.null_)
    assert 0 < a.pvalue_ <= 1


def test_errors():
    from graphdot_amd.model.two_sample import KernelTwoSampleTest, _mmd
    torch = _torch()
    K, lab = stored(65)
    K, z0 = np.ascontiguousarray(K[:6, :6]), np.arange(6) < 3
    with pytest.raises(ValueError, match='estimator'):
        _model(estimator='linear')
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match='n_permutations'):
            _model(n_permutations=bad)
    for empty in (0, 6, np.zeros(6, dtype=bool), np.ones(6, dtype=bool)):
        with pytest.raises(ValueError, match='empty sample'):
            _model().fit(K, empty)
    for small in (1, 5):
        with pytest.raises(ValueError, match='two points'):
            _model().fit(K, small)
        assert np.isfinite(_model(estimator='biased', n_permutations=3)
                           .fit(K, small).statistic_)
    with pytest.raises(ValueError, match='square'):
        _model().fit(K[:, :4], 2)
    with pytest.raises(ValueError, match='length 6'):
        _model().fit(K, z0[:5])
    with pytest.raises(ValueError, match='membership'):
        _model().fit(K, np.arange(6))
    with pytest.raises(ValueError, match='first sample'):
        _model().fit(K, 7)
    for bad in (np.nan, np.inf):
        Kb = K.copy()
        Kb[2, 3] = Kb[3, 2] = bad
        with pytest.raises(ValueError, match='not finite'):
            _model().fit(Kb, z0)
    with pytest.raises(ValueError, match='before fit'):
        _model().witness(K)
    with pytest.raises(ValueError, match='empty sample'):
        KernelTwoSampleTest(lambda X, Y=None: None, device='cpu').fit(
            [], [1, 2])
    # the launches' host side checks its arguments on any device
    Kt, Z, s = _t(K), _t(_mmd.splits(z0, 4, 0)), _t(weights(z0))
    with pytest.raises(TypeError, match='CUDA'):
        _mmd.forms(Kt, Z, s)
    with pytest.raises(TypeError, match='K'):
        _mmd.forms_torch(Kt[:, :4], Z, s)
    with pytest.raises(TypeError, match='K'):
        _mmd.forms_torch(Kt.to(torch.float16), Z, s)
    with pytest.raises(TypeError, match='Z'):
        _mmd.forms_torch(Kt, Z.to(torch.float64), s)
    with pytest.raises(TypeError, match='Z'):
        _mmd.forms_torch(Kt, Z[:, :5], s)
    with pytest.raises(TypeError, match='Z'):
        _mmd.forms_torch(Kt, Z[:0], s)
    with pytest.raises(TypeError, match='Z'):
        _mmd.forms_torch(Kt, Z[0], s)
    with pytest.raises(TypeError, match='s'):
        _mmd.forms_torch(Kt, Z, s.float())
    with pytest.raises(ValueError, match='negative strides'):
        _mmd.forms_torch(Kt.as_subclass(negative_strides()), Z, s)
    with pytest.raises(ValueError, match='not finite'):
        _mmd.statistics(np.zeros((1, 3)), np.inf, 1.0, 3, 3, 'biased')
    with pytest.raises(ValueError, match='not finite'):
        _mmd.statistics(np.zeros((1, 3)), 1.0, np.nan, 3, 3, 'biased')
    with pytest.raises(ValueError, match='estimator'):
        _mmd.statistics(np.zeros((1, 3)), 1.0, 1.0, 3, 3, 'linear')
    out, fused = _mmd.solve(Kt, Z, s)
    assert fused is False and out[0].shape == (5, 3)


# -- a graph kernel on the host --------------------------------------------------------
def test_graph_kernel_on_the_host():
    """Ten small graphs, the five smallest against the five largest, with the
    host kernel: the model against the definition on the kernel's matrix of
    the pooled graphs."""
    import test_alignment as ta
    from graphdot_amd.model.two_sample import KernelTwoSampleTest
    kernel, G, _, size = ta.graph_case()
    theta0 = np.array(kernel.theta)
    order = np.argsort(size, kind='stable')
    X, Y = G[order[:5]], G[order[5:]]
    K = np.asarray(kernel(np.concatenate((X, Y))), dtype=np.float64)
    z0 = np.arange(10) < 5
    for estimator in ESTIMATORS:
        m = KernelTwoSampleTest(kernel, n_permutations=49, random_state=1,
                                estimator=estimator, device='cpu').fit(X, Y)
        stat, null, p = define_test(K, z0, 49, 1, estimator)
        assert (m.n_, m.m_) == (5, 5)
        assert m.statistic_ == pytest.approx(stat, rel=1e-9, abs=1e-13)
        assert np.allclose(m.null_, null, rtol=0, atol=1e-12)
        assert m.pvalue_ == (1 + np.sum(m.null_ >= m.statistic_)) / 50
        assert m.statistic(X, Y) == m.statistic_
        assert m.last_timing['fused'] is False
        assert m.last_timing['adopted'] is False
    print(f'statistic {m.statistic_:.6g}, p {m.pvalue_:.3g} (definition {p})')
    # the witness at the pooled graphs themselves is witness_ (the plain
    # kernel: a cross matrix needs no diagonal)
    plain = KernelTwoSampleTest(kernel.kernel, n_permutations=0,
                                device='cpu').fit(X, Y)
    assert np.allclose(plain.witness(np.concatenate((X, Y))),
                       plain.witness_, rtol=0,
                       atol=1e-10 * np.abs(plain.witness_).max())
    # a sample against itself in another order: a statistic near zero
    same = KernelTwoSampleTest(kernel, n_permutations=0, estimator='biased',
                               device='cpu').fit(X, X[::-1])
    assert abs(same.statistic_) <= 1e-12
    assert np.array_equal(kernel.theta, theta0)
