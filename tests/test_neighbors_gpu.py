"""The device path of the neighbour models on an MI355X: `knn_topk_*` and
`knn_merge` against the definition of the lists in numpy (test_neighbors.py:
its definition, its data and its rounding bounds) on the stored matrix widened
to double, with equal indices and equal bits of d2, for float and double
storage, both layouts and every split of the columns; `knn_average`,
`knn_lrd` and `knn_ratio` against the torch restatements on the same device
tensors; the flag word; the arguments; and the four models on the HIP backend
against the restatement on the very matrices they worked on -- no host kernel
evaluation.

The edges of the launch shapes.  Rows b: one row, two, the strip of 32 on
both sides (31, 32, 33) and three strips (65).  Columns n: one and two, the
tile of 64 on both sides (63, 64, 65) and several tiles (129, 257: five
tiles, so that of 7 parts two are empty; with n <= 64 all parts but the
first are).  k: 1, 2, and the list's 64 lanes on both sides of full (63, 64),
clipped to the number of candidates.  The data have many d2 clamped to zero,
so that the column decides in every list."""
import numpy as np
import pytest

import test_neighbors as cpu

pytestmark = pytest.mark.gpu

EPS = cpu.EPS
ROWS = [1, 2, 31, 32, 33, 65]
COLUMNS = [1, 2, 63, 64, 65, 129, 257]
SQUARES = [2, 33, 64, 65, 129]
KS = [1, 2, 63, 64]
PARTS = [1, 2, 3, 7]


def _torch():
    import torch
    import graphdot_amd.model.neighbors  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


def _matrix(K, layout):
    """K on the device, contiguous along the index `layout` names."""
    A = _t(K).cuda()
    return A.t().contiguous().t() if layout == 'column-major' else A


def _random(b, n, seed, dtype):
    """(K (b, n) as stored, dq, dt): about one d2 in six is negative before
    the clamp, and those tie at zero."""
    rng = np.random.default_rng(seed)
    K = rng.normal(size=(b, n)).astype(dtype)
    dt = rng.uniform(0.5, 1.5, size=n)
    dq = dt.copy() if b == n else rng.uniform(0.5, 1.5, size=b)
    return K, dq, dt


def _same(got, want2, want):
    torch = _torch()
    d2, idx, flag = got
    return d2.dtype == torch.float64 and idx.dtype == torch.int64 \
        and torch.equal(idx, want) \
        and torch.equal(d2.view(torch.int64), want2.view(torch.int64)) \
        and int(flag) == 0


def _check(K, dq, dt, exclude_self, ks=KS, parts=PARTS):
    """Every k, layout and split of one stored matrix against the
    definition; the number of launches."""
    from graphdot_amd.model.neighbors import _knn
    b, n = K.shape
    most = n - 1 if exclude_self else n
    dqd, dtd = _t(dq).cuda(), _t(dt).cuda()
    launches = 0
    for k in sorted({min(k, most) for k in ks} - {0}):
        want2, want = cpu.define_topk(K, dq, dt, k, exclude_self)
        want2, want = _t(want2).cuda(), _t(want).cuda()
        for layout in ('row-major', 'column-major'):
            Kd = _matrix(K, layout)
            if b > 1 and n > 1:
                assert Kd.stride() == ((n, 1) if layout == 'row-major'
                                       else (1, b))
            for p in [None] + parts:
                got = _knn.topk(Kd, dqd, dtd, k, exclude_self, p)
                assert _same(got, want2, want), \
                    (b, n, k, layout, p, exclude_self)
                launches += 1
    return launches


# -- 1. the search against the definition ----------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', COLUMNS)
def test_search_against_the_definition(n, dtype):
    zeros = 0
    for b in ROWS:
        K, dq, dt = _random(b, n, 100 * b + n, dtype)
        zeros += (cpu.define_d2(K, dq, dt) == 0.0).sum()
        _check(K, dq, dt, False)
    assert zeros > len(ROWS) or n < 63


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', SQUARES)
def test_search_that_leaves_the_sample_out(n, dtype):
    K, dq, dt = _random(n, n, n, dtype)
    _check(K, dq, dt, True)
    _check(K, dq, dt, False, ks=[1, 64])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_search_on_tied_data(dtype):
    for b, n in ((33, 257), (65, 65)):
        K, dq, dt = cpu.tied(b, n, seed=b + n, dtype=dtype)
        _check(K, dq, dt, False)
        if b == n:
            _check(K, dq, dt, True)
    K, d = cpu.duplicated(129, seed=5, dtype=dtype)
    assert (cpu.define_d2(K, d, d) == 0.0).sum() >= 129 + 2 * 42
    _check(K, d, d, False)
    _check(K, d, d, True)


def test_search_twice_and_in_any_company():
    """The same bits from a second call, and for a row whatever the other
    rows are: the lists of a row depend on that row's data alone."""
    from graphdot_amd.model.neighbors import _knn
    torch = _torch()
    K, dq, dt = _random(65, 257, 7, np.float64)
    Kd, dqd, dtd = _t(K).cuda(), _t(dq).cuda(), _t(dt).cuda()
    for k in (1, 64):
        one = _knn.topk(Kd, dqd, dtd, k)
        two = _knn.topk(Kd, dqd, dtd, k)
        for x, y in zip(one, two):
            assert torch.equal(x, y)
        for rows in ([40], [64, 3, 33], list(range(31, 65))):
            part = _knn.topk(Kd[rows], dqd[rows], dtd, k, parts=2)
            assert torch.equal(part[1], one[1][rows])
            assert torch.equal(part[0].view(torch.int64),
                               one[0][rows].view(torch.int64))
    # a strided matrix is read as it is
    big = torch.zeros((130, 514), dtype=torch.float64, device='cuda')
    big[::2, ::2] = Kd
    for x, y in zip(_knn.topk(big[::2, ::2], dqd, dtd, 5),
                    _knn.topk(Kd, dqd, dtd, 5)):
        assert torch.equal(x, y)


# -- 2. what is made of the lists ------------------------------------------------------
@pytest.mark.parametrize('k', [1, 64])
def test_sums_over_the_lists_against_the_restatement(k):
    from graphdot_amd.model.neighbors import _knn
    torch = _torch()
    n = 129
    K, d = cpu.duplicated(n, seed=11)
    Kd, dd = _t(K).cuda(), _t(d).cuda()
    rng = np.random.default_rng(k)
    share = 0.0
    for exclude_self in (False, True):
        d2, idx, _ = _knn.topk(Kd, dd, dd, k, exclude_self)
        zeros = (d2 == 0.0).sum(1)
        # lists with one zero distance, with two and (left out) with none
        assert set(zeros.cpu().tolist()) == (
            {0, 1} if exclude_self else {1} if k == 1 else {1, 2})
        for m in (1, 3, 17):
            T = _t(rng.normal(size=(n, m))).cuda()
            for weights in _knn.WEIGHTS:
                got, fused = _knn.mean(d2, idx, T, weights)
                assert fused is True and got.shape == (n, m)
                want = _knn.average_torch(d2, idx, T, weights)
                err = (got - want).abs().max().item()
                lim = cpu.bound(k, cpu.C_MEAN, T.abs().max().item())
                share = max(share, err / lim)
                assert err <= lim, (k, m, weights, exclude_self)
        kdist = _t(rng.uniform(0.0, 1.0, size=n)).cuda()
        got, want = _knn.lrd(d2, idx, kdist), _knn.lrd_torch(d2, idx, kdist)
        assert torch.all((got - want).abs()
                         <= cpu.bound(k, cpu.C_MEAN, 1.0) * want.abs())
        train = _t(rng.uniform(0.5, 2.0, size=n)).cuda()
        lof = _knn.ratio(idx, train, got)
        want = _knn.ratio_torch(idx, train, got)
        assert torch.all((lof - want).abs()
                         <= cpu.bound(k, cpu.C_LOF, 1.0) * want.abs())
        (lof, own), fused = _knn.factors(d2, idx, kdist, train)
        assert fused is True and torch.equal(own, got)
    print(f'k {k}: the means are off by at most {share:.3g} of their bound')


# -- 3. the flag -----------------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_entries_that_are_not_finite(bad):
    from graphdot_amd.model.neighbors import (
        KernelLocalOutlierFactor, KernelNearestNeighbors, _knn)
    K, Ks, dt, dq, _, _ = cpu.continuous(70, 33, seed=0)
    m = KernelNearestNeighbors('precomputed', 3, device='cuda').fit(
        _t(K).cuda())
    want = cpu.define_topk(Ks, dq, dt, 3)
    d, idx = m.kneighbors(_t(Ks).cuda(), diag=dq)
    assert m.last_timing['fused'] is True
    assert np.array_equal(idx, want[1])
    assert np.array_equal(d, np.sqrt(want[0]))
    Kb = Ks.copy()
    Kb[32, 69] = bad
    with pytest.raises(ValueError, match='not finite'):
        m.kneighbors(_t(Kb).cuda(), diag=dq)
    assert m.last_timing['fused'] is True
    db = dq.copy()
    db[5] = bad
    with pytest.raises(ValueError, match='not finite'):
        m.kneighbors(_t(Ks).cuda(), diag=db)
    Kb = K.copy()
    Kb[40, 3] = Kb[3, 40] = bad
    with pytest.raises(ValueError, match='not finite'):
        KernelLocalOutlierFactor('precomputed', 3, device='cuda').fit(
            _t(Kb).cuda())
    Kb = K.copy()
    Kb[9, 9] = bad                           # a training self-similarity
    with pytest.raises(ValueError, match='not finite'):
        KernelNearestNeighbors('precomputed', 3, device='cuda').fit(
            _t(Kb).cuda()).kneighbors(_t(Ks).cuda(), diag=dq)
    # the flag itself, with the columns split
    for p in (1, 3):
        flag = _knn.topk(_t(Kb).cuda(), _t(np.diag(Kb).copy()),
                         _t(np.diag(Kb).copy()), 3, True, p)[2]
        assert int(flag) == 1


# -- 4. arguments ------------------------------------------------------------------------
def test_launches_check_their_arguments():
    import test_two_sample as two
    from graphdot_amd.model.neighbors import _knn
    torch = _torch()
    K, dq, dt = _random(33, 129, 3, np.float64)
    Kd, dqd, dtd = _t(K).cuda(), _t(dq).cuda(), _t(dt).cuda()
    # more neighbours than the lists hold: the torch chain, the same lists
    (d2, idx, flag), fused = _knn.search(Kd, dqd, dtd, 65)
    assert fused is False and d2.is_cuda
    want2, want = cpu.define_topk(K, dq, dt, 65)
    assert _same((d2, idx, flag), _t(want2).cuda(), _t(want).cuda())
    (d2, idx, flag), fused = _knn.search(Kd, dqd, dtd, 64)
    assert fused is True
    assert _same((d2, idx, flag), _t(want2[:, :64]).cuda(),
                 _t(want[:, :64]).cuda())
    out, fused = _knn.search(Kd.cpu(), dqd, dtd, 5)
    assert fused is False and not out[0].is_cuda
    with pytest.raises(ValueError, match='64 at the most'):
        _knn.topk(Kd, dqd, dtd, 65)
    with pytest.raises(TypeError, match='CUDA'):
        _knn.topk(Kd.cpu(), dqd, dtd, 5)
    with pytest.raises(TypeError, match='Ks'):
        _knn.topk(Kd.to(torch.float16), dqd, dtd, 5)
    with pytest.raises(TypeError, match='Ks'):
        _knn.topk(Kd[0], dqd, dtd, 5)
    with pytest.raises(TypeError, match='dq'):
        _knn.topk(Kd, dqd.to(torch.float32), dtd, 5)
    with pytest.raises(TypeError, match='dq'):
        _knn.topk(Kd, dqd[:5], dtd, 5)
    with pytest.raises(TypeError, match='dt'):
        _knn.topk(Kd, dqd, dtd[:5], 5)
    with pytest.raises(ValueError, match='negative strides'):
        _knn.topk(Kd.as_subclass(two.negative_strides()), dqd, dtd, 5)
    with pytest.raises(ValueError, match='exceeds'):
        _knn.topk(Kd[:, :4], dqd, dtd[:4], 5)
    with pytest.raises(ValueError, match='square'):
        _knn.topk(Kd, dqd, dtd, 5, exclude_self=True)
    with pytest.raises(ValueError, match='parts'):
        _knn.topk(Kd, dqd, dtd, 5, parts=0)
    d2, idx, _ = _knn.topk(Kd, dqd, dtd, 5)
    T = _t(np.ones((129, 2))).cuda()
    with pytest.raises(TypeError, match='lists'):
        _knn.average(d2, idx.to(torch.int32), T)
    with pytest.raises(TypeError, match='lists'):
        _knn.average(d2.to(torch.float32), idx, T)
    with pytest.raises(TypeError, match='T'):
        _knn.average(d2, idx, T.to(torch.float32))
    with pytest.raises(ValueError, match='weights'):
        _knn.average(d2, idx, T, 'rank')
    with pytest.raises(TypeError, match='kdist'):
        _knn.lrd(d2, idx, T)
    with pytest.raises(TypeError, match='idx'):
        _knn.ratio(idx.to(torch.int32), T[:, 0], T[:33, 0])
    with pytest.raises(TypeError, match='lrd_rows'):
        _knn.ratio(idx, T[:, 0].contiguous(), T[:5, 0].contiguous())
    # dq and dt from the host, and no rows at all
    a = _knn.topk(Kd, dqd.cpu(), dtd.cpu(), 5)
    assert torch.equal(a[1], idx)
    none = _knn.topk(Kd[:0], dqd[:0], dtd, 5)
    assert none[0].shape == none[1].shape == (0, 5)


# -- 5. the models on QM7-like graphs --------------------------------------------------
N_TRAIN, N_NEW, K_GRAPHS = 40, 8, 3


def _graphs():
    import cases
    G = np.asarray(list(cases.config3_graphs(N_TRAIN + N_NEW, seed=29)),
                   dtype=object)
    return G[:N_TRAIN], G[N_TRAIN:]


def _kernel(real):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    knode, kedge, q = cases.config3_fit_kernels()
    return Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, q_bounds=(1e-3, 0.5),
        backend=HIPBackend(real=real),
        ftol=1e-13 if real is np.float64 else 1e-8))


@pytest.mark.parametrize('real', [np.float32, np.float64])
def test_models_on_the_device_path(real, monkeypatch):
    """The four models against the restatement on the CPU (a model of the
    precomputed kernel with ``device='cpu'``) on the very matrices the device
    path worked on: adopted again from `device_gram`, `device_cross_gram` and
    `device_diag` and downloaded here, for the test.  No tolerance on
    indices."""
    from graphdot_amd.model.neighbors import (
        KernelKNeighborsClassifier, KernelKNeighborsRegressor,
        KernelLocalOutlierFactor, KernelNearestNeighbors)
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G, Z = _graphs()
    k = K_GRAPHS
    kernel = _kernel(real)
    theta0 = np.array(kernel.theta)
    K = torch.as_tensor(kernel.device_gram(G), device='cuda').cpu().numpy()
    Ks = torch.as_tensor(kernel.device_cross_gram(Z, G),
                         device='cuda').cpu().numpy()
    dz = torch.as_tensor(kernel.device_diag(Z), device='cuda').cpu().numpy()
    size = np.array([float(len(g.nodes)) for g in G])
    lab = [('heavy' if s > np.median(size) else 'light') for s in size]
    calls = []

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
        monkeypatch.setattr(cls, 'diag', counting)

    def on_device(model):
        assert model.last_timing['adopted'] is True
        assert model.last_timing['fused'] is True

    dev = KernelNearestNeighbors(kernel, k, device='cuda').fit(G)
    on_device(dev)
    host = KernelNearestNeighbors('precomputed', k, device='cpu').fit(K)
    for got, want in ((dev.kneighbors(Z), host.kneighbors(Ks, diag=dz)),
                      (dev.kneighbors(), host.kneighbors()),
                      (dev.kneighbors(Z, N_TRAIN),
                       host.kneighbors(Ks, N_TRAIN, diag=dz))):
        on_device(dev)
        assert np.array_equal(got[1], want[1])
        assert np.array_equal(got[0], want[0])
    for weights in ('uniform', 'distance'):
        dev = KernelKNeighborsClassifier(kernel, k, weights,
                                         device='cuda').fit(G, lab)
        on_device(dev)
        host = KernelKNeighborsClassifier('precomputed', k, weights,
                                          device='cpu').fit(K, lab)
        got, want = dev.predict_proba(Z), host.predict_proba(Ks, diag=dz)
        on_device(dev)
        assert np.all(np.abs(got - want) <= cpu.bound(k, cpu.C_MEAN, 1.0))
        top = np.sort(want, axis=1)
        assert np.all(top[:, -1] - top[:, -2] > cpu.bound(k, cpu.C_MEAN, 1.0))
        assert dev.predict(Z).tolist() == host.predict(Ks, diag=dz).tolist()
        assert dev.loo_score() == host.loo_score()
        on_device(dev)
        for y in (size, np.stack((size, np.sqrt(size)), axis=1)):
            dev = KernelKNeighborsRegressor(kernel, k, weights,
                                            device='cuda').fit(G, y)
            host = KernelKNeighborsRegressor('precomputed', k, weights,
                                             device='cpu').fit(K, y)
            got, want = dev.predict(Z), host.predict(Ks, diag=dz)
            on_device(dev)
            assert got.shape == want.shape == (N_NEW,) + y.shape[1:]
            assert np.all(np.abs(got - want)
                          <= cpu.bound(k, cpu.C_MEAN, np.abs(y).max()))
            assert dev.loo_score() == pytest.approx(host.loo_score(),
                                                    rel=1e-12)
    dev = KernelLocalOutlierFactor(kernel, 2 * k, device='cuda').fit(G)
    on_device(dev)
    host = KernelLocalOutlierFactor('precomputed', 2 * k, device='cpu').fit(K)
    for got, want in ((dev.negative_outlier_factor_,
                       host.negative_outlier_factor_),
                      (dev.score_samples(Z),
                       host.score_samples(Ks, diag=dz))):
        on_device(dev)
        assert np.all(np.abs(got - want)
                      <= cpu.bound(2 * k, cpu.C_LOF, np.abs(want)))
    print(f'{real.__name__}: outlier factors of at most '
          f'{-dev.negative_outlier_factor_.min():.3g}, of the new graphs '
          f'{-got.min():.3g}')
    assert np.array_equal(kernel.theta, theta0)
    assert calls == []
