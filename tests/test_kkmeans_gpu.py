"""The device path of KernelKMeans on an MI355X: every launch of lloyd.hip
against its torch restatement (run in double on the CPU) on the same stored
inputs (tile, wave and block edges, every register chunk and the passes above
16 clusters, one and three restarts, f32 / f64 matrices in both layouts,
bit-identical repeats), the seeding on its defining properties, the whole fit
with the assertions and matrices of test_kkmeans.py, and the model on the HIP
backend against the same model on the host given the downloaded matrices, with
no host kernel evaluation and no n x n download on the device path.

Every bound is derived: either side's sum of n terms is within ``(n - 1) eps
sum |terms|`` of the exact one whatever its order (contraction to FMA only
removes roundings), so two sides differ by ``2 n eps sum |terms|``; a sum over
such sums adds the same again."""
import warnings
import numpy as np
import pytest

import test_kkmeans as cpu

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SIZES = [2, 3, 63, 64, 65, 257, 1000]
CLUSTERS = [1, 2, 9, 16, 17, 64]
NK = [(n, k) for n in SIZES for k in CLUSTERS if k <= n]
RESTARTS = [1, 3]
#: the share of samples a case may leave out because the reference's own gap
#: between the best and the second-best cluster is within the bound on d2
LEFT_OUT = 0.01


def _torch():
    import torch
    import graphdot_amd.model.clustering  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


def _matrix(K, dtype, layout):
    """K stored as `dtype`, contiguous along the index `layout` names; the
    values both sides then work on."""
    A = _t(K.astype(dtype))
    return A.t().contiguous().t() if layout == 'column-major' else A


_inputs = {}


def _case(n, k, R):
    """(K, labels (R, n) int32): a blob matrix and random labels -- computed
    once (with 64 clusters some are empty)."""
    if (n, k, R) not in _inputs:
        K = cpu.blobs(n, min(k, 17), 7)[1]
        lab = np.random.default_rng(100 * n + k).integers(
            0, k, (R, n)).astype(np.int32)
        _inputs[n, k, R] = (K, lab)
    return _inputs[n, k, R]


def _twice(fn, *args):
    torch = _torch()
    a, b = fn(*args), fn(*args)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)                  # bit-identical repeats
    return [x.cpu().numpy() for x in a]


def _same_argmin(got, D, bound, what):
    """`got` equals the argmin of the reference distances D (..., k) at every
    point whose gap between the best and the second-best exceeds twice the
    largest bound on its distances; at most LEFT_OUT of the points do not."""
    want = D.argmin(-1)
    if D.shape[-1] == 1:
        assert np.array_equal(got, want)
        return
    two = np.sort(D, axis=-1)[..., :2]
    with np.errstate(invalid='ignore'):
        gap = np.where(np.isinf(two[..., 1]), np.inf, two[..., 1] - two[..., 0])
    sure = gap > 2 * np.where(np.isfinite(D), bound, 0).max(-1)
    print(f'{what}: {int((~sure).sum())} of {sure.size} points left out')
    assert (~sure).mean() <= LEFT_OUT
    assert np.array_equal(got[sure], want[sure])


# -- the launches against their restatements ------------------------------------------
@pytest.mark.parametrize('layout', ['row-major', 'column-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n,k', NK)
def test_accumulate_against_restatement(n, k, dtype, layout):
    """``|S - S_ref| <= 2 n eps (|K| Z)``; T is one more sum over S, ``4 n
    eps`` of the same terms; the counts are integers and exact."""
    from graphdot_amd.model.clustering import _lloyd
    for R in RESTARTS:
        K, lab = _case(n, k, R)
        Kt = _matrix(K, dtype, layout)
        assert n == 1 or Kt.stride(0 if layout == 'column-major' else 1) == 1
        stored = Kt.to(_torch().float64).numpy()
        rS, rpart = (x.numpy() for x in _lloyd.accumulate_torch(
            _t(stored), _t(lab), k))
        S, part = _twice(_lloyd.accumulate, Kt.cuda(), _t(lab).cuda(), k)
        kc, nch, nrb, nab = _lloyd.grid(n, k)
        assert S.shape == (R, n, k) and part.shape == (R, nrb, 2 * k)
        Z = (lab[:, :, None] == np.arange(k)).astype(np.float64)
        size = np.einsum('ij,rjc->ric', np.abs(stored), Z)
        assert np.all(np.abs(S - rS) <= 2 * n * EPS * size)
        tot = part.sum(1)
        assert np.array_equal(tot[:, k:], rpart[:, 0, k:])
        assert np.array_equal(tot[:, k:], Z.sum(1))
        assert np.all(np.abs(tot[:, :k] - rpart[:, 0, :k])
                      <= 4 * n * EPS * (size * Z).sum(1))


@pytest.mark.parametrize('layout', ['row-major', 'column-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n,k', NK)
def test_assign_against_restatement(n, k, dtype, layout):
    """Both sides are given the same S and the same shares (three row
    blocks, whose sums are exact): ``d2 = K_ii - 2 S / n_c + T / n_c^2`` then
    carries a few roundings of its terms, ``4 eps (|K_ii| + 2 |S| / n_c + |T|
    / n_c^2)`` over both sides.  The inertia is a sum of n such terms."""
    from graphdot_amd.model.clustering import _lloyd
    torch = _torch()
    for R in RESTARTS:
        K, lab = _case(n, k, R)
        Kt = _matrix(K, dtype, layout)
        stored = Kt.to(torch.float64)
        S, part = _lloyd.accumulate_torch(stored, _t(lab), k)
        part = (part * _t(np.array([0.5, 0.25, 0.25]))[None, :, None]) \
            .contiguous()
        assert torch.equal(part.sum(1)[:, k:],
                           _t((lab[:, :, None] == np.arange(k)).sum(1))
                           .to(torch.float64))
        rnext, rapart = (x.numpy() for x in _lloyd.assign_torch(
            stored, _t(lab), S, part))
        nxt, apart = _twice(_lloyd.assign, Kt.cuda(), _t(lab).cuda(),
                            S.cuda(), part.cuda())
        nab = _lloyd.grid(n, k)[3]
        assert nxt.shape == (R, n) and apart.shape == (R, 3, nab)
        T, counts = (x.numpy() for x in _lloyd.totals_torch(part))
        diag = np.abs(np.diagonal(stored.numpy()))
        D = _lloyd.distances_torch(stored.diagonal(), S, _t(T),
                                   _t(counts)).numpy()
        with np.errstate(divide='ignore', invalid='ignore'):
            bound = 4 * EPS * (
                diag[None, :, None]
                + 2 * np.abs(S.numpy()) / counts[:, None, :]
                + (np.abs(T) / counts ** 2)[:, None, :])
        assert np.all(counts[np.arange(R)[:, None], nxt] > 0)
        _same_argmin(nxt, D, bound, f'assign {n} {k} {R}')
        tot = apart.sum(2)
        assert np.array_equal(tot[:, 0], (nxt != lab).sum(1))
        assert np.all(tot[:, 2] == 0)
        own = np.take_along_axis(np.abs(S.numpy()), lab[:, :, None].astype(
            np.int64), 2)[:, :, 0] / np.take_along_axis(
                counts, lab.astype(np.int64), 1)
        assert np.all(np.abs(tot[:, 1] - rapart[:, 1, 0])
                      <= 2 * (n + 4) * EPS * (diag[None, :] + own).sum(1))


def test_reduce_against_restatement():
    """The sums, the sticky status and the stamp of the first round without
    a change."""
    from graphdot_amd.model.clustering import _lloyd
    torch = _torch()
    rng = np.random.default_rng(5)
    R, nab = 4, 300
    apart = np.zeros((R, 3, nab))
    apart[:, 1] = rng.normal(size=(R, nab)) + 2.0
    apart[1, 0, 17] = 3.0                 # restart 1 changes three labels
    apart[2, 2, 299] = 1.0                # restart 2 meets a NaN
    later = apart.copy()
    later[1, 0] = 0.0
    later[2, 2] = 0.0
    info_d = torch.zeros((R, 4), dtype=torch.float64).cuda()
    info_h = torch.zeros((R, 4), dtype=torch.float64)
    for rnd, a in ((5, apart), (6, later), (7, later)):
        _lloyd.reduce(_t(a).cuda(), info_d, rnd)
        _lloyd.reduce_torch(_t(a), info_h, rnd)
        got, want = info_d.cpu().numpy(), info_h.numpy()
        assert np.array_equal(got[:, [0, 2, 3]], want[:, [0, 2, 3]])
        assert np.all(np.abs(got[:, 1] - want[:, 1])
                      <= 2 * nab * EPS * np.abs(a[:, 1]).sum(1))
    assert got[:, 3].tolist() == [5, 6, 0, 5] and got[:, 2].tolist() \
        == [0, 0, 1, 0]


@pytest.mark.parametrize('layout', ['row-major', 'column-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('init', ['k-means++', 'farthest'])
@pytest.mark.parametrize('n,k', NK)
def test_seeding_properties(n, k, init, dtype, layout):
    """The properties of test_kkmeans.check_seeding on what the kernel
    returned, for the stored values."""
    from graphdot_amd.model.clustering import _lloyd
    K = _case(n, k, 1)[0]
    Kt = _matrix(K, dtype, layout)
    stored = Kt.to(_torch().float64).numpy()
    u = np.random.default_rng(n + k).random((3, k))
    u[2, 0] = 1 - 2.0 ** -53              # (the last sample)
    seeds, lab, mind = _twice(
        lambda: _lloyd.seed(Kt.cuda(), k, init, u))
    assert seeds.shape == (3, k) and lab.shape == mind.shape == (3, n)
    cpu.check_seeding(stored, k, init, u, seeds, lab, mind)


def test_given_seeds_and_coincident_samples():
    from graphdot_amd.model.clustering import _lloyd
    n, k = 65, 9
    K = _case(n, k, 1)[0]
    given = np.stack([np.random.default_rng(r).choice(n, k, replace=False)
                      for r in range(3)])
    seeds, lab, mind = _twice(
        lambda: _lloyd.seed(_t(K).cuda(), k, 'given', seeds=given))
    assert np.array_equal(seeds, given)
    cpu.check_seeding(K, k, 'given', None, seeds, lab, mind)
    u = np.array([[0.5, 0.9, 0.1]])
    ones = np.ones((7, 7))
    seeds, lab, mind = _twice(
        lambda: _lloyd.seed(_t(ones).cuda(), 3, 'k-means++', u))
    assert seeds.tolist() == [[3, 0, 1]]
    cpu.check_seeding(ones, 3, 'k-means++', u, seeds, lab, mind)


@pytest.mark.parametrize('layout', ['column-major', 'row-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('k', [1, 2, 16, 17, 64])
@pytest.mark.parametrize('b', [1, 5, 64, 65])
def test_predict_against_restatement(b, k, dtype, layout):
    """``D = -2 S_zc / n_c + T_c / n_c^2``: a sum of n terms per side and a
    few roundings, ``4 (n + 4) eps (|Ks| Z / n_c + |T_c| / n_c^2)``."""
    from graphdot_amd.model.clustering import _lloyd
    torch = _torch()
    n = 257
    rng = np.random.default_rng(100 * b + k)
    Ks = rng.normal(size=(b, n)) + 0.7
    lab = rng.integers(0, k, n).astype(np.int32)
    counts = np.bincount(lab, minlength=k).astype(np.float64)
    T = rng.uniform(0.5, 2.0, size=k) * counts ** 2
    Kt = _t(Ks.astype(dtype))
    if layout == 'column-major':               # z + i b, as the solver leaves it
        Kt = Kt.t().contiguous().t()
    stored = Kt.to(torch.float64).numpy()
    rD, rarg = (x.numpy() for x in _lloyd.predict_torch(
        _t(stored), _t(lab), _t(T), _t(counts)))
    D, arg = _twice(_lloyd.predict, Kt.cuda(), _t(lab).cuda(), _t(T).cuda(),
                    _t(counts).cuda())
    assert D.shape == rD.shape == (b, k) and arg.shape == (b,)
    Z = (lab[:, None] == np.arange(k)).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        bound = 4 * (n + 4) * EPS * (np.abs(stored) @ Z / counts
                                     + np.abs(T) / counts ** 2)
    empty = counts == 0
    assert np.all(np.isinf(D[:, empty])) and np.all(np.isinf(rD[:, empty]))
    assert np.all(np.abs(D[:, ~empty] - rD[:, ~empty]) <= bound[:, ~empty])
    _same_argmin(arg, rD, bound, f'predict {b} {k}')


def test_launches_check_their_arguments():
    torch = _torch()
    from graphdot_amd.model.clustering import _lloyd
    n, k = 8, 3
    K = torch.eye(n, dtype=torch.float64, device='cuda')
    lab = torch.zeros((1, n), dtype=torch.int32, device='cuda')
    S, part = _lloyd.accumulate(K, lab, k)
    with pytest.raises(TypeError):
        _lloyd.accumulate(K.cpu(), lab, k)
    with pytest.raises(TypeError):
        _lloyd.accumulate(K.to(torch.float16), lab, k)
    with pytest.raises(ValueError):
        _lloyd.accumulate(K[:, ::2][:4], lab[:, :4], k)     # strided
    with pytest.raises(TypeError):
        _lloyd.accumulate(K, lab.long(), k)
    with pytest.raises(ValueError):
        _lloyd.accumulate(K, lab[:, :4], k)
    with pytest.raises(ValueError):
        _lloyd.accumulate(K, lab, 9)
    with pytest.raises(ValueError):
        _lloyd.assign(K, lab, S, part, (lab, torch.empty(
            (1, 3, 1), dtype=torch.float64, device='cuda')))
    with pytest.raises(TypeError):
        _lloyd.assign(K, lab, S.cpu(), part)
    with pytest.raises(ValueError):
        _lloyd.seed(K, k, 'given', seeds=np.array([0, 1, 8]))
    with pytest.raises(ValueError):
        _lloyd.seed(K, k, 'k-means++', np.array([[0.1, 0.2, 1.0]]))
    with pytest.raises(TypeError):
        _lloyd.predict(K, lab[0].cpu(), part[0, 0, :k], part[0, 0, k:])
    empty = torch.zeros((0, n), dtype=torch.float64, device='cuda')
    D, arg = _lloyd.predict(empty, lab[0], part[0, 0, :k].contiguous(),
                            part[0, 0, k:].contiguous())
    assert D.shape == (0, k) and arg.shape == (0,)


# -- the whole fit ------------------------------------------------------------------
@pytest.mark.parametrize('n,k', cpu.NK)
def test_fit_against_lloyd_on_explicit_features(n, k):
    X, K, labels0 = cpu.blobs(n, k, 0)
    lab, it, history = cpu.lloyd(X, labels0, k)
    km = cpu.model(k, device='cuda')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        km.fit(_t(K).cuda(), labels0=labels0)
    cpu.check_fit(km, X, K, lab, it, history)
    assert km.last_timing['rounds'] == -(-it // 4) * 4
    assert np.array_equal(km.predict(_t(K).cuda()), lab)


def test_unconverged_and_empty_on_the_device():
    X, K, labels0 = cpu.blobs(257, 16, 0)
    for rounds in (1, 2, 5):
        with pytest.warns(UserWarning, match='not converged'):
            km = cpu.model(16, device='cuda', max_iter=rounds).fit(
                _t(K).cuda(), labels0=labels0)
        lab, it, history = cpu.lloyd(X, labels0, 16, max_iter=rounds)
        cpu.check_fit(km, X, K, lab, it, history)
    X, K, _ = cpu.blobs(65, 3, 6)
    labels0 = np.arange(65) % 3
    with pytest.warns(UserWarning, match='1 of 4 clusters are empty'):
        km = cpu.model(4, device='cuda').fit(_t(K).cuda(), labels0=labels0)
    cpu.check_fit(km, X, K, *cpu.lloyd(X, labels0, 4))
    assert km.medoid_indices_[3] == -1
    bad = K.copy()
    bad[3, 5] = bad[5, 3] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        cpu.model(3, device='cuda').fit(_t(bad).cuda())


@pytest.mark.parametrize('init', ['k-means++', 'farthest'])
def test_restarts_on_the_device_match_the_host(init):
    n, k, R = 257, 6, 5
    X, K, _ = cpu.blobs(n, k, 3)
    host = cpu.model(k, init=init, n_init=R, random_state=11).fit(K)
    dev = cpu.model(k, init=init, n_init=R, random_state=11,
                    device='cuda').fit(_t(K).cuda())
    assert np.array_equal(dev.seed_indices_, host.seed_indices_)
    assert np.array_equal(dev.restart_n_iter_, host.restart_n_iter_)
    assert dev.best_restart_ == host.best_restart_
    assert np.array_equal(dev.labels_, host.labels_)
    np.testing.assert_allclose(dev.restart_inertia_, host.restart_inertia_,
                               rtol=1e-9)
    again = cpu.model(k, init=init, n_init=R, random_state=11,
                      device='cuda').fit(_t(K).cuda())
    assert again.inertia_ == dev.inertia_
    assert np.array_equal(again.labels_, dev.labels_)


# -- the model on QM7-like graphs ---------------------------------------------------
N_TRAIN, N_HELD_OUT, K_GRAPHS = 40, 8, 3


def _graphs():
    import cases
    G = np.asarray(list(cases.config3_graphs(N_TRAIN + N_HELD_OUT, seed=29)),
                   dtype=object)
    return G[:N_TRAIN], G[N_TRAIN:]


def _kernel(real, transform):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    knode, kedge, q = cases.config3_fit_kernels()
    k = MarginalizedGraphKernel(
        knode, kedge, q=q, q_bounds=(1e-3, 0.5),
        backend=HIPBackend(real=real),
        ftol=1e-13 if real is np.float64 else 1e-8)
    return Normalization(k) if transform == 'normalized' else k


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('transform', ['plain', 'normalized'])
def test_device_matches_host(real, transform, monkeypatch):
    """The model on the device path against the host chain on the very
    matrices the device path worked on (downloaded here, for the test).  The
    inertia is a sum of n terms ``K_ii - S / n_c``, each a sum of n entries:
    ``4 n eps (sum |K_ii| + sum_c sum |K_cc| / n_c)``; a squared distance of
    `transform` is within ``8 n eps`` of the largest entry."""
    from graphdot_amd.model.clustering import KernelKMeans
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G, Z = _graphs()
    n, k = N_TRAIN, K_GRAPHS
    kernel = _kernel(real, transform)
    labels0 = np.arange(n) % k
    K = torch.as_tensor(kernel.device_gram(G), device='cuda').cpu().numpy()
    Ks = torch.as_tensor(kernel.device_cross_gram(Z, G),
                         device='cuda').cpu().numpy()
    dz = torch.as_tensor(kernel.device_diag(Z), device='cuda').cpu().numpy()
    host = KernelKMeans('precomputed', k, device='cpu').fit(K, labels0=labels0)
    p_h, t_h = host.predict(Ks), host.transform(Ks, diag=dz)
    # the device path: no host kernel evaluation, no n x n download
    calls, downloads = [], []

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
        monkeypatch.setattr(cls, 'diag', counting)
    to_host = torch.Tensor.cpu

    def cpu_counting(self, *args, **kwargs):
        if self.is_cuda and self.numel() >= n * n:
            downloads.append(tuple(self.shape))
        return to_host(self, *args, **kwargs)
    monkeypatch.setattr(torch.Tensor, 'cpu', cpu_counting)
    dev = KernelKMeans(kernel, k, device='cuda').fit(G, labels0=labels0)
    p_d, t_d = dev.predict(Z), dev.transform(Z)
    seeded = KernelKMeans(kernel, k, n_init=4, device='cuda').fit(G)
    assert dev.last_timing['adopted'] is True
    assert calls == [] and downloads == []
    a = np.abs(K.astype(np.float64))
    size = np.trace(a) + sum(
        a[np.ix_(host.labels_ == c, host.labels_ == c)].sum()
        / max((host.labels_ == c).sum(), 1) for c in range(k))
    print(f'{real.__name__} {transform}: rounds {dev.n_iter_}, sizes '
          f'{dev.cluster_sizes_}, inertia {dev.inertia_} against '
          f'{host.inertia_} (bound {4 * n * EPS * size:.3g}), transform '
          f'{np.abs(t_d ** 2 - t_h ** 2).max():.3g} (bound '
          f'{8 * n * EPS * a.max():.3g})')
    assert np.array_equal(dev.labels_, host.labels_)
    assert dev.n_iter_ == host.n_iter_
    assert np.array_equal(dev.medoid_indices_, host.medoid_indices_)
    assert np.array_equal(dev.cluster_sizes_, host.cluster_sizes_)
    assert abs(dev.inertia_ - host.inertia_) <= 4 * n * EPS * size
    assert np.array_equal(p_d, p_h) and p_d.shape == (N_HELD_OUT,)
    assert t_d.shape == (N_HELD_OUT, k)
    assert np.all(np.abs(t_d ** 2 - t_h ** 2) <= 8 * n * EPS * a.max())
    assert seeded.inertia_ == seeded.restart_inertia_.min()
    assert seeded.cluster_sizes_.sum() == n
