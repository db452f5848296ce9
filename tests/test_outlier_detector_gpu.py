"""The fused device path of the outlier detector on an MI355X: outlier.hip's
epilogue against numpy float64 (tile edges, f32 / f64 planes, plane subsets,
both plane layouts, bit-identical repeats), device against host on QM7-like
graphs with each inverse path, no host kernel evaluation, and a seeded fit
that finds three shifted targets."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    import graphdot_amd.model.gaussian_process  # noqa: F401 (torch first)
    return torch


# -- the epilogue against numpy float64 ---------------------------------------------
def _case(n, m, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, n))
    Ks = A @ A.T / n + np.eye(n)
    Kinv = np.linalg.inv(Ks)
    Kinv = 0.5 * (Kinv + Kinv.T)
    P = rng.normal(size=(n, n, m))
    P = P + P.transpose(1, 0, 2)
    return Ks, Kinv, rng.normal(size=n), rng.uniform(0.01, 1, n), P


def _reference(Ks, Kinv, y, s2, P, planes):
    a = Kinv @ y
    W = Kinv - np.outer(a, a)
    return np.concatenate((
        [y @ a, np.abs(Ks).sum(1).max(), np.abs(Kinv).sum(1).max()],
        np.einsum('ij,ijk->k', W, P[:, :, planes].astype(np.float64)),
        (np.diag(Kinv) - a**2) * 2 * s2))


def _planes(P, dtype, layout):
    torch = _torch()
    if layout == 'column-major':      # i + n j + n^2 k (device_gram)
        t = torch.from_numpy(np.ascontiguousarray(
            P.transpose(2, 1, 0)).astype(dtype)).cuda()
        return t.permute(2, 1, 0)
    return torch.from_numpy(P.astype(dtype)).cuda()   # k fastest (torch.cat)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('layout', ['column-major', 'row-major'])
@pytest.mark.parametrize('m,planes', [(1, [0]), (7, [0, 1, 2, 3, 4, 5, 6]),
                                      (16, list(range(16))), (9, [7, 2, 5])])
def test_epilogue_against_numpy(n, dtype, layout, m, planes):
    torch = _torch()
    from graphdot_amd.model.gaussian_process import _outlier
    if n == 1000 and m == 16 and layout == 'row-major':
        pytest.skip('covered by the column-major case (memory of the host '
                    'reference)')
    Ks, Kinv, y, s2, P = _case(n, m, n + m)
    Pt = _planes(P, dtype, layout)
    assert Pt.stride(0 if layout == 'column-major' else 2) == 1
    out = _outlier.epilogue(torch.from_numpy(Kinv).cuda(),
                            torch.from_numpy(Ks).cuda(), y, s2, Pt,
                            planes).cpu().numpy()
    ref = _reference(Ks, Kinv, y, s2, P.astype(dtype), planes)
    # (double arithmetic on the same stored inputs: summation order only)
    np.testing.assert_allclose(out[:3], ref[:3], rtol=1e-12)
    np.testing.assert_allclose(out[3:], ref[3:], rtol=1e-10,
                               atol=1e-12 * np.abs(ref[3:]).max())


def test_epilogue_repeat_bits_and_no_planes():
    torch = _torch()
    from graphdot_amd.model.gaussian_process import _outlier
    Ks, Kinv, y, s2, P = _case(333, 12, 5)
    args = (torch.from_numpy(Kinv).cuda(), torch.from_numpy(Ks).cuda(), y,
            s2, _planes(P, np.float32, 'column-major'), [11, 0, 4, 9, 3])
    a = _outlier.epilogue(*args).cpu().numpy()
    b = _outlier.epilogue(*args).cpu().numpy()
    assert np.array_equal(a, b)
    c = _outlier.epilogue(*args[:4]).cpu().numpy()
    assert len(c) == 3 + 333
    assert np.array_equal(c[:3], a[:3]) and np.array_equal(c[3:], a[8:])
    with pytest.raises(IndexError):
        _outlier.epilogue(*args[:5], [12])


# -- the detector on QM7-like graphs ----------------------------------------------
def _graphs(n=60, copies=9, seed=17):
    """n QM7-like molecules and `copies` more copies of the first: the
    kernel matrix is singular, so a small sigma makes the clamp active."""
    import cases
    from graphdot_amd.graph import Graph
    G = list(cases.config3_graphs(n, seed=seed))
    G = Graph.unify_datatype(G + [G[0]] * copies)
    rng = np.random.default_rng(seed)
    return np.asarray(G, dtype=object), rng.normal(size=len(G))


def _kernel(real, transform):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization, Exponentiation
    knode, kedge, q = cases.config3_fit_kernels()
    k = MarginalizedGraphKernel(knode, kedge, q=q, backend=HIPBackend(
        real=real), ftol=1e-13 if real is np.float64 else 1e-8)
    if transform == 'normalized':
        k = Normalization(k)
    elif transform == 'exponentiated':
        k = Exponentiation(Normalization(k), xi=2.0)
    return k


def _sigma(K, path, beta=1e-8):
    """Per-sample noise levels for which the inverse takes `path`."""
    n = len(K)
    if path == 'A':
        return np.full(n, 0.3 * np.sqrt(np.median(np.diag(K))))
    if path == 'B':
        # the duplicates' null space has inverse row sums ~ 1.8 / sigma^2:
        # ||K|| ||K^-1|| ~ 1.5 / beta fails A, while K - beta ||K|| I keeps
        # eigenvalues >= 0.2 beta ||K||
        return np.full(n, np.sqrt(1.2 * beta * np.abs(K).sum(1).max()))
    return np.full(n, 1e-4 * np.sqrt(np.median(np.diag(K))))


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('transform', ['raw', 'normalized', 'exponentiated'])
@pytest.mark.parametrize('path', ['A', 'B', 'eigh'])
def test_device_matches_host(real, transform, path):
    from graphdot_amd.model.gaussian_process import GPROutlierDetector
    if path == 'B' and real is np.float32:
        pytest.skip('a float kernel matrix is not positive definite to '
                    'within beta ||K||')
    G, y = _graphs()
    k = _kernel(real, transform)
    K = np.asarray(k(G), dtype=np.float64)
    sigma = _sigma(K, path)
    theta_ext = np.concatenate((k.theta, np.log(sigma)))
    out = {}
    for device in ('cuda', 'cpu'):
        m = GPROutlierDetector(k, device=device)
        v, g = m.log_marginal_likelihood(theta_ext, X=G, y=y,
                                         eval_gradient=True)
        out[device] = (v, g, m.last_timing['path'])
    assert out['cuda'][2] == path
    assert out['cpu'][2] == path
    # same kernel values (f64) or the same float solves; the inverse by
    # potrf.hip or rocSOLVER's eigh against LAPACK: cond(K) <= 1 / beta
    rv, rg = {('A', np.float64): (1e-10, 1e-7), ('B', np.float64): (1e-7,
                                                                     1e-4),
              ('eigh', np.float64): (1e-7, 1e-4), ('A', np.float32): (1e-5,
                                                                      1e-3),
              ('eigh', np.float32): (1e-4, 1e-2)}[path, real]
    assert out['cuda'][0] == pytest.approx(out['cpu'][0], rel=rv)
    hg = out['cpu'][1]
    np.testing.assert_allclose(out['cuda'][1], hg, rtol=rg,
                               atol=rg * np.abs(hg).max())


def test_no_host_round_trip(monkeypatch):
    """The device path never calls the kernel's numpy `__call__`."""
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization, Exponentiation
    from graphdot_amd.model.gaussian_process import GPROutlierDetector
    G, y = _graphs(40, 0)
    models = [(GPROutlierDetector(_kernel(r, t), device='cuda'), t)
              for r, t in ((np.float64, 'raw'), (np.float32, 'normalized'),
                           (np.float64, 'exponentiated'))]

    def refuse(*args, **kwargs):
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization, Exponentiation):
        monkeypatch.setattr(cls, '__call__', refuse)
    for m, t in models:
        theta_ext = np.concatenate((m.kernel.theta, np.full(len(G), -1.0)))
        v, g = m.log_marginal_likelihood(theta_ext, X=G, y=y,
                                         eval_gradient=True)
        assert np.isfinite(v) and np.all(np.isfinite(g))
        assert m.last_timing['path'] == 'A'


def test_fit_flags_shifted_targets():
    """Targets drawn from the kernel's own GP (plus a small jitter), three
    of them shifted by four standard deviations: the fit ranks exactly those
    three highest in y_uncertainty, clearly apart from the rest."""
    from graphdot_amd.model.gaussian_process import GPROutlierDetector
    G, _ = _graphs(80, 0, seed=29)
    k = _kernel(np.float64, 'normalized')
    K = np.asarray(k(G), dtype=np.float64)
    rng = np.random.default_rng(29)
    y = np.linalg.cholesky(K + 1e-2 * np.eye(len(G))) @ rng.normal(
        size=len(G))
    shifted = [5, 41, 66]
    y[shifted] += 4.0 * y.std() * np.array([1, -1, 1])
    m = GPROutlierDetector(k, normalize_y=True, device='cuda')
    np.random.seed(0)
    m.fit(G, y, w=0.3)
    u = m.y_uncertainty
    top = sorted(int(i) for i in np.argsort(u)[-3:])
    assert top == shifted, (top, u[shifted], np.sort(u)[-6:])
    others = np.delete(u, shifted)
    # (host run of the same fit: 0.71 against at most 0.48)
    assert u[shifted].min() > 1.3 * others.max(), (u[shifted], others.max())
