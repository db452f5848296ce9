"""KernelOverMetric on an MI355X: MaxiMin.device_distance against
MaxiMin.__call__ (bit for bit), the HIP map of kernel_over_metric.hip against
numpy, the device methods of KernelOverMetric(MaxiMin) against its host
calls, the regressors on the device path against the CPU algebra, and the
fallback for graphs beyond the owner-computes solvers."""
import numpy as np
import pytest
import sympy

pytestmark = pytest.mark.gpu

GAUSS = 'v * exp(-d^2 / ell^2)'
RQ = 'v * (1 + d**2 / (2 * a * ell**2)) ** -a'
F32_ROUND = 2.0**-24        # relative rounding of a float32 K


def _torch():
    import torch
    import graphdot_amd.model.gaussian_process  # noqa: F401 (torch first)
    return torch


@pytest.fixture(autouse=True)
def _torch_first():
    """torch's HIP runtime comes up before libgdhip's (see
    graphdot_amd.hip.runtime._let_torch_initialise_first)."""
    _torch().cuda.is_available()


def _np(t):
    return _torch().as_tensor(t, device='cuda').cpu().numpy()


def _maximin(real='f32', **kw):
    import cases
    from graphdot_amd.metric.maximin import MaxiMin
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    knode, kedge, q = cases.config3_kernels()
    backend = HIPBackend(real={'f32': np.float32, 'f64': np.float64}[real])
    return MaxiMin(knode, kedge, q=q, backend=backend, **kw)


def _kom(expr=GAUSS, real='f32', **hypers):
    from graphdot_amd.kernel import KernelOverMetric
    hypers = hypers or dict(v=(1.0, (1e-2, 1e2)), ell=(0.6, (1e-2, 1e2)))
    return KernelOverMetric(_maximin(real), expr, 'd', **hypers)


# -- MaxiMin.device_distance ---------------------------------------------------
@pytest.mark.parametrize('real', ['f32', 'f64'])
@pytest.mark.parametrize('cross', [False, True])
@pytest.mark.parametrize('grad', [False, True])
def test_device_distance_is_the_call(real, cross, grad):
    import cases
    G = cases.config3_graphs(11, seed=5)
    X, Y = (G[:6], G[6:]) if cross else (G, None)
    mm = _maximin(real)
    host = mm(X, Y, eval_gradient=grad)
    dev = mm.device_distance(X, Y, eval_gradient=grad)
    D, dD = dev if grad else (dev, None)
    assert D.dtype == np.dtype(np.float32 if real == 'f32' else np.float64)
    Dh = host[0] if grad else host
    Dd = _np(D)
    assert np.array_equal(Dd.astype(np.float32), Dh)
    if grad:
        mask = np.asarray(mm.active_theta_mask)
        g = _np(dD)
        assert g.shape == (len(X), len(Y or X), mm.n_dims)
        assert np.array_equal(g[:, :, mask].astype(np.float32), host[1])
    # a later evaluation leaves these views alone
    keep = Dd.copy()
    mm.device_distance(G[2:9], eval_gradient=grad)
    mm(G[1:4], eval_gradient=True)
    assert np.array_equal(_np(D), keep)


def test_device_distance_refuses_other_backends():
    """TypeError where the fused evaluation does not apply: a backend
    without it, and a backend whose solvers for these graphs are not the
    owner-computes ones (the two-stage general solver)."""
    import cases
    from graphdot_amd.metric.maximin import MaxiMin
    from graphdot_amd.kernel.marginalized._backend_hip import (
        HIPBackend, GENERAL)
    knode, kedge, q = cases.config3_kernels()
    G = cases.config3_graphs(4, seed=2)
    mm = MaxiMin(knode, kedge, q=q, backend='hip')
    mm.backend = object()
    with pytest.raises(TypeError):
        mm.device_distance(G)
    general = HIPBackend(variants=[GENERAL])
    mm = MaxiMin(knode, kedge, q=q, backend=general)
    with pytest.raises(TypeError):
        mm.device_distance(G, eval_gradient=True)


# -- the map against numpy ------------------------------------------------------
def _numpy_map(expr, names, D, h, P, planes):
    d = sympy.Symbol('d')
    hs = [sympy.Symbol(n) for n in names]
    e = sympy.sympify(expr)
    f = sympy.lambdify((d, *hs), e, 'numpy')
    D = D.astype(np.float64)
    K = f(D, *h)
    own = [np.broadcast_to(sympy.lambdify((d, *hs), sympy.diff(e, s),
                                          'numpy')(D, *h), D.shape)
           for s in hs]
    S = sympy.lambdify((d, *hs), sympy.diff(e, d), 'numpy')(D, *h)
    dist = [S * P[:, :, k].astype(np.float64) for k in planes]
    return K, np.stack(own + dist, axis=2) if own + dist else \
        np.zeros((*D.shape, 0)), np.stack(own, axis=2), S


def _fortran_tensor(a):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    return t.permute(*range(a.ndim - 1, -1, -1))


@pytest.mark.parametrize('shape', [(1, 1), (257, 130), (300, 1), (64, 513)])
@pytest.mark.parametrize('td', [np.float32, np.float64])
@pytest.mark.parametrize('tp', [np.float32, np.float64])
@pytest.mark.parametrize('nplanes,planes', [(0, []), (5, [0, 1, 2, 3, 4]),
                                            (5, [4, 1, 3])])
def test_map_against_numpy(shape, td, tp, nplanes, planes):
    from graphdot_amd.kernel._kom_map import DeviceMap
    names = ('v', 'a', 'ell')
    h = np.array([1.3, 0.8, 0.7])
    rng = np.random.default_rng(shape[0] * 7 + nplanes)
    D = rng.uniform(0, 2, shape).astype(td)
    P = rng.normal(size=(*shape, nplanes)).astype(tp)
    m = DeviceMap(RQ, 'd', names)
    Dt, Pt = _fortran_tensor(D), _fortran_tensor(P)
    K, G, own, S = _numpy_map(RQ, names, D, h, P, planes)
    tol = dict(rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(_np(m(Dt, h)), K, **tol)
    Kd, Gd = m(Dt, h, Pt, planes, form='dense')
    assert Gd.shape == (*shape, 3 + len(planes))
    assert Gd.permute(2, 1, 0).is_contiguous()
    np.testing.assert_allclose(_np(Kd), K, **tol)
    np.testing.assert_allclose(_np(Gd), G, **tol)
    Kl, Gl, Sl = m(Dt, h, form='lazy')
    np.testing.assert_allclose(_np(Gl), own, **tol)
    np.testing.assert_allclose(_np(Sl), S, **tol)
    # row-major D and P (any strides) give the same numbers
    Kr, Gr = m(_torch().from_numpy(D).cuda(), h,
               _torch().from_numpy(P).cuda(), planes, form='dense')
    assert np.array_equal(_np(Kr), _np(Kd))
    assert np.array_equal(_np(Gr), _np(Gd))
    # repeated calls: the same bits
    Kd2, Gd2 = m(Dt, h, Pt, planes, form='dense')
    assert np.array_equal(_np(Kd2), _np(Kd))
    assert np.array_equal(_np(Gd2), _np(Gd))


def test_map_checks_its_arguments():
    from graphdot_amd.kernel._kom_map import DeviceMap
    torch = _torch()
    m = DeviceMap(GAUSS, 'd', ('v', 'ell'))
    D = torch.zeros((4, 3), dtype=torch.float32, device='cuda')
    P = torch.zeros((4, 3, 2), dtype=torch.float32, device='cuda')
    with pytest.raises(IndexError):
        m(D, [1.0, 1.0], P, [2], form='dense')
    with pytest.raises(ValueError):
        m(D, [1.0], P, [0], form='dense')
    with pytest.raises(ValueError):
        m(D, [1.0, 1.0], P[:3], [0], form='dense')


# -- the device methods against the host calls ---------------------------------
def _check_k(Kd, Kh):
    """The device's float64 K against the host's float32 K: within the
    float32 rounding of the host's value."""
    Kd = np.asarray(Kd, dtype=np.float64)
    Kh = np.asarray(Kh, dtype=np.float64)
    assert np.all(np.abs(Kd - Kh) <= F32_ROUND * np.abs(Kd) + 1e-300)


def _check_g(Gd, Gh):
    """Both from the same distances: 1e-12 relative, column by column."""
    assert Gd.shape == Gh.shape
    scale = np.abs(Gh).max(axis=(0, 1))
    assert np.all(np.abs(Gd - Gh) <= 1e-12 * scale + 1e-300)


@pytest.mark.parametrize('expr,hypers', [
    (GAUSS, dict(v=(1.0, (1e-2, 1e2)), ell=(0.6, (1e-2, 1e2)))),
    (RQ, dict(v=1.2, a=(0.9, 1e-3, 1e3), ell=(0.5,))),
])
def test_device_methods_match_the_host(expr, hypers):
    import cases
    G = cases.config3_graphs(30, seed=3)
    k = _kom(expr, **hypers)
    K, dK = k.device_gram(G, eval_gradient=True)
    assert K.dtype == _torch().float64 and dK.shape[2] == len(k.theta)
    Kh, dKh = k(G, eval_gradient=True)
    assert Kh.dtype == np.float32
    _check_k(_np(K), Kh)
    _check_g(_np(dK), dKh)
    _check_k(_np(k.device_gram(G)), k(G))
    X, Y = G[:13], G[13:]
    K, dK = k.device_cross_gram(X, Y, eval_gradient=True)
    Kh, dKh = k(X, Y, eval_gradient=True)
    _check_k(_np(K), Kh)
    _check_g(dK.dense().cpu().numpy(), dKh)
    _check_k(_np(k.device_cross_gram(X, Y)), k(X, Y))
    d, dd = k.device_diag(X, eval_gradient=True)
    assert np.array_equal(_np(d), k.diag(X))
    dd = _np(dd)
    assert dd.shape == (len(X), len(k.theta))
    nh = len(k.get_params())
    at0 = [k._eval(fn, np.zeros(len(X))) for fn in k._grad]
    assert np.array_equal(dd[:, :nh], np.stack(at0, axis=1))
    assert np.all(dd[:, nh:] == 0)


def test_fixed_distance_hyperparameters():
    """A MaxiMin with fixed hyperparameters: the active planes only."""
    import cases
    from graphdot_amd.metric.maximin import MaxiMin
    from graphdot_amd.kernel import KernelOverMetric
    from graphdot_amd.microkernel import (TensorProduct, KroneckerDelta,
                                          SquareExponential)
    knode = TensorProduct(atomic_number=KroneckerDelta(0.5, 'fixed'),
                          hcount=SquareExponential(1.0),
                          aromatic=KroneckerDelta(0.8, 'fixed'))
    kedge = TensorProduct(order=SquareExponential(0.5),
                          conjugated=KroneckerDelta(0.5, 'fixed'))
    mm = MaxiMin(knode, kedge, q=0.01, backend='hip')
    assert not np.all(mm.active_theta_mask)
    k = KernelOverMetric(mm, GAUSS, 'd', v=1.0, ell=0.6)
    G = cases.config3_graphs(12, seed=4)
    K, dK = k.device_gram(G, eval_gradient=True)
    Kh, dKh = k(G, eval_gradient=True)
    _check_k(_np(K), Kh)
    _check_g(_np(dK), dKh)
    K, dK = k.device_cross_gram(G[:5], G[5:], eval_gradient=True)
    _check_g(dK.dense().cpu().numpy(), k(G[:5], G[5:], eval_gradient=True)[1])


# -- the regressors ----------------------------------------------------------------
class HostOfDevice:
    """The kernel protocol served from the device methods (downloaded): the
    CPU algebra fed with the device's own K and planes."""

    def __init__(self, k):
        self.k = k

    theta = property(lambda self: self.k.theta)
    bounds = property(lambda self: self.k.bounds)

    def clone_with_theta(self, theta):
        return HostOfDevice(self.k.clone_with_theta(theta))

    def __call__(self, X, Y=None, eval_gradient=False):
        if Y is None:
            out = self.k.device_gram(X, eval_gradient=eval_gradient)
        else:
            out = self.k.device_cross_gram(X, Y, eval_gradient=eval_gradient)
        if not eval_gradient:
            return _np(out)
        K, dK = out
        dK = dK.dense() if hasattr(dK, 'dense') else dK
        return _np(K), np.asfortranarray(_np(dK))

    def diag(self, X, eval_gradient=False):
        return _np(self.k.device_diag(X))


class NoHost:
    """Makes the host evaluation of KernelOverMetric fail for the duration
    (the device path must not use it); `values=True` lets value-only calls
    through (GaussianProcessRegressor.fit factors the final K on the host
    path, for any kernel)."""

    def __init__(self, values=False):
        self.values = values

    def __enter__(self):
        from graphdot_amd.kernel import KernelOverMetric
        self.saved = KernelOverMetric.__call__, KernelOverMetric.diag
        call, values = self.saved[0], self.values

        def fail(self, X, Y=None, eval_gradient=False):
            if values and not eval_gradient:
                return call(self, X, Y)
            raise AssertionError('host evaluation on the device path')
        KernelOverMetric.__call__ = KernelOverMetric.diag = fail

    def __exit__(self, *exc):
        from graphdot_amd.kernel import KernelOverMetric
        KernelOverMetric.__call__, KernelOverMetric.diag = self.saved


def _targets(G, seed=0):
    rng = np.random.default_rng(seed)
    return np.array([len(g.nodes) for g in G], dtype=float) * 0.1 + \
        rng.normal(size=len(G)) * 0.05


def _first_order_bound(K, y, dK):
    """Bounds on |d value| and |d gradient_k| of y^T K^-1 y + log|K| for a
    perturbation of K by its float32 rounding (|dK_ij| <= 2^-24 |K_ij|), to
    first order: |d value| <= ||E|| (||a||^2 + ||K^-1||_F) and |d g_k| <=
    ||E|| (||K^-1||^2 + 2 ||K^-1|| ||a||^2) ||dK_k||_F, with a = K^-1 y, E
    the rounding matrix (Frobenius norm) and ||K^-1|| the spectral norm.
    A factor 2 covers the second order."""
    Kinv = np.linalg.inv(K)
    a = Kinv @ y
    e = F32_ROUND * np.linalg.norm(K)
    s = np.linalg.norm(Kinv, 2)
    dv = e * (a @ a + np.linalg.norm(Kinv))
    dg = e * (s**2 + 2 * s * (a @ a)) * np.linalg.norm(dK, axis=(0, 1))
    return 2 * dv, 2 * dg


def test_gpr_device_path():
    import cases
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    G = cases.config3_graphs(48, seed=21)
    y = _targets(G)
    k = _kom()
    dev = GaussianProcessRegressor(k, alpha=1e-2, device='cuda')
    dev.X, dev.y = G, y
    with NoHost():
        v, g = dev.log_marginal_likelihood(eval_gradient=True)
    # the CPU algebra on the device's own K and planes
    ref = GaussianProcessRegressor(HostOfDevice(k), alpha=1e-2,
                                   device='cpu')
    ref.X, ref.y = G, y
    vr, gr = ref.log_marginal_likelihood(eval_gradient=True)
    np.testing.assert_allclose(v, vr, rtol=1e-8)
    np.testing.assert_allclose(g, gr, rtol=1e-8, atol=1e-8 * np.abs(gr).max())
    # the plain host path: float32 K
    host = GaussianProcessRegressor(k, alpha=1e-2, device='cpu')
    host.X, host.y = G, y
    vh, gh = host.log_marginal_likelihood(eval_gradient=True)
    K, dK = k(G, eval_gradient=True)
    K = K.astype(np.float64) + 1e-2 * np.eye(len(G))
    dv, dg = _first_order_bound(K, y, dK)
    assert abs(v - vh) <= dv, (v - vh, dv)
    assert np.all(np.abs(g - gh) <= dg * np.exp(k.theta)), (g - gh, dg)


def test_gpr_fit_on_the_device():
    import cases
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    G = cases.config3_graphs(64, seed=8)
    y = _targets(G, seed=2)
    k = _kom()
    gpr = GaussianProcessRegressor(k, alpha=1e-2, optimizer=True,
                                   device='cuda')
    gpr.X, gpr.y = G, y
    start = gpr.log_marginal_likelihood()
    with NoHost(values=True):
        gpr.fit(G, y, tol=1e-3)
    assert np.all(np.isfinite(gpr.kernel.theta))
    assert gpr.log_marginal_likelihood() < start


def test_lowrank_and_outlier_device_paths():
    import cases
    from graphdot_amd.model.gaussian_process import (LowRankApproximateGPR,
                                                     GPROutlierDetector)
    G = cases.config3_graphs(60, seed=17)
    X, C = G[:44], G[44:]
    y = _targets(X, seed=5)
    k = _kom()
    out = {}
    for name, kern, dev in (('dev', k, 'cuda'), ('ref', HostOfDevice(k),
                                                 'cpu'), ('host', k, 'cpu')):
        m = LowRankApproximateGPR(kern, alpha=1e-3, device=dev)
        m.C, m.X, m.y = C, X, y
        if name == 'dev':
            with NoHost():
                out[name] = m.log_marginal_likelihood(eval_gradient=True)
        else:
            out[name] = m.log_marginal_likelihood(eval_gradient=True)
    np.testing.assert_allclose(out['dev'][0], out['ref'][0], rtol=1e-8)
    np.testing.assert_allclose(out['dev'][1], out['ref'][1], rtol=1e-8,
                               atol=1e-8 * np.abs(out['ref'][1]).max())
    # against the float32 host: the rounding of K amplified by the
    # conditioning of the core matrix
    Kc = k(C).astype(np.float64) + 1e-3 * np.eye(len(C))
    tol = 4 * len(X) * np.linalg.cond(Kc) * F32_ROUND
    np.testing.assert_allclose(out['dev'][0], out['host'][0], rtol=tol)
    np.testing.assert_allclose(out['dev'][1], out['host'][1], rtol=tol,
                               atol=tol * np.abs(out['host'][1]).max())

    theta_ext = np.concatenate((k.theta, np.log(np.full(len(X), 0.1))))
    out = {}
    for name, kern, dev in (('dev', k, 'cuda'), ('ref', HostOfDevice(k),
                                                 'cpu'), ('host', k, 'cpu')):
        m = GPROutlierDetector(kern, device=dev)
        m.X, m.y = X, y
        if name == 'dev':
            with NoHost():
                out[name] = m.log_marginal_likelihood(theta_ext,
                                                      eval_gradient=True)
        else:
            out[name] = m.log_marginal_likelihood(theta_ext,
                                                  eval_gradient=True)
    np.testing.assert_allclose(out['dev'][0], out['ref'][0], rtol=1e-8)
    np.testing.assert_allclose(out['dev'][1], out['ref'][1], rtol=1e-8,
                               atol=1e-8 * np.abs(out['ref'][1]).max())
    Ks = k(X).astype(np.float64) + 0.01 * np.eye(len(X))
    tol = 4 * len(X) * np.linalg.cond(Ks) * F32_ROUND
    np.testing.assert_allclose(out['dev'][0], out['host'][0], rtol=tol)
    np.testing.assert_allclose(out['dev'][1], out['host'][1], rtol=tol,
                               atol=tol * np.abs(out['host'][1]).max())


# -- graphs beyond the owner-computes solvers ----------------------------------------
def test_fallback_beyond_owner_computes():
    import cases
    from graphdot_amd.metric.maximin import MaxiMin
    from graphdot_amd.kernel import KernelOverMetric
    from graphdot_amd.kernel.marginalized._backend_hip import NotOwnerComputes
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    G = cases.protein_like_graphs(3, nmin=150, nmax=190, seed=41)
    knode, kedge, q = cases.tang2019_kernels()
    mm = MaxiMin(knode, kedge, q=q, backend='hip')
    with pytest.raises(NotOwnerComputes):
        mm.backend.maximin_distance(*mm._maximin_args(G, None, False, 0))
    with pytest.raises(TypeError):
        mm.device_distance(G)
    k = KernelOverMetric(mm, GAUSS, 'd', v=1.0, ell=0.6)
    with pytest.raises(TypeError):
        k.device_gram(G)
    y = _targets(G)
    vals = []
    for dev in ('cuda', 'cpu'):
        gpr = GaussianProcessRegressor(k, alpha=1e-2, device=dev)
        gpr.X, gpr.y = G, y
        vals.append(gpr.log_marginal_likelihood())
    np.testing.assert_allclose(vals[0], vals[1], rtol=1e-12)
