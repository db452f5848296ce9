"""The fused device path of the Gaussian field regressor on an MI355X:
field.hip's two entry points against numpy float64, bit-identical repeats,
device/host parity of the regressor on QM7-like graphs (raw marginalized
graph kernel in float and double, and its normalisation), the gradient
against finite differences, no host kernel evaluation, the peak memory of
the contraction, and which path is taken."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    import graphdot_amd.model.gaussian_field  # noqa: F401 (torch first)
    return torch


# -- the kernels against numpy float64 ----------------------------------------------
def _np_reference(K, kr, kc, dkr, dkc, sigma, smoothing, alpha, beta, gamma,
                  P, planes, self_block, y, row, col, u, v):
    half, eps = 0.4999997, 1e-4
    K = K.astype(np.float64)
    d = np.sqrt(np.maximum(0.0, -K + half * kr[:, None] + half * kc[None, :]))
    w = np.exp(-0.5 * d**2 * sigma**-2)
    if self_block:
        np.fill_diagonal(w, 0.0)
    s = (w + smoothing).sum(1)
    t = (w + smoothing) @ y
    A = alpha[:, None] + beta[:, None] * gamma[None, :]
    dK = P[:, :, planes].astype(np.float64)
    if row is not None:
        dK = dK * row[:, None, None]
    if col is not None:
        dK = dK * col[None, :, None]
    if u is not None:
        dK = dK + K[:, :, None] * u[:, None, :]
    if v is not None:
        dK = dK + K[:, :, None] * v[None, :, :]
    g0 = (A * d**2 * w * sigma**-3).sum()
    dD = (-dK + 0.5 * dkr[:, None, :] + 0.5 * dkc[None, :, :]) \
        * (0.5 / (d + eps))[:, :, None]
    gk = np.einsum('rc,rck->k', A * (-d * w * sigma**-2), dD)
    return s, t, w + smoothing, np.concatenate(([g0], gk))


def _case(rng, Nr, Nc, nplanes, planes, self_block, factors):
    if self_block:
        Nc = Nr
    X = rng.normal(size=(Nr, 3))
    Y = X if self_block else rng.normal(size=(Nc, 3))
    d2 = ((X[:, None, :] - Y[None, :, :])**2).sum(-1)
    K = np.exp(-0.3 * d2)
    kr, kc = np.ones(Nr), np.ones(Nc)
    n = len(planes)
    P = rng.normal(size=(Nr, Nc, nplanes))
    f = dict(row=None, col=None, u=None, v=None)
    if factors:
        f = dict(row=rng.uniform(0.5, 1.5, Nr), col=rng.uniform(0.5, 1.5, Nc),
                 u=rng.normal(size=(Nr, n)), v=rng.normal(size=(Nc, n)))
    return dict(K=K, kr=kr, kc=kc, dkr=rng.normal(size=(Nr, n)),
                dkc=rng.normal(size=(Nc, n)), alpha=rng.normal(size=Nr),
                beta=rng.normal(size=Nr), gamma=rng.normal(size=Nc),
                y=rng.normal(size=Nc), P=P, planes=np.array(planes),
                self_block=self_block, **f)


def _run(c, kdt, pdt, sigma=0.9, smoothing=1e-3):
    torch = _torch()
    from graphdot_amd.model.gaussian_field import _field

    def fortran(a, dt):
        t = torch.from_numpy(np.asfortranarray(a).astype(dt).T.copy())
        return t.cuda().permute(*reversed(range(a.ndim)))
    K, P = fortran(c['K'], kdt), fortran(c['P'], pdt)
    s, t, W = _field.rowsums(K, c['kr'], c['kc'], sigma, smoothing,
                             c['self_block'], y=c['y'], write=True)
    out = _field.contract(K, c['kr'], c['kc'], c['dkr'], c['dkc'], sigma,
                          c['alpha'], c['beta'], c['gamma'], P, c['planes'],
                          c['self_block'], row=c['row'], col=c['col'],
                          u=c['u'], v=c['v'])
    return [x.cpu().numpy() for x in (s, t, W, out)]


@pytest.mark.parametrize('kdt,pdt', [(np.float32, np.float32),
                                     (np.float64, np.float64),
                                     (np.float64, np.float32)])
@pytest.mark.parametrize('shape,planes', [
    ((70, 130), [0]), ((200, 33), [2, 0, 1]), ((1, 97), [4, 3, 2, 1, 0]),
    ((129, 1), [1, 3]), ((65, 190), list(range(17)))])
@pytest.mark.parametrize('self_block', [False, True])
@pytest.mark.parametrize('factors', [False, True])
def test_field_kernels_against_numpy(kdt, pdt, shape, planes, self_block,
                                     factors):
    rng = np.random.default_rng(len(planes) * 7 + shape[0])
    c = _case(rng, *shape, max(planes) + 2, planes, self_block, factors)
    s, t, W, out = _run(c, kdt, pdt)
    K = c['K'].astype(kdt)          # (what the kernel reads)
    P = c['P'].astype(pdt)
    rs, rt, rW, rout = _np_reference(
        K, c['kr'], c['kc'], c['dkr'], c['dkc'], 0.9, 1e-3, c['alpha'],
        c['beta'], c['gamma'], P, c['planes'], c['self_block'], c['y'],
        c['row'], c['col'], c['u'], c['v'])
    # (double arithmetic on the same stored inputs: summation order only)
    np.testing.assert_allclose(s, rs, rtol=1e-12)
    np.testing.assert_allclose(t, rt, rtol=1e-10, atol=1e-12 * np.abs(rt).max())
    np.testing.assert_allclose(W, rW, rtol=1e-14)
    np.testing.assert_allclose(out, rout, rtol=1e-10,
                               atol=1e-12 * np.abs(rout).max())


def test_field_kernels_repeat_bits_and_empty():
    torch = _torch()
    from graphdot_amd.model.gaussian_field import _field
    rng = np.random.default_rng(3)
    c = _case(rng, 300, 211, 6, [5, 1, 3, 0], False, True)
    a = _run(c, np.float32, np.float32)
    b = _run(c, np.float32, np.float32)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    K = torch.zeros((0, 5), dtype=torch.float64, device='cuda')
    P = torch.zeros((0, 5, 2), dtype=torch.float64, device='cuda')
    s, t, W = _field.rowsums(K, np.zeros(0), np.ones(5), 1.0, 0.1, False,
                             y=np.ones(5), write=True)
    assert s.shape == (0,) and W.shape == (0, 5)
    out = _field.contract(K, np.zeros(0), np.ones(5), np.zeros((0, 2)),
                          np.zeros((5, 2)), 1.0, np.zeros(0), np.zeros(0),
                          np.ones(5), P, [0, 1], False)
    assert out.cpu().numpy().tolist() == [0.0, 0.0, 0.0]


def test_contract_peak_memory():
    """No N x N temporary: the contraction's workspace is (n + 1) partial
    sums per workgroup."""
    torch = _torch()
    from graphdot_amd.model.gaussian_field import _field
    rng = np.random.default_rng(5)
    Nr, Nc, n = 2000, 1500, 5
    K = torch.rand((Nc, Nr), dtype=torch.float32, device='cuda').t()
    P = torch.rand((n, Nc, Nr), dtype=torch.float32,
                   device='cuda').permute(2, 1, 0)
    args = (K, np.ones(Nr), np.ones(Nc), rng.normal(size=(Nr, n)),
            rng.normal(size=(Nc, n)), 1.0, rng.normal(size=Nr),
            rng.normal(size=Nr), rng.normal(size=Nc), P, list(range(n)),
            False)
    _field.contract(*args)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _field.contract(*args)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < Nr * Nc * 8


# -- the regressor on QM7-like graphs -----------------------------------------------
def _graphs():
    import cases
    G = cases.config3_graphs(120, seed=17)
    rng = np.random.default_rng(17)
    y = cases.synthetic_energies(G)
    y = (y - y.mean()) / y.std()
    b = (y > 0).astype(float)
    unl = rng.choice(len(G), 80, replace=False)
    y[unl] = np.nan
    b[unl] = np.nan
    return np.asarray(G), y, b


def _model(real, normalized, device, optimizer=None):
    """sigma near the 10th percentile of the distances on this set: 0.3 of
    the normalised kernel, 5 of the raw one."""
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.metric import KernelInducedDistance
    from graphdot_amd.model.gaussian_field import (GaussianFieldRegressor,
                                                   RBFOverDistance)
    knode, kedge, q = cases.config3_fit_kernels()
    k = MarginalizedGraphKernel(knode, kedge, q=q, backend=HIPBackend(
        real=real), ftol=1e-13 if real is np.float64 else 1e-8)
    if normalized:
        k = Normalization(k)
    return GaussianFieldRegressor(
        RBFOverDistance(KernelInducedDistance(k), 0.3 if normalized else 5.0),
        optimizer=optimizer, smoothing=1e-3, device=device)


#: (values, gradients) relative tolerances.  f64: the two paths read the same
#: kernel matrices and differ in summation order and in the factorisation
#: (torch on the device, LAPACK on the host).  f32: the host path converts
#: the float kernel to double the same way, but the host and device kernel
#: evaluations are separate float solves (cross block vs Gram matrix and
#: diagonal), each good to ~1e-6 relative; distances of nearby graphs
#: amplify that by K / d^2, which reaches ~1e2 on this set.
TOL = {np.float64: (1e-9, 1e-7), np.float32: (1e-3, 1e-2)}


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('normalized', [False, True])
def test_device_matches_host(real, normalized):
    G, y, b = _graphs()
    rv, rg = TOL[real]
    dev, host = _model(real, normalized, 'cuda'), _model(real, normalized,
                                                          'cpu')
    np.testing.assert_allclose(dev.predict(G, y), host.predict(G, y),
                               rtol=rv, atol=rv * 1e-2)
    z, infl = dev.predict(G, y, return_influence=True)
    zh, inflh = host.predict(G, y, return_influence=True)
    np.testing.assert_allclose(z, zh, rtol=rv, atol=rv * 1e-2)
    np.testing.assert_allclose(infl, inflh, rtol=rv, atol=rv * 1e-3)
    for f, args in (('average_label_entropy', (G, b)),
                    ('loocv_error', (G, y))):
        lv, lg = getattr(dev, f)(*args, eval_gradient=True)
        hv, hg = getattr(host, f)(*args, eval_gradient=True)
        assert lv == pytest.approx(hv, rel=rv)
        np.testing.assert_allclose(lg, hg, rtol=rg,
                                   atol=rg * np.abs(hg).max())
        assert getattr(dev, f)(*args) == pytest.approx(hv, rel=rv)


def test_gradient_against_finite_differences():
    """The reference's gradient divides by d + 1e-4 where the derivative of
    d = sqrt(d^2) divides by d: a relative error of 1e-4 / d per element
    (pairs at d = 0 exactly -- duplicate graphs -- contribute zero either
    way).  The nonzero distances of this set are measured below; the
    tolerance is three times 1e-4 over the smallest of them, and no less
    than 1e-5 for the central differences in log theta of step 1e-4.  ALE:
    the gradient is the derivative in log theta; LOOCV: the linear-scale
    columns, i.e. the same divided by exp(theta)."""
    torch = _torch()
    G, y, b = _graphs()
    g = _model(np.float64, False, 'cuda')
    theta = g.weight.theta.copy()
    K = torch.as_tensor(g.weight.metric.kernel.device_gram(list(G)),
                        device='cuda').cpu().numpy()
    kd = K.diagonal()
    D = np.sqrt(np.maximum(0, -K + 0.4999997 * (kd[:, None] + kd[None, :])))
    dmin = D[D > 0].min()
    assert dmin > 1e-2, dmin            # (the data the test needs)
    tol = max(1e-5, 3e-4 / dmin)
    h = 1e-4
    for f, labels, scale in (('average_label_entropy', b, np.ones_like(theta)),
                             ('loocv_error', y, np.exp(theta))):
        _, grad = getattr(g, f)(G, labels, theta=theta, eval_gradient=True)
        fd = []
        for i in range(len(theta)):
            tp, tm = theta.copy(), theta.copy()
            tp[i] += h
            tm[i] -= h
            fd.append((getattr(g, f)(G, labels, theta=tp)
                       - getattr(g, f)(G, labels, theta=tm)) / (2 * h))
        fd = np.array(fd) / scale
        np.testing.assert_allclose(grad, fd, rtol=tol,
                                   atol=tol * np.abs(fd).max())
        g.weight.theta = theta


def test_no_host_kernel_evaluation(monkeypatch):
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    G, y, b = _graphs()
    models = [_model(np.float64, False, 'auto'),
              _model(np.float32, True, 'auto')]

    def refuse(*args, **kwargs):
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', refuse)
        monkeypatch.setattr(cls, 'diag', refuse)
    for g in models:
        g.predict(G, y, return_influence=True)
        g.average_label_entropy(G, b, eval_gradient=True)
        g.loocv_error(G, y, eval_gradient=True)


def test_exponentiation_takes_the_host_path():
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Exponentiation
    from graphdot_amd.metric import KernelInducedDistance
    from graphdot_amd.model.gaussian_field import (GaussianFieldRegressor,
                                                   RBFOverDistance)
    G, y, _ = _graphs()
    G, y = G[:30], y[:30].copy()
    y[:3] = [0.1, -0.2, 0.3]
    knode, kedge, q = cases.config3_fit_kernels()
    k = Exponentiation(MarginalizedGraphKernel(knode, kedge, q=q,
                                               backend='hip'), xi=2.0)
    w = RBFOverDistance(KernelInducedDistance(k), 0.3)
    auto = GaussianFieldRegressor(w, device='auto')
    assert auto._fused() is None
    cpu = GaussianFieldRegressor(w, device='cpu')
    np.testing.assert_allclose(auto.predict(G, y), cpu.predict(G, y),
                               rtol=1e-12)
    with pytest.raises(TypeError, match='MarginalizedGraphKernel'):
        GaussianFieldRegressor(w, device='cuda').predict(G, y)


def test_fit_on_device_matches_host():
    G, y, _ = _graphs()
    out = []
    for device in ('cuda', 'cpu'):
        g = _model(np.float64, False, device, optimizer=True)
        np.random.seed(0)
        g.fit(G, y, loss='loocv2', repeat=1, tol=1e-9)
        out.append(g.weight.theta)
    np.testing.assert_allclose(out[0], out[1], rtol=1e-4, atol=1e-6)
