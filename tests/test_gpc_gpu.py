"""The fused device path of GaussianProcessClassifier on an MI355X: every
launch of laplace.hip against its torch restatement (run in double on the
CPU) on the same stored inputs (tile edges, plane counts across the register
chunks, f32 / f64 planes, both plane layouts, bit-identical repeats), the
classifier on the HIP backend against the same classifier forced to its host
path, no host kernel evaluation on the device path, and the host path for a
kernel without `device_gram` or with kernel options.

The margins of device against host are ten times the largest differences
measured on an MI355X, relative to the largest host magnitude of the quantity,
over the four kernels (float / double, plain / normalised) and both thetas:
see the constants, which carry the measured figures."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _torch():
    import torch
    import graphdot_amd.model.gaussian_process  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


# -- the launches against their restatements ------------------------------------------
def _case(n, m, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, n))
    K = A @ A.T / n + 0.1 * np.eye(n)
    P = rng.normal(size=(n, n, m))
    P = P + P.transpose(1, 0, 2)
    y = (rng.uniform(size=n) < 0.5).astype(float)
    return K, P, y, 2.0 * rng.normal(size=n), rng.normal(size=n)


def _inverse(B):
    Binv = np.linalg.inv(B)
    return 0.5 * (Binv + Binv.T)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
def test_step_launches_against_restatements(n):
    """Both sides work in double on the same inputs and differ in the order
    of their sums of n terms -- ``|fl(sum) - sum| <= (n - 1) eps sum
    |terms|`` for any order, twice -- and in the last bits of exp, sqrt and
    log1p, a few eps of each term: ``4 (n + 4) eps sum |terms|``.  What is
    not summed (B, pi, s, g, b) agrees within 8 eps of its terms."""
    torch = _torch()
    from graphdot_amd.model.gaussian_process import _laplace
    K, _, y, f, a = _case(n, 0, n)
    c = 4 * (n + 4) * EPS
    host = (_t(K), _t(f), _t(y), _t(a))
    dev = tuple(t.cuda() for t in host)
    B, vec, sums = _laplace.build(*dev)
    B2, vec2, sums2 = _laplace.build(*dev)
    torch.cuda.synchronize()
    assert torch.equal(B, B2) and torch.equal(vec, vec2) \
        and torch.equal(sums, sums2)              # bit-identical repeats
    B, vec, sums = (t.cpu().numpy() for t in (B, vec, sums))
    rB, rvec, rsums = (t.numpy() for t in _laplace.build_torch(*host))
    pi, s, b, g = (rvec[k * n:(k + 1) * n] for k in range(4))
    np.testing.assert_allclose(B, rB, rtol=8 * EPS, atol=0)
    np.testing.assert_allclose(vec[:2 * n], rvec[:2 * n], rtol=8 * EPS)
    size_b = np.abs(pi * (1 - pi) * f) + np.abs(g)
    assert np.all(np.abs(vec[2 * n:3 * n] - b) <= 8 * EPS * size_b)
    assert np.all(np.abs(vec[3 * n:4 * n] - g) <= 8 * EPS)
    assert np.all(np.abs(vec[4 * n:] - rvec[4 * n:])
                  <= c * (np.abs(K) @ size_b))
    assert abs(sums[0] - rsums[0]) <= c * (np.abs(a) @ np.abs(f))
    assert abs(sums[1] - rsums[1]) <= c * rsums[1]

    Binv = _inverse(rB)
    a1 = _laplace.solve(_t(Binv).cuda(), _t(rvec).cuda())
    a2 = _laplace.solve(_t(Binv).cuda(), _t(rvec).cuda())
    assert torch.equal(a1, a2)
    ra = _laplace.solve_torch(_t(Binv), _t(rvec)).numpy()
    kb = rvec[4 * n:]
    assert np.all(np.abs(a1.cpu().numpy() - ra) <= c * (
        np.abs(b) + s * (np.abs(Binv) @ np.abs(s * kb))))

    f1 = _laplace.apply(dev[0], _t(ra).cuda())
    f2 = _laplace.apply(dev[0], _t(ra).cuda())
    assert torch.equal(f1, f2)
    rf = _laplace.apply_torch(_t(K), _t(ra)).numpy()
    assert np.all(np.abs(f1.cpu().numpy() - rf)
                  <= c * (np.abs(K) @ np.abs(ra)))


def _planes(P, dtype, layout):
    if layout == 'column-major':      # i + n j + n^2 k (device_gram)
        return _t(P.transpose(2, 1, 0).astype(dtype)).permute(2, 1, 0)
    return _t(P.astype(dtype))        # k fastest


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('nt', [0, 1, 3, 7, 17])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('layout', ['column-major', 'row-major'])
def test_contraction_against_restatement(n, nt, dtype, layout):
    """``d_k = sum_ij M_ij P_ijk``: M's entries carry a few eps of their
    four terms ``(|a_i a_j| + |s_i Binv_ij s_j| + |u_i g_j| + |g_i u_j|) / 2
    =: |M|``, and either side's sum over the n^2 products is blocked (lanes,
    waves, tiles; a matrix-vector product) to a depth well below n:
    ``8 (n + 8) eps sum_ij |M|_ij |P_ijk|``."""
    torch = _torch()
    from graphdot_amd.model.gaussian_process import _laplace
    m = nt + 2
    K, P, y, f, _ = _case(n, m, 7 * n + nt)
    planes = list(range(m))[::-1][:nt]       # (a subset, not in order)
    rB, rvec, _ = _laplace.build_torch(_t(K), _t(f), _t(y),
                                       _t(np.zeros(n)))
    Binv = _t(_inverse(rB.numpy()))
    a = _laplace.solve_torch(Binv, rvec)
    u = _laplace.third_order(_t(K), Binv, rvec)
    s, g = rvec[n:2 * n], rvec[3 * n:4 * n]
    Pt = _planes(P, dtype, layout)
    assert n == 1 or Pt.stride(0 if layout == 'column-major' else 2) == 1
    ref = _laplace.contract_torch(Pt, planes, Binv, s, a, u, g).numpy()
    args = (Pt.cuda(), planes, *(t.cuda() for t in (Binv, s, a, u, g)))
    out = _laplace.contract(*args)
    out2 = _laplace.contract(*args)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)              # bit-identical repeats
    out = out.cpu().numpy()
    assert out.shape == ref.shape == (nt,)
    s, a, u, g, Binv = (np.abs(t.numpy()) for t in (s, a, u, g, Binv))
    Mabs = 0.5 * (np.outer(a, a) + s[:, None] * Binv * s[None, :]
                  + np.outer(u, g) + np.outer(g, u))
    stored = np.abs(P.astype(dtype).astype(np.float64))
    for k, j in enumerate(planes):
        bound = 8 * (n + 8) * EPS * (Mabs * stored[:, :, j]).sum()
        assert abs(out[k] - ref[k]) <= bound, (k, out[k], ref[k], bound)


def test_contraction_checks_its_arguments():
    torch = _torch()
    from graphdot_amd.model.gaussian_process import _laplace
    n = 5
    v = torch.zeros(n, dtype=torch.float64, device='cuda')
    Binv = torch.eye(n, dtype=torch.float64, device='cuda')
    P = torch.zeros((n, n, 2), device='cuda')
    with pytest.raises(IndexError):
        _laplace.contract(P, [2], Binv, v, v, v, v)
    with pytest.raises(TypeError):
        _laplace.contract(P.to(torch.float16), [0], Binv, v, v, v, v)
    with pytest.raises(TypeError):
        _laplace.contract(P, [0], Binv.cpu(), v, v, v, v)
    assert _laplace.contract(None, [], Binv, v, v, v, v).shape == (0,)


# -- the classifier on QM7-like graphs ----------------------------------------------
#: device against host, relative to the largest host magnitude of the
#: quantity: ten times the largest difference measured on an MI355X over the
#: eight (kernel, theta) cases.  The largest ones all
#: come from the plain kernel, whose B is badly conditioned (the two paths
#: stop after 9 to 11 Newton steps, not always the same number); under
#: `Normalization` every figure is below 2e-13.
RTOL_VALUE = 1.2e-10         # measured 1.17e-11 (float, plain, theta 1)
RTOL_GRAD = 2.5e-8           # measured 2.51e-9 (double, plain, theta 1)
RTOL_LATENT = 1.0e-5         # measured 1.04e-6 (float, plain, theta 1)
RTOL_PROBA = 7.5e-6          # measured 7.48e-7 (float, plain, theta 1)
RTOL_FIT_VALUE = 2.6e-8      # measured 2.59e-9 (double, plain)

N_TRAIN, N_HELD_OUT = 90, 10


def _graphs():
    import cases
    G = list(cases.config3_graphs(N_TRAIN + N_HELD_OUT, seed=23))
    e = cases.synthetic_energies(G)[:N_TRAIN]
    G = np.asarray(G, dtype=object)
    return G[:N_TRAIN], (e > np.median(e)).astype(int), G[N_TRAIN:]


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


def _pair(kernel, **kwargs):
    """(the classifier on the device path, the same forced to the host)."""
    from graphdot_amd.model.gaussian_process import GaussianProcessClassifier
    dev = GaussianProcessClassifier(kernel, **kwargs)
    dev.device = 'cuda'
    host = GaussianProcessClassifier(kernel, **kwargs)
    host.device = 'cpu'
    return dev, host


def _close(name, got, want, rtol):
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f'{name}: largest difference {err:.3g} of the largest magnitude')
    assert got.shape == want.shape and np.all(np.isfinite(got))
    assert err <= rtol, (name, err, rtol)


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('transform', ['plain', 'normalized'])
def test_device_matches_host(real, transform):
    G, y, Z = _graphs()
    kernel = _kernel(real, transform)
    theta0 = np.array(kernel.theta)
    lo, hi = np.asarray(kernel.bounds, dtype=float).T
    thetas = (theta0, np.clip(theta0 + 0.3 * np.cos(np.arange(len(theta0))),
                              lo, hi))
    for k, theta in enumerate(thetas):
        dev, host = _pair(kernel.clone_with_theta(theta))
        out = {}
        for name, m in (('device', dev), ('host', host)):
            m.fit(G, y)
            v, g = m.log_marginal_likelihood(theta, eval_gradient=True)
            assert m.last_timing['fused'] is (name == 'device')
            f, std = m.latent(Z, return_std=True)
            out[name] = (v, g, np.concatenate((f, std)), m.predict_proba(Z),
                         m.predict(Z), m.last_timing['newton_steps'])
        d, h = out['device'], out['host']
        print(f'{real.__name__} {transform} theta {k}: objective {h[0]:.6g}, '
              f'Newton steps {d[5]} / {h[5]}')
        _close('objective', d[0], h[0], RTOL_VALUE)
        _close('gradient', d[1], h[1], RTOL_GRAD)
        _close('latent', d[2], h[2], RTOL_LATENT)
        _close('probabilities', d[3], h[3], RTOL_PROBA)
        assert d[3].shape == (N_HELD_OUT, 2)
        assert set(d[4]) <= {0, 1}


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('transform', ['plain', 'normalized'])
def test_short_fit_matches_host(real, transform):
    G, y, _ = _graphs()
    out = {}
    for name in ('device', 'host'):
        m = _pair(_kernel(real, transform), optimizer=True)[name == 'host']
        start = m.log_marginal_likelihood(X=G, y=y)
        m.fit(G, y, tol=1e-2)
        assert m.log_marginal_likelihood_value_ > start
        out[name] = (m.log_marginal_likelihood_value_,
                     m.optimization_result.nfev)
    print(f'{real.__name__} {transform}: evaluations '
          f'{out["device"][1]} / {out["host"][1]}')
    _close('final objective', out['device'][0], out['host'][0],
           RTOL_FIT_VALUE)


def test_no_host_round_trip(monkeypatch):
    """The device path never calls the kernel's numpy `__call__`."""
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    G, y, Z = _graphs()
    models = [_pair(_kernel(r, t))[0] for r, t in (
        (np.float64, 'plain'), (np.float32, 'normalized'))]
    calls = []

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
    for m in models:
        v, g = m.log_marginal_likelihood(m.kernel.theta, X=G, y=y,
                                         eval_gradient=True)
        assert np.isfinite(v) and np.all(np.isfinite(g))
        assert m.last_timing['fused'] is True
        m.fit(G, y)
        assert np.all(np.isfinite(m.predict_proba(Z)))
    assert calls == []


def test_timing_script_times_every_launch():
    """scripts/time_gpc.py drives the launches through the same protocol and
    launch functions as the classifier; this is its only cover."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), 'scripts', 'time_gpc.py')
    spec = importlib.util.spec_from_file_location('time_gpc', path)
    time_gpc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(time_gpc)
    G, y, _ = _graphs()
    kernel = _kernel(np.float64, 'normalized')
    out = time_gpc.launches(kernel, G, y)
    assert out['planes'] == len(kernel.theta)
    for kind in ('lp_build', 'potrf', 'lp_solve', 'lp_apply',
                 'third_order_torch', 'lp_planes_reduce'):
        assert out[f'{kind}_ms'] > 0


class _HostOnly:
    """A kernel that offers the protocol's host methods alone."""

    def __init__(self, kernel):
        self.kernel = kernel

    def __call__(self, X, Y=None, eval_gradient=False, **options):
        return self.kernel(X, Y, eval_gradient=eval_gradient, **options)

    def diag(self, X, **options):
        return self.kernel.diag(X, **options)

    theta = property(lambda self: self.kernel.theta,
                     lambda self, t: setattr(self.kernel, 'theta', t))
    bounds = property(lambda self: self.kernel.bounds)

    def clone_with_theta(self, theta):
        return _HostOnly(self.kernel.clone_with_theta(theta))


@pytest.mark.parametrize('how', ['no device_gram', 'kernel_options'])
def test_host_path_where_the_device_path_does_not_apply(how):
    from graphdot_amd.model.gaussian_process import GaussianProcessClassifier
    G, y, Z = _graphs()
    kernel = _kernel(np.float64, 'normalized')
    dev, _ = _pair(kernel)
    if how == 'no device_gram':
        other = GaussianProcessClassifier(_HostOnly(kernel))
    else:
        other = GaussianProcessClassifier(kernel, kernel_options={'lmin': 0})
    other.device = 'cuda'
    out = []
    for m in (dev, other):
        m.fit(G, y)
        v, g = m.log_marginal_likelihood(kernel.theta, eval_gradient=True)
        out.append((v, g, m.predict_proba(Z), m.last_timing['fused']))
    assert out[0][3] is True and out[1][3] is False
    _close('objective', out[1][0], out[0][0], RTOL_VALUE)
    _close('gradient', out[1][1], out[0][1], RTOL_GRAD)
    _close('probabilities', out[1][2], out[0][2], RTOL_PROBA)
