"""GPROutlierDetector on the CPU: parity with values recorded from the
reference (tests/golden/make_golden_outlier_detector.py), the reference's
own two tests restated, which inverse path is taken, masked targets, the two
reference crashes that are not kept, and save / load."""
import json
import os
import numpy as np
import pytest

from graphdot_amd.model.gaussian_process import GPROutlierDetector

HERE = os.path.dirname(os.path.abspath(__file__))


class RBFKernel:
    """The reference test's kernel: v exp(-d^2 / 2 L^2), gradient columns
    d/dv and d/dL."""

    def __init__(self, v, L):
        self.v = v
        self.L = L

    def __call__(self, X, Y=None, eval_gradient=False):
        v, L = self.v, self.L
        d = np.subtract.outer(X, Y if Y is not None else X)
        f = v * np.exp(-0.5 * d**2 / L**2)
        if eval_gradient is False:
            return f
        j1 = np.exp(-0.5 * d**2 / L**2)
        j2 = v * np.exp(-0.5 * d**2 / L**2) * d**2 * L**-3
        return f, np.stack((j1, j2), axis=2)

    def diag(self, X):
        return np.ones_like(X)

    @property
    def theta(self):
        return np.log([self.v, self.L])

    @theta.setter
    def theta(self, t):
        self.v, self.L = np.exp(t)

    @property
    def bounds(self):
        return np.log([[1e-5, 1e5], [1e-2, 10]])

    def clone_with_theta(self, theta):
        k = RBFKernel(1.0, 1.0)
        k.theta = theta
        return k


def _golden():
    with open(os.path.join(HERE, 'golden', 'outlier_detector.json')) as f:
        return json.load(f)


def _data():
    X = np.linspace(-1, 1, 12, endpoint=False)
    y = np.sin(X * np.pi)
    y[3] += 0.5
    y[7] -= 0.4
    return X, y


def _theta_ext(v, L, sigma, n=12):
    return np.concatenate((np.log([v, L]), np.log(np.full(n, sigma))))


# -- parity with the reference -----------------------------------------------------
@pytest.mark.parametrize('case', range(7))
def test_log_marginal_likelihood_matches_reference(case):
    g = _golden()
    c = g['lml'][case]
    gpr = GPROutlierDetector(RBFKernel(c['v'], c['L']),
                             normalize_y=c['normalize_y'], device='cpu')
    gpr.X, gpr.y = np.array(g['X']), np.array(g['y'])
    value, grad = gpr.log_marginal_likelihood(np.array(c['theta_ext']),
                                              eval_gradient=True)
    # the two inverses (Cholesky or eigh here, LAPACK's eigh there) agree
    # to about cond(K) times the rounding unit
    tol = max(1e-9, 1e-14 * c['cond'])
    assert value == pytest.approx(c['value'], rel=tol)
    ref = np.array(c['grad'])
    np.testing.assert_allclose(grad, ref, rtol=tol,
                               atol=tol * np.abs(ref).max())
    if c['clamped']:
        assert gpr.last_timing['path'] == 'eigh'


@pytest.mark.parametrize('case', range(3))
def test_fit_matches_reference(case):
    g = _golden()
    c = g['fit'][case]
    X, y, Z = np.array(g['X']), np.array(g['y']), np.array(g['Z'])
    gpr = GPROutlierDetector(RBFKernel(1.0, 1.0),
                             normalize_y=c['normalize_y'], device='cpu')
    np.random.seed(c['seed'])
    gpr.fit(X, y, w=c['w'], repeat=c['repeat'], theta_jitter=1.0)
    # (the optimiser's path amplifies the rounding of each evaluation)
    np.testing.assert_allclose(gpr.kernel.theta, c['theta'], rtol=1e-3,
                               atol=1e-3)
    np.testing.assert_allclose(gpr.y_uncertainty, c['y_uncertainty'],
                               rtol=2e-2, atol=2e-4)
    mean, std = gpr.predict(Z, return_std=True)
    _, cov = gpr.predict(Z, return_cov=True)
    np.testing.assert_allclose(mean, c['mean'], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(std, c['std'], rtol=1e-2, atol=1e-3)
    np.testing.assert_allclose(cov, c['cov'], rtol=1e-2, atol=1e-4)


# -- the reference's own tests ---------------------------------------------------
@pytest.mark.parametrize('v', [0.25, 0.5, 1.0, 2.0, 5.0])
@pytest.mark.parametrize('L', np.logspace(-1, 0.5, 10))
def test_gradient_against_finite_differences(v, L):
    eps = 1e-4
    X = np.linspace(-1, 1, 6, endpoint=False)
    y = np.sin(X * np.pi)
    gpr = GPROutlierDetector(RBFKernel(v, L), device='cpu')
    theta_ext0 = _theta_ext(v, L, 0.01, len(y))
    _, dL = gpr.log_marginal_likelihood(theta_ext0, X=X, y=y,
                                        eval_gradient=True)
    for i in range(len(theta_ext0)):
        tn, tp = theta_ext0.copy(), theta_ext0.copy()
        tn[i] -= eps
        tp[i] += eps
        fd = (gpr.log_marginal_likelihood(tp, X=X, y=y)
              - gpr.log_marginal_likelihood(tn, X=X, y=y)) / (2 * eps)
        assert dL[i] == pytest.approx(fd, 1e-3, 1e-3)


def test_outlier_detection():
    X = np.linspace(-1, 1, 12, endpoint=False)
    y = np.sin(X * np.pi)
    y[3] += 0.5
    y[7] -= 0.4
    np.random.seed(0)
    gpr = GPROutlierDetector(RBFKernel(1.0, 1.0), device='cpu')
    gpr.fit(X, y, w=0.0, repeat=7, theta_jitter=1.0)
    for i, u in enumerate(gpr.y_uncertainty):
        if i in (3, 7):
            assert u > 0.2
        else:
            assert u < 0.01


# -- which inverse ---------------------------------------------------------------
@pytest.mark.parametrize('sigma,path', [(0.1, 'A'), (3.8e-4, 'B'),
                                        (1e-4, 'eigh')])
def test_inverse_path(monkeypatch, sigma, path):
    import torch
    X, y = _data()
    calls = []
    eigh = torch.linalg.eigh

    def counted(*args, **kwargs):
        calls.append(1)
        return eigh(*args, **kwargs)
    monkeypatch.setattr(torch.linalg, 'eigh', counted)
    gpr = GPROutlierDetector(RBFKernel(1.0, 1.0), device='cpu')
    value, grad = gpr.log_marginal_likelihood(_theta_ext(1.0, 1.0, sigma),
                                              X=X, y=y, eval_gradient=True)
    assert gpr.last_timing['path'] == path
    assert len(calls) == (path == 'eigh')
    # the same numbers as the reference's clamped eigendecomposition
    K = RBFKernel(1.0, 1.0)(X) + sigma**2 * np.eye(len(X))
    a, Q = np.linalg.eigh(K)
    a = np.where(a > 1e-8 * a.max(), a, 1e-8 * a.max())
    Kinv = (Q / a) @ Q.T
    cond = a.max() / a.min()
    assert value == pytest.approx(y @ Kinv @ y + np.log(a).sum(),
                                  rel=1e-13 * cond)
    if path != 'eigh':
        assert a.min() > 1e-8 * a.max()      # (the certificate's claim)


def test_certificates_are_sufficient():
    """Whenever a certificate passes, the clamp changes nothing."""
    from graphdot_amd.model.gaussian_process.outlier_detector import _Inverse
    X, y = _data()
    rng = np.random.default_rng(0)
    for _ in range(40):
        v, L = np.exp(rng.uniform(-1, 1.5)), np.exp(rng.uniform(-1.5, 0.5))
        sigma = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), len(X)))
        K = RBFKernel(v, L)(X) + np.diag(sigma**2)
        a = np.linalg.eigvalsh(K)
        nK = np.abs(K).sum(1).max()
        if _Inverse.certified(nK, np.abs(np.linalg.inv(K)).sum(1).max(),
                              1e-8):
            assert a.min() > 1e-8 * a.max()
        if np.all(np.linalg.eigvalsh(K - 1e-8 * nK * np.eye(len(X))) > 0):
            assert a.min() > 1e-8 * a.max()


# -- masked targets, decided crashes, persistence --------------------------------
def test_masked_targets_equal_the_subset():
    X, y = _data()
    ym = y.astype(object)
    ym[[2, 9]] = None
    ym[5] = np.nan
    keep = np.ones(len(y), bool)
    keep[[2, 5, 9]] = False
    a = GPROutlierDetector(RBFKernel(1.0, 1.0), device='cpu')
    b = GPROutlierDetector(RBFKernel(1.0, 1.0), device='cpu')
    te = _theta_ext(1.0, 1.0, 0.05, keep.sum())
    va, ga = a.log_marginal_likelihood(te, X=X, y=ym, eval_gradient=True)
    vb, gb = b.log_marginal_likelihood(te, X=X[keep], y=y[keep],
                                       eval_gradient=True)
    assert va == vb
    assert np.array_equal(ga, gb)
    np.random.seed(4)
    a.fit(X, ym, w=0.01, repeat=2)
    np.random.seed(4)
    b.fit(X[keep], y[keep], w=0.01, repeat=2)
    assert len(a.y_uncertainty) == keep.sum()
    np.testing.assert_array_equal(a.y_uncertainty, b.y_uncertainty)
    np.testing.assert_array_equal(a.kernel.theta, b.kernel.theta)
    Z = np.linspace(-1, 1, 5)
    np.testing.assert_array_equal(a.predict(Z, return_std=True),
                                  b.predict(Z, return_std=True))


def test_fit_without_optimizer_raises():
    X, y = _data()
    gpr = GPROutlierDetector(RBFKernel(1.0, 1.0), optimizer=None,
                             device='cpu')
    with pytest.raises(RuntimeError, match='needs an optimizer'):
        gpr.fit(X, y, w=0.0)
    with pytest.raises(AttributeError, match='learned via fit'):
        gpr.y_uncertainty
    with pytest.raises(RuntimeError, match='not trained'):
        gpr.predict(X)


def test_verbose_without_gradient(capsys):
    X, y = _data()
    gpr = GPROutlierDetector(RBFKernel(1.0, 1.0), device='cpu')
    value = gpr.log_marginal_likelihood(_theta_ext(1.0, 1.0, 0.1), X=X, y=y,
                                        verbose=True)
    out = capsys.readouterr().out
    assert 'logP' in out and 'dlogP' not in out
    assert np.isfinite(value)
    gpr.log_marginal_likelihood(_theta_ext(1.0, 1.0, 0.1), X=X, y=y,
                                eval_gradient=True, verbose=True)
    assert 'dlogP' in capsys.readouterr().out


def test_theta_ext_length_is_checked():
    X, y = _data()
    gpr = GPROutlierDetector(RBFKernel(1.0, 1.0), device='cpu')
    with pytest.raises(ValueError, match='noise levels'):
        gpr.log_marginal_likelihood(np.zeros(5), X=X, y=y)


def test_save_load(tmp_path):
    X, y = _data()
    np.random.seed(0)
    gpr = GPROutlierDetector(RBFKernel(1.0, 1.0), device='cpu')
    gpr.fit(X, y, w=0.0, repeat=2)
    gpr.save(str(tmp_path))
    with pytest.raises(RuntimeError, match='already exists'):
        gpr.save(str(tmp_path))
    other = GPROutlierDetector(RBFKernel(2.0, 0.3), device='cpu')
    other.load(str(tmp_path))
    np.testing.assert_array_equal(other.kernel.theta, gpr.kernel.theta)
    np.testing.assert_array_equal(other.y_uncertainty, gpr.y_uncertainty)
    Z = np.linspace(-1, 1, 9)
    np.testing.assert_array_equal(other.predict(Z, return_cov=True)[1],
                                  gpr.predict(Z, return_cov=True)[1])


def test_epilogue_torch_matches_numpy():
    """The torch form of the fused epilogue (the CPU path) against the
    formulas, with a subset of planes in a different order."""
    import torch
    from graphdot_amd.model.gaussian_process._outlier import epilogue_torch
    rng = np.random.default_rng(1)
    n, m = 17, 5
    A = rng.normal(size=(n, n))
    Ks = A @ A.T + n * np.eye(n)
    Kinv = np.linalg.inv(Ks)
    y, s2 = rng.normal(size=n), rng.uniform(0.1, 1, n)
    P = rng.normal(size=(n, n, m))
    P = P + P.transpose(1, 0, 2)
    planes = [3, 0, 4]
    out = epilogue_torch(torch.from_numpy(Kinv), torch.from_numpy(Ks), y, s2,
                         torch.from_numpy(np.asfortranarray(P)),
                         planes).numpy()
    a = Kinv @ y
    W = Kinv - np.outer(a, a)
    ref = np.concatenate((
        [y @ a, np.abs(Ks).sum(1).max(), np.abs(Kinv).sum(1).max()],
        np.einsum('ij,ijk->k', W, P[:, :, planes]),
        (np.diag(Kinv) - a**2) * 2 * s2))
    np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-12)
