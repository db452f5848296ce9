"""The Gaussian field regressor and the kernel-induced distance on the host
(graphdot_amd.model.gaussian_field, graphdot_amd.metric): the reference's
recorded results (tests/golden/gaussian_field.json, made by
tests/golden/make_golden_gaussian_field.py), the reference's own tests
restated, the O(N_u N n) gradient against the reference's dense formula,
the distance over a marginalized graph kernel, and a gfx950 build of
field.hip.  No GPU needed."""
import json
import os
import sys
import numpy as np
import pytest
from scipy.spatial.distance import cdist

HERE = os.path.dirname(os.path.abspath(__file__))


sys.path.insert(0, os.path.join(HERE, 'golden'))
from make_golden_gaussian_field import RBF     # noqa: E402 (the golden's kernel)


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'gaussian_field.json')) as f:
        g = json.load(f)
    for k in ('X', 'Y', 'y', 'b'):
        g[k] = np.array(g[k], dtype=float)
    return g


def _weight(g):
    from graphdot_amd.metric import KernelInducedDistance
    from graphdot_amd.model.gaussian_field import RBFOverDistance
    s, l, sigma = g['params']
    return RBFOverDistance(KernelInducedDistance(RBF(s, l)), sigma)


def _gfr(g, smoothing=1e-3, optimizer=None):
    from graphdot_amd.model.gaussian_field import GaussianFieldRegressor
    return GaussianFieldRegressor(_weight(g), optimizer=optimizer,
                                  smoothing=smoothing, device='cpu')


def close(a, b, rtol=1e-10, atol=1e-13):
    np.testing.assert_allclose(np.asarray(a, float), np.asarray(b, float),
                               rtol=rtol, atol=atol)


# -- golden parity -----------------------------------------------------------------
def test_kernel_induced_distance_golden(golden):
    from graphdot_amd.metric import KernelInducedDistance
    s, l, _ = golden['params']
    X, Y = golden['X'], golden['Y']
    d = KernelInducedDistance(RBF(s, l))
    D, dD = d(X, eval_gradient=True)
    close(D, golden['kid_xx'])
    close(dD, golden['kid_xx_grad'])
    D, dD = d(X, Y, eval_gradient=True)
    close(D, golden['kid_xy'])
    close(dD, golden['kid_xy_grad'])
    close(d(X), golden['kid_xx'])
    close(d(X, Y), golden['kid_xy'])
    close(d.theta, np.log([s, l]))
    close(d.clone_with_theta(np.log([2.0, 3.0])).theta, np.log([2.0, 3.0]))
    close(d.theta, np.log([s, l]))                  # (a clone, not a view)


def test_weights_golden(golden):
    from graphdot_amd.model.gaussian_field import RBFOverFixedDistance
    X, Y = golden['X'], golden['Y']
    w = _weight(golden)
    W, dW = w(X, eval_gradient=True)
    close(W, golden['rbf_xx'])
    close(dW, golden['rbf_xx_grad'])
    W, dW = w(X, Y, eval_gradient=True)
    close(W, golden['rbf_xy'])
    close(dW, golden['rbf_xy_grad'])
    Dfix = np.sqrt(((X[:, None, :] - X[None, :, :])**2).sum(-1))
    wf = RBFOverFixedDistance(Dfix, golden['params'][2])
    idx, jdx = golden['fixed_idx'], golden['fixed_jdx']
    W, dW = wf(idx, eval_gradient=True)
    close(W, golden['fixed_xx'])
    close(dW, golden['fixed_xx_grad'])
    close(wf(idx, jdx), golden['fixed_xy'])


def test_predict_golden(golden):
    X, y = golden['X'], golden['y']
    for case in golden['predict']:
        g = _gfr(golden, case['smoothing'])
        close(g.predict(X, y), case['z'])
        z, infl = g.predict(X, y, return_influence=True)
        close(z, case['z_infl'])
        close(infl, case['influence'])


def test_not_positive_definite_golden(golden):
    from graphdot_amd.model.gaussian_field import GaussianFieldRegressor
    c = golden['not_pd']
    y = np.array(c['y'], dtype=float)
    g = GaussianFieldRegressor('precomputed', smoothing=0, device='cpu')
    with pytest.warns(UserWarning, match='not positive definite'):
        z = g.predict(np.array(c['W']), y)
    close(z, c['z'])


def test_losses_golden(golden):
    X, y, b = golden['X'], golden['y'], golden['b']
    for case in golden['ale']:
        g = _gfr(golden, case['smoothing'])
        loss, grad = g.average_label_entropy(X, b, eval_gradient=True)
        close(loss, case['loss'])
        close(grad, case['grad'])
        close(_gfr(golden, case['smoothing']).average_label_entropy(X, b),
              case['loss'])
    for case in golden['loocv']:
        g = _gfr(golden)
        loss, grad = g.loocv_error(X, y, p=case['p'], eval_gradient=True)
        close(loss, case['loss'])
        close(grad, case['grad'])
        close(_gfr(golden).loocv_error(X, y, p=case['p']), case['loss'])
    g = _gfr(golden)
    close(g.loocv_error_1(X, y), golden['loocv'][0]['loss'])
    close(g.loocv_error_2(X, y), golden['loocv'][2]['loss'])


def test_fit_golden(golden):
    X, y, b = golden['X'], golden['y'], golden['b']
    for case in golden['fit']:
        labels = b if case['loss'] == 'ale' else y
        g = _gfr(golden, optimizer=True)
        np.random.seed(0)
        assert g.fit(X, labels, loss=case['loss'], repeat=1) is g
        close(g.weight.theta, case['theta'], rtol=1e-4, atol=1e-6)
        f = (g.average_label_entropy if case['loss'] == 'ale'
             else g.loocv_error_2)(X, labels)
        close(f, case['value'], rtol=1e-4)


def test_fit_errors(golden):
    X, y = golden['X'], golden['y']
    with pytest.raises(RuntimeError, match='Unknown loss'):
        _gfr(golden, optimizer=True).fit(X, y, loss='nope')
    with pytest.raises(RuntimeError, match='All samples are labeled'):
        _gfr(golden).predict(X, np.ones(len(X)))

    def stubborn(fun, x0, **kwargs):
        class R:
            success, x, fun = False, x0, 0.0
        return R()
    g = _gfr(golden, optimizer=stubborn)
    with pytest.raises(RuntimeError, match='Optimizer did not converge'):
        g.fit(X, y)


# -- the reference's own tests, restated --------------------------------------------
class _LookUp:
    def __init__(self, W):
        self.W = W

    def __call__(self, X, Y=None):
        return self.W[X, :][:, X if Y is None else Y]


_PATHS = [
    (np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]]),
     [True, False, True], [[0.5, 0.5]]),
    (np.array([[0.0, 3.0, 0.0], [3.0, 0.0, 1.0], [0.0, 1.0, 0.0]]),
     [True, False, True], [[0.75, 0.25]]),
    (np.array([[0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 1.0, 0.0],
               [0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0]]),
     [True, False, False, True], [[2 / 3, 1 / 3], [1 / 3, 2 / 3]]),
    (np.array([[0.0, 1.0, 1.0, 1.0], [1.0, 0.0, 1.0, 1.0],
               [1.0, 1.0, 0.0, 1.0], [1.0, 1.0, 1.0, 0.0]]),
     [True, True, True, False], [[1 / 3, 1 / 3, 1 / 3]]),
]


@pytest.mark.parametrize('case', _PATHS)
def test_path_graph_prediction_and_influence(case):
    from graphdot_amd.model.gaussian_field import GaussianFieldRegressor
    W, labeled, truth = case
    labeled = np.array(labeled)
    g = GaussianFieldRegressor(_LookUp(W), smoothing=0)
    rng = np.random.default_rng(0)
    for _ in range(20):
        X = np.arange(len(W))
        y = rng.normal(size=len(W))
        y[~labeled] = np.nan
        z = g.fit_predict(X, y)
        assert len(z) == len(y)
        np.testing.assert_allclose(z[~labeled], np.array(truth) @ y[labeled],
                                   atol=1e-4)
    z, influence = g.fit_predict(X, y, return_influence=True)
    assert np.allclose(influence, truth)


def test_average_label_entropy_value():
    from graphdot_amd.model.gaussian_field import GaussianFieldRegressor
    g = GaussianFieldRegressor(weight='precomputed', smoothing=0)
    e = g.average_label_entropy(
        X=np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]]),
        y=np.array([0, np.nan, 1]))
    assert e == pytest.approx(-np.log(0.5))


def test_loocv_error_value():
    from graphdot_amd.model.gaussian_field import GaussianFieldRegressor
    g = GaussianFieldRegressor(weight='precomputed', smoothing=0)
    path = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    full = np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    for y in (np.zeros(3), np.ones(3), -np.ones(3)):
        assert g.loocv_error(X=path, y=y) == pytest.approx(0)
    y = np.array([-1.0, 0.0, 1.0])
    assert g.loocv_error(X=full, y=y, p=1) == pytest.approx(1.0)
    assert g.loocv_error(X=full, y=y, p=2) == pytest.approx(np.sqrt(1.5))


class OneOverRn:
    """w = 1 / (r + a)^b, gradient in log scale (the reference's test
    weight)."""

    def __init__(self, a=0.1, b=1):
        self.a = a
        self.b = b

    def __call__(self, X, Y=None, eval_gradient=False):
        d = self.a + (cdist(X, X) if Y is None else cdist(X, Y))
        w = d**-self.b
        j1 = -self.b * d**(-self.b - 1)
        j2 = -d**(-self.b) * np.log(d)
        if eval_gradient:
            return w, np.stack([j1, j2], axis=2) \
                * np.exp(self.theta)[None, None, :]
        return w

    @property
    def theta(self):
        return np.log([self.a, self.b])

    @theta.setter
    def theta(self, values):
        self.a, self.b = np.exp(values)

    @property
    def bounds(self):
        return np.log([[0.001, 100.0], [0.001, 100.0]])


def _fd(f, theta, eps=1e-3):
    out = []
    for i in range(len(theta)):
        pos, neg = theta.copy(), theta.copy()
        pos[i] += eps
        neg[i] -= eps
        out.append((f(pos) - f(neg)) / (2 * eps))
    return np.array(out)


@pytest.mark.parametrize('n', [4, 7, 25])
@pytest.mark.parametrize('k', [2, 3, 8])
@pytest.mark.parametrize('d', [1, 4, 20])
@pytest.mark.parametrize('loss', ['ale', 1, 1.5, 2, 3])
@pytest.mark.parametrize('smoothing', [0, 0.1, 0.5])
def test_loss_gradient_against_finite_differences(n, k, d, loss, smoothing):
    """(The reference's tests.  OneOverRn's gradient is log-scale and the
    ALE multiplies by exp(theta) again; at a = b = 1 that is a factor 1.)"""
    from graphdot_amd.model.gaussian_field import GaussianFieldRegressor
    rng = np.random.default_rng([n, k, d, int(10 * smoothing)])
    gfr = GaussianFieldRegressor(weight=OneOverRn(a=1.0, b=1.0),
                                 smoothing=smoothing)
    X = rng.normal(size=(n, d))
    y = rng.uniform(size=n)
    y[rng.choice(n, max(1, n // k), replace=False)] = np.nan
    if loss == 'ale':
        f = gfr.average_label_entropy
    else:
        def f(X, y, **kw):
            return gfr.loocv_error(X, y, p=loss, **kw)
    _, dloss = f(X, y, eval_gradient=True)
    theta = np.copy(gfr.weight.theta)
    fd = _fd(lambda t: f(X, y, theta=t), theta)
    np.testing.assert_allclose(dloss, fd, rtol=1e-5, atol=1e-6)


# -- the O(N_u N n) gradient against the reference's dense formula -----------------
def _reference_df_u(L_inv, f_u, f_l, dW_uu, dW_ul):
    """The reference's df_u (gfr.py, `_predict_gradient`): a dense L^-1
    contracted with the whole dW."""
    dL_inv = L_inv * f_u
    return (np.einsum('im,n,mnj->ij', L_inv, f_u, dW_uu, optimize=True)
            + np.einsum('im,n,mnj->ij', L_inv, f_l, dW_ul, optimize=True)
            - np.einsum('imn,mnj->ij', dL_inv[:, :, None], dW_uu)
            - np.einsum('imn,mnj->ij', dL_inv[:, :, None], dW_ul))


@pytest.mark.parametrize('seed', range(6))
def test_rank_structured_gradient_matches_dense(seed):
    from graphdot_amd.model.gaussian_field.gfr import _rank_contract
    rng = np.random.default_rng(seed)
    nu, nl, n = rng.integers(2, 30), rng.integers(1, 30), rng.integers(1, 6)
    W_uu = rng.uniform(size=(nu, nu))
    W_uu = W_uu + W_uu.T
    W_ul = rng.uniform(size=(nu, nl))
    dW_uu = rng.normal(size=(nu, nu, n))
    dW_ul = rng.normal(size=(nu, nl, n))
    f_l = rng.normal(size=nl)
    L = np.diag(W_uu.sum(1) + W_ul.sum(1)) - W_uu
    L_inv = np.linalg.inv(L)
    f_u = L_inv @ (W_ul @ f_l)
    g = rng.normal(size=nu)
    dense = g @ _reference_df_u(L_inv, f_u, f_l, dW_uu, dW_ul)
    v = np.linalg.solve(L, g)
    fast = _rank_contract(dW_uu, -v * f_u, v, f_u) \
        + _rank_contract(dW_ul, -v * f_u, v, f_l)
    np.testing.assert_allclose(fast, dense, rtol=1e-9, atol=1e-11)
    # the LOOCV form of the reference, restated
    W = W_uu + 0.1
    y = rng.normal(size=nu)
    D = W.sum(1)
    derr = rng.normal(size=nu)
    ref = (np.einsum('pq, pqi', (derr / D**2 * (W @ y))[:, None], dW_uu)
           - np.einsum('p, q, pqi', derr / D, y, dW_uu))
    np.testing.assert_allclose(
        _rank_contract(dW_uu, derr / D**2 * (W @ y), -derr / D, y), ref,
        rtol=1e-9, atol=1e-11)


# -- the distance over the marginalized graph kernel --------------------------------
def test_kernel_induced_distance_over_graph_kernel():
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.metric import KernelInducedDistance
    G = cases.config3_graphs(12, seed=3)
    knode, kedge, q = cases.config3_kernels()
    mgk = MarginalizedGraphKernel(knode, kedge, q=q, backend=OracleBackend())

    def diag(Z, eval_gradient=False):
        # (the oracle backend solves pairs only: the self-similarities of
        # Z as the diagonal of its Gram matrix)
        K, dK = mgk(Z, eval_gradient=True)
        return (K.diagonal(), np.einsum('iik->ik', dK)) if eval_gradient \
            else K.diagonal()
    mgk.diag = diag
    X, Y = G[:7], G[7:]
    for kernel in (mgk, Normalization(mgk)):
        d = KernelInducedDistance(kernel)
        KX, dKX = kernel(X, eval_gradient=True)
        kx, dkx = KX.diagonal(), np.einsum('iik->ik', dKX)
        ky, dky = kernel.diag(Y, eval_gradient=True)
        # without Y the diagonal of K(X), with Y kernel.diag (ones for
        # Normalization, whose X diagonal is ~0 in the gradient)
        for Z, (kz, dkz), (kl, dkl) in (
                (None, (kx, dkx), (kx, dkx)),
                (Y, (ky, dky), kernel.diag(X, eval_gradient=True))):
            K, dK = kernel(X, Z, eval_gradient=True)
            D, dD = d(X, Z, eval_gradient=True)
            ref = np.sqrt(np.maximum(
                0, -K + 0.4999997 * (kl[:, None] + kz[None, :])))
            np.testing.assert_allclose(D, ref, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(
                dD, (-dK + 0.5 * dkl[:, None, :] + 0.5 * dkz[None, :, :])
                * (0.5 / (ref + 1e-4))[:, :, None], rtol=1e-12, atol=1e-12)
        # (value-only solves stop at the solver's ftol, the gradient ones
        # converge further: the same distances to ~1e-8)
        np.testing.assert_allclose(d(X, Y), ref, rtol=1e-6, atol=1e-9)


def test_device_path_selection_on_host():
    """What cannot take the fused path runs on the host with 'auto' and is
    refused with 'cuda'; 'cpu' never asks."""
    from graphdot_amd.model.gaussian_field import (
        GaussianFieldRegressor, RBFOverFixedDistance)
    from graphdot_amd.model.gaussian_field.gfr import _fused_reason
    from graphdot_amd.metric import KernelInducedDistance
    w = _weight({'params': (1.0, 1.0, 1.0)})
    assert 'MarginalizedGraphKernel' in _fused_reason(w)
    assert 'RBFOverDistance' in _fused_reason('precomputed')
    assert 'RBFOverDistance' in _fused_reason(
        RBFOverFixedDistance(np.eye(3), 1.0))
    from graphdot_amd.model.gaussian_field import RBFOverDistance
    assert 'KernelInducedDistance' in _fused_reason(
        RBFOverDistance(lambda X, Y=None: None, 1.0))
    assert 'options' in _fused_reason(RBFOverDistance(
        KernelInducedDistance(RBF(), {'nodal': False}), 1.0))
    g = GaussianFieldRegressor(w, device='cuda')
    with pytest.raises(TypeError, match='MarginalizedGraphKernel'):
        g.predict(np.zeros((3, 2)), np.array([1.0, np.nan, 0.0]))
    with pytest.raises(ValueError):
        GaussianFieldRegressor(w, device='gpu')


def test_field_hip_compiles_for_gfx950():
    from graphdot_amd.model.gaussian_field import _field
    path = _field.precompile()
    assert os.path.getsize(path) > 0
