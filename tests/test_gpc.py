"""GaussianProcessClassifier on its host path (no GPU needed) against what
scikit-learn's classifier gave (tests/golden/gpc.json, recorded by
tests/golden/make_golden_gpc.py), its handling of labels, warm starts and
persistence, its gradient against central differences, and the torch
restatements of laplace.hip's launches against plain numpy.

Each tolerance against the recorded numbers is ten times the largest
difference measured for that quantity over all cases (double arithmetic on
both sides; the sums differ in their order only).  Measured, relative to the
largest recorded magnitude of the quantity: objective 1.7e-16, gradient
1.4e-15, pi 4.9e-16, probabilities 5.6e-13 (their five terms are of the order
of 10^3 and cancel to the order of 1), the fit's final objective 7.2e-16."""
import json
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_golden_gpc as recorded      # noqa: E402

RTOL_VALUE = 1.7e-15
RTOL_GRAD = 1.4e-14
RTOL_PI = 4.9e-15
RTOL_PROBA = 5.6e-12
RTOL_FIT_VALUE = 7.2e-15


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'gpc.json')) as f:
        return json.load(f)


def _classifier(kernel, **kwargs):
    from graphdot_amd.model.gaussian_process import GaussianProcessClassifier
    gpc = GaussianProcessClassifier(kernel, **kwargs)
    gpc.device = 'cpu'
    return gpc


def _close(name, got, want, rtol):
    got, want = np.asarray(got, float), np.asarray(want, float)
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print(f'{name}: largest difference {err:.3g} of the largest magnitude')
    assert got.shape == want.shape
    assert err <= rtol, (name, err, rtol)


# -- against scikit-learn ----------------------------------------------------------
@pytest.mark.parametrize('case', range(len(recorded.THETAS)))
def test_points_reproduce_scikit_learn(golden, case):
    p = golden['points']
    X, y, Z = (np.array(p[k]) for k in 'XyZ')
    at = p['at'][case]
    assert at['theta'] == recorded.THETAS[case]
    gpc = _classifier(recorded.ConstantRBF(*np.exp(at['theta'])))
    gpc.fit(X, y)
    value, grad = gpc.log_marginal_likelihood(at['theta'], eval_gradient=True)
    _close('objective', value, at['value'], RTOL_VALUE)
    _close('objective after fit', gpc.log_marginal_likelihood_value_,
           at['value'], RTOL_VALUE)
    _close('gradient', grad, at['grad'], RTOL_GRAD)
    _close('pi', gpc.pi_, at['pi'], RTOL_PI)
    proba = gpc.predict_proba(Z)
    _close('probabilities', proba, at['proba'], RTOL_PROBA)
    assert list(gpc.classes_) == [0, 1]
    assert np.array_equal(gpc.predict(Z), (proba[:, 1] > 0.5).astype(int))


def test_fit_reproduces_scikit_learn(golden):
    """L-BFGS-B with scipy's own stopping rule (``tol=None``), as
    scikit-learn calls it, from the recorded start."""
    p = golden['points']
    X, y = np.array(p['X']), np.array(p['y'])
    gpc = _classifier(recorded.ConstantRBF(*np.exp(p['fit']['start'])),
                      optimizer=True)
    gpc.fit(X, y, tol=None)
    assert gpc.optimization_result.success
    _close('final objective', gpc.log_marginal_likelihood_value_,
           p['fit']['value'], RTOL_FIT_VALUE)
    assert -gpc.optimization_result.fun == pytest.approx(
        gpc.log_marginal_likelihood_value_, rel=1e-12)


def _stored(q):
    return recorded.Stored(q['K_all'], q['dK'], q['theta'],
                           np.array(q['bounds']))


def test_graphs_reproduce_scikit_learn(golden):
    q = golden['graphs']
    n, held = len(q['labels']), len(q['proba'])
    assert (n, held) == (recorded.N_GRAPHS, recorded.N_HELD_OUT)
    gpc = _classifier(_stored(q))
    gpc.fit(np.arange(n), q['labels'])
    value, grad = gpc.log_marginal_likelihood(q['theta'], eval_gradient=True)
    assert len(grad) == len(q['theta']) >= 5
    _close('objective', value, q['value'], RTOL_VALUE)
    _close('gradient', grad, q['grad'], RTOL_GRAD)
    _close('pi', gpc.pi_, q['pi'], RTOL_PI)
    _close('probabilities', gpc.predict_proba(n + np.arange(held)),
           q['proba'], RTOL_PROBA)


# -- labels -----------------------------------------------------------------------
def _points(golden):
    p = golden['points']
    return np.array(p['X']), np.array(p['y']), np.array(p['Z'])


def test_labels_of_any_hashable_type(golden):
    X, y, Z = _points(golden)
    plain = _classifier(recorded.ConstantRBF()).fit(X, y)
    names = _classifier(recorded.ConstantRBF()).fit(
        X, ['toxic' if v else 'benign' for v in y])
    assert names.classes_ == ['benign', 'toxic']
    assert np.array_equal(names.y, y)
    assert np.array_equal(names.predict_proba(Z), plain.predict_proba(Z))
    assert np.array_equal(names.predict(Z) == 'toxic', plain.predict(Z) == 1)
    value = names.log_marginal_likelihood(
        names.kernel.theta, X=X[:20], y=['toxic' if v else 'benign'
                                         for v in y[:20]])
    assert np.isfinite(value)
    with pytest.raises(ValueError, match='not among the classes'):
        names.log_marginal_likelihood(names.kernel.theta, X=X[:2],
                                      y=['toxic', 'inert'])


def test_masked_labels_drop_their_samples(golden):
    X, y, Z = _points(golden)
    labels = [float(v) for v in y]
    labels[3], labels[17] = None, float('nan')
    keep = np.ones(len(y), dtype=bool)
    keep[[3, 17]] = False
    masked = _classifier(recorded.ConstantRBF()).fit(X, labels)
    subset = _classifier(recorded.ConstantRBF()).fit(X[keep], y[keep])
    assert masked.classes_ == [0.0, 1.0]
    assert len(masked.pi_) == keep.sum()
    assert masked.log_marginal_likelihood_value_ == \
        subset.log_marginal_likelihood_value_
    assert np.array_equal(masked.predict_proba(Z), subset.predict_proba(Z))
    v, g = masked.log_marginal_likelihood([0.3, -0.2], eval_gradient=True)
    w, h = subset.log_marginal_likelihood([0.3, -0.2], eval_gradient=True)
    assert v == w and np.array_equal(g, h)


@pytest.mark.parametrize('labels', [[1] * 40, [None] * 39 + [1],
                                    [0, 1, 2] * 13 + [0]])
def test_one_class_or_three_raise(golden, labels):
    X, _, _ = _points(golden)
    with pytest.raises(ValueError, match='binary classifier'):
        _classifier(recorded.ConstantRBF()).fit(X, labels)


def test_untrained_model_raises(golden):
    _, _, Z = _points(golden)
    with pytest.raises(RuntimeError, match='not trained'):
        _classifier(recorded.ConstantRBF()).predict_proba(Z)


def test_objective_of_an_unfitted_model_leaves_it_unfitted(golden):
    """Labels given to `log_marginal_likelihood` before any `fit` are sorted
    for that call alone: other labels may follow."""
    X, y, _ = _points(golden)
    gpc = _classifier(recorded.ConstantRBF())
    theta = gpc.kernel.theta
    value = gpc.log_marginal_likelihood(theta, X=X, y=y)
    assert not hasattr(gpc, 'classes_')
    named = gpc.log_marginal_likelihood(
        theta, X=X, y=['toxic' if v else 'benign' for v in y])
    assert named == value == _classifier(
        recorded.ConstantRBF()).fit(X, y).log_marginal_likelihood_value_


# -- warm start, persistence --------------------------------------------------------
def test_warm_start_begins_at_the_last_mode(golden):
    """The search stops once a step raises the objective by less than 1e-10
    and Newton's steps shrink quadratically, so what is left above the
    returned value is below that too: a search begun at the mode agrees with
    one begun at zero within 2e-10, in fewer steps."""
    X, y, _ = _points(golden)
    theta = recorded.THETAS[1]
    cold = _classifier(recorded.ConstantRBF())
    cold.fit(X, y)
    v_cold = cold.log_marginal_likelihood(theta)
    steps_cold = cold.last_timing['newton_steps']
    assert cold.log_marginal_likelihood(theta) == v_cold
    assert cold.last_timing['newton_steps'] == steps_cold
    warm = _classifier(recorded.ConstantRBF(), warm_start=True)
    warm.fit(X, y)
    warm.log_marginal_likelihood(theta)       # (from another theta's mode)
    v_warm = warm.log_marginal_likelihood(theta)
    assert warm.last_timing['newton_steps'] < steps_cold
    assert abs(v_warm - v_cold) <= 2e-10


def test_save_and_load(golden, tmp_path):
    X, y, Z = _points(golden)
    gpc = _classifier(recorded.ConstantRBF(2.0, 0.7)).fit(
        X, ['b' if v else 'a' for v in y])
    gpc.save(str(tmp_path))
    with pytest.raises(RuntimeError, match='already exists'):
        gpc.save(str(tmp_path))
    fresh = _classifier(recorded.ConstantRBF())
    fresh.load(str(tmp_path))
    assert np.array_equal(fresh.kernel.theta, gpc.kernel.theta)
    assert fresh.classes_ == ['a', 'b']
    assert np.array_equal(fresh.predict_proba(Z), gpc.predict_proba(Z))
    assert np.array_equal(fresh.predict(Z), gpc.predict(Z))
    f, std = fresh.latent(Z, return_std=True)
    assert np.array_equal(f, gpc.latent(Z)) and np.all(std >= 0)
    assert fresh.log_marginal_likelihood() == gpc.log_marginal_likelihood()


def test_variance_is_clamped_at_zero(golden):
    """A candidate that is a training point of a sharply peaked posterior
    may come out with ``k** - k*^T R k*`` a rounding error below zero:
    the standard deviation is 0 there and the probability finite."""
    X, y, _ = _points(golden)
    gpc = _classifier(recorded.ConstantRBF(1e4, 1.0)).fit(X, y)
    f, std = gpc.latent(X, return_std=True)
    assert np.all(np.isfinite(std)) and np.all(std >= 0)
    assert np.all(np.isfinite(gpc.predict_proba(X)))
    gpc.R = gpc.R * (1 + 2e-2)          # (... and pushed below zero outright)
    Ks = gpc.kernel(X[:3], X)
    assert np.all(gpc.kernel.diag(X[:3])
                  - np.einsum('ij,jk,ik->i', Ks, gpc.R, Ks) < 0)
    assert np.array_equal(gpc.latent(X[:3], return_std=True)[1], np.zeros(3))
    assert np.all(np.isfinite(gpc.predict_proba(X[:3])))


# -- the gradient ----------------------------------------------------------------------
def test_gradient_against_central_differences(golden):
    """Central differences of step h = 1e-3 in log-theta: truncation
    ``h^2 |Z'''| / 6`` and, since the mode search leaves up to 1e-10 of the
    objective unresolved, noise ``1e-10 / h = 1e-7``.  With third
    derivatives of the order of the gradient itself that is within
    ``1e-6 (1 + max |gradient|)``."""
    h = 1e-3
    X, y, _ = _points(golden)
    gpc = _classifier(recorded.ConstantRBF())
    theta = np.array([0.4, -0.3])
    value, grad = gpc.log_marginal_likelihood(theta, X=X, y=y,
                                              eval_gradient=True)
    assert value == gpc.log_marginal_likelihood(theta, X=X, y=y)
    numeric = np.empty_like(grad)
    for k in range(len(theta)):
        e = np.zeros_like(theta)
        e[k] = h
        numeric[k] = (gpc.log_marginal_likelihood(theta + e, X=X, y=y)
                      - gpc.log_marginal_likelihood(theta - e, X=X, y=y)) \
            / (2 * h)
    err = np.abs(numeric - grad).max()
    print(f'central differences: {err:.3g}, gradient {np.abs(grad).max():.3g}')
    assert err <= 1e-6 * (1 + np.abs(grad).max())


# -- the restatements of laplace.hip against plain numpy ------------------------------
def _case(n, m, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, n))
    K = A @ A.T / n + 0.1 * np.eye(n)
    P = rng.normal(size=(n, n, m))
    P = P + P.transpose(1, 0, 2)
    y = (rng.uniform(size=n) < 0.5).astype(float)
    return K, P, y, rng.normal(size=n), rng.normal(size=n)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize('n', [1, 5, 70])
def test_step_restatements_against_numpy(n):
    """Every sum here has n terms of double products: within ``4 n eps``
    of the sum of the terms' magnitudes."""
    from graphdot_amd.model.gaussian_process import _laplace
    eps = np.finfo(float).eps
    K, _, y, f, a = _case(n, 0, n)
    B, vec, sums = (t.numpy() for t in _laplace.build_torch(
        _t(K), _t(f), _t(y), _t(a)))
    pi = 1 / (1 + np.exp(-f))
    w = pi * (1 - pi)
    s = np.sqrt(w)
    b = w * f + (y - pi)
    np.testing.assert_allclose(B, np.eye(n) + s[:, None] * K * s[None, :],
                               rtol=8 * eps, atol=0)
    np.testing.assert_allclose(vec[:4 * n], np.concatenate((pi, s, b, y - pi)),
                               rtol=0, atol=8 * eps)
    bound = 4 * n * eps
    assert np.all(np.abs(vec[4 * n:] - K @ b) <= bound * (np.abs(K) @ np.abs(b)))
    terms = np.log1p(np.exp(-(2 * y - 1) * f))
    assert abs(sums[0] - a @ f) <= bound * (np.abs(a) @ np.abs(f))
    assert abs(sums[1] - terms.sum()) <= bound * terms.sum()
    Binv = np.linalg.inv(B)
    Binv = 0.5 * (Binv + Binv.T)
    got = _laplace.solve_torch(_t(Binv), _t(vec)).numpy()
    kb = vec[4 * n:]
    want = b - s * (Binv @ (s * kb))
    assert np.all(np.abs(got - want) <= bound * (
        np.abs(b) + s * (np.abs(Binv) @ np.abs(s * kb))))
    got = _laplace.apply_torch(_t(K), _t(a)).numpy()
    assert np.all(np.abs(got - K @ a) <= bound * (np.abs(K) @ np.abs(a)))


@pytest.mark.parametrize('layout', ['column-major', 'row-major'])
@pytest.mark.parametrize('n,m,planes', [(1, 1, [0]), (33, 3, [0, 1, 2]),
                                        (70, 9, [7, 2, 5]), (12, 4, [])])
def test_gradient_restatements_against_algorithm_5_1(n, m, planes, layout):
    """`third_order` and `contract_torch` (one weight matrix M) against the
    per-plane loop ``s_1 + s_2 . s_3`` of algorithm 5.1 as scikit-learn
    writes it.  The loop chains three products of n terms each; the bound is
    ``8 n eps`` of the magnitudes it adds up."""
    from graphdot_amd.model.gaussian_process import _laplace
    eps = np.finfo(float).eps
    K, P, y, f, _ = _case(n, m, 3 * n + m)
    B, vec, _ = (t.numpy() for t in _laplace.build_torch(
        _t(K), _t(f), _t(y), _t(np.zeros(n))))
    pi, s, g = vec[:n], vec[n:2 * n], vec[3 * n:4 * n]
    Binv = np.linalg.inv(B)
    Binv = 0.5 * (Binv + Binv.T)
    a = _laplace.solve_torch(_t(Binv), _t(vec)).numpy()
    u = _laplace.third_order(_t(K), _t(Binv), _t(vec))
    Pt = _t(P.transpose(2, 1, 0)).permute(2, 1, 0) \
        if layout == 'column-major' else _t(P)
    got = _laplace.contract_torch(Pt, planes, _t(Binv), _t(s), _t(a), u,
                                  _t(g)).numpy()
    R = s[:, None] * Binv * s[None, :]
    s_2 = -0.5 * (np.diag(K) - np.einsum('ij,jk,ki->i', K, R, K)) \
        * (pi * (1 - pi) * (1 - 2 * pi))
    assert len(got) == len(planes)
    for k, j in enumerate(planes):
        C = P[:, :, j]
        s_1 = 0.5 * a @ C @ a - 0.5 * R.T.ravel() @ C.ravel()
        bb = C @ g
        s_3 = bb - K @ (R @ bb)
        size = 0.5 * np.abs(a) @ np.abs(C) @ np.abs(a) \
            + 0.5 * np.abs(R).ravel() @ np.abs(C).ravel() \
            + np.abs(s_2) @ (np.abs(C) @ np.abs(g) + np.abs(K) @ (
                np.abs(R) @ (np.abs(C) @ np.abs(g))))
        assert abs(got[k] - (s_1 + s_2 @ s_3)) <= 8 * n * eps * size
    M = _laplace.weights_torch(_t(Binv), _t(s), _t(a), u, _t(g)).numpy()
    assert np.abs(M - M.T).max() <= 4 * eps * np.abs(M).max()
