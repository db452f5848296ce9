"""KernelSVR and KernelOneClassSVM without a GPU: the host chain
(`_smo.smo2_torch`, the restatement of svr.hip, and `_smo.smo_torch_from` from
`_smo.one_class_start`) on the definitions of the dual problems -- feasibility,
the optimality gap recomputed in numpy from K, z and epsilon -- and against
scikit-learn's ``SVR(kernel='precomputed')`` and
``OneClassSVM(kernel='precomputed')`` (libsvm): the objective within the bound
that convexity gives, predictions and decision values within the reference's
own sensitivity to its tolerance; `cross_val_score` against a loop of fits on
the sub-matrices, a graph kernel on the host, the errors and the warnings.

The matrices are ``exp(-gamma |x - x'|^2)`` on 4-dimensional Gaussian features
and the targets a noisy linear function of them.  Nothing here is compared
with a second SMO written in the test: the yardsticks are the definitions and
scikit-learn.

Figures these tests print (host chain, float64): the objectives differ from
scikit-learn's by at most 3.0e-5 of the bound (SVR) and 5.6e-4 (one-class);
the predictions by at most 1.03 x the reference's own difference between tol
and tol / 1000 (SVR) and the decision values by at most 1.69 x (one-class),
where 4 x is allowed."""
import warnings
import numpy as np
import pytest

from test_svc import EPS, NEW, TOL, check_feasible, gap_of

#: (gamma, C, epsilon)
SETTINGS = [(0.05, 1.0, 0.1), (0.5, 10.0, 0.05), (0.02, 10.0, 0.3)]
#: (gamma, nu)
NU_SETTINGS = [(0.05, 0.2), (0.5, 0.5), (0.02, 0.05)]
SIZES = [2, 3, 65, 257]
DIM = 4


def _torch():
    import torch
    import graphdot_amd.model.svm  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


_cases = {}


def data(n, gamma, seed=0):
    """(K (n, n), Ks (NEW, n), targets (n,), targets of the new points):
    computed once and left unchanged."""
    key = (n, gamma, seed)
    if key not in _cases:
        rng = np.random.default_rng(1000 * seed + 10 * n + 7)
        X = rng.normal(size=(n + NEW, DIM))
        z = X @ rng.normal(size=DIM) + 0.3 * rng.normal(size=n + NEW)
        d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
        K = np.exp(-gamma * d2)
        assert np.array_equal(K, K.T)
        _cases[key] = (np.ascontiguousarray(K[:n, :n]),
                       np.ascontiguousarray(K[n:, :n]), z[:n].copy(),
                       z[n:].copy())
    return _cases[key]


def signs(n):
    return np.repeat(np.array([1, -1], dtype=np.int8), n)


def gap2_of(K, z, eps, U, alpha):
    """(m - M, its rounding bound) of one epsilon-SVR problem, from the
    definitions in numpy double: ``G = Q alpha + p`` with ``Q alpha = s K (a -
    a*)`` and ``p = (eps - z, eps + z)``, ``v = -s G``; `U` (n,), `alpha`
    (2n,).  The bound: a sum of 2n terms and the linear term added to it."""
    n = len(z)
    s = signs(n).astype(np.float64)
    Kc = K @ (alpha[:n] - alpha[n:])
    G = np.concatenate((Kc + (eps - z), -Kc + (eps + z)))
    v = -s * G
    U2 = np.tile(U, 2)
    up = np.where(s > 0, alpha < U2, alpha > 0)
    low = np.where(s > 0, alpha > 0, alpha < U2)
    if not up.any() or not low.any():
        return -np.inf, 0.0
    size = np.abs(K) @ (alpha[:n] + alpha[n:]) + np.abs(z) + eps
    return v[up].max() - v[low].min(), 4 * 2 * n * EPS * size.max()


def check2(K, z, eps, U, alpha, tol):
    """Assertions 1 and 2 on a batch: `z`, `U` (P, n), `eps` (P,), `alpha`
    (P, 2n)."""
    P, n = U.shape
    check_feasible(np.tile(signs(n), (P, 1)), np.tile(U, 2), alpha)
    for p in range(P):
        gap, slack = gap2_of(K, z[p], eps[p], U[p], alpha[p])
        assert gap <= tol + slack, (p, gap, tol, slack)


def objective2_of(K, z, eps, a, astar):
    c = a - astar
    return 0.5 * c @ K @ c + eps * (a + astar).sum() - z @ c


_refs = {}


def sk_svr(K, z, C, eps, tol, key=None):
    """scikit-learn's model, computed once where a `key` names the inputs."""
    svm = pytest.importorskip('sklearn.svm')
    if key is not None and (key, C, eps, tol) in _refs:
        return _refs[key, C, eps, tol]
    ref = svm.SVR(C=C, epsilon=eps, kernel='precomputed', tol=tol,
                  cache_size=50).fit(K, z)
    if key is not None:
        _refs[key, C, eps, tol] = ref
    return ref


def sk_one(K, nu, tol, key=None):
    svm = pytest.importorskip('sklearn.svm')
    if key is not None and (key, nu, tol) in _refs:
        return _refs[key, nu, tol]
    ref = svm.OneClassSVM(nu=nu, kernel='precomputed', tol=tol,
                          cache_size=50).fit(K)
    if key is not None:
        _refs[key, nu, tol] = ref
    return ref


def sk_coef(ref, n):
    c = np.zeros(n)
    c[ref.support_] = ref.dual_coef_[0]
    return c


def sk_objective2(ref, K, z, eps):
    c = sk_coef(ref, len(K))
    return objective2_of(K, z, eps, np.maximum(c, 0), np.maximum(-c, 0))


def svr(**kwargs):
    from graphdot_amd.model.svm import KernelSVR
    kwargs.setdefault('device', 'cpu')
    kwargs.setdefault('tol', TOL)
    return KernelSVR('precomputed', **kwargs)


def one_class(**kwargs):
    from graphdot_amd.model.svm import KernelOneClassSVM
    kwargs.setdefault('device', 'cpu')
    kwargs.setdefault('tol', TOL)
    return KernelOneClassSVM('precomputed', **kwargs)


def delta_svr(K, Z, z, C, eps, key=None):
    """(the reference's predictions at `Z`, the unscaled delta): the largest
    difference between its predictions at tol and at tol / 1000."""
    ref = sk_svr(K, z, C, eps, TOL, key)
    fine = sk_svr(K, z, C, eps, TOL / 1000, key)
    want = ref.predict(Z)
    return want, np.abs(want - fine.predict(Z)).max()


def delta_one(K, Z, nu, key=None):
    ref = sk_one(K, nu, TOL, key)
    fine = sk_one(K, nu, TOL / 1000, key)
    want = ref.decision_function(Z)
    return want, np.abs(want - fine.decision_function(Z)).max()


# -- epsilon-SVR ---------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('gamma,C,eps', SETTINGS)
def test_svr_feasible_optimal_and_objective(gamma, C, eps, n):
    """Assertions 1 to 3 on the solver's own 2n variables.  Any feasible
    point with gap e has ``f - f* <= e sum_t U_t`` over the variables
    (convexity, as in test_svc.py), and so has scikit-learn's at the same
    tol: the two objectives differ by at most ``tol 2 sum U``."""
    from graphdot_amd.model.svm import _smo
    K, _, z, _ = data(n, gamma)
    U = np.full((1, n), C)
    r = _smo.smo2_torch(_t(K), _t(U), _t(z[None]), _t(np.array([eps])), TOL)
    alpha, G, info = r.alpha.numpy(), r.G.numpy(), r.info.numpy()
    assert alpha.shape == G.shape == (1, 2 * n) and info[0, 3] == 0
    assert info[0, 1] - info[0, 2] < TOL
    check2(K, z[None], [eps], U, alpha, TOL)
    f = objective2_of(K, z, eps, alpha[0, :n], alpha[0, n:])
    m = svr(C=C, epsilon=eps).fit(K, z)
    assert np.array_equal(m.dual_coef_, alpha[0, :n] - alpha[0, n:])
    assert m.n_iter_ == info[0, 0] and m.gap_ == info[0, 1] - info[0, 2]
    assert abs(m.objective_ - f) <= 8 * 2 * n * EPS * (
        abs(f) + (1 + np.abs(z).max() + eps) * alpha.sum())
    assert np.array_equal(m.support_, np.flatnonzero(m.dual_coef_))
    f_ref = sk_objective2(sk_svr(K, z, C, eps, TOL, (n, gamma)), K, z, eps)
    bound = TOL * 2 * U.sum()
    print(f'n {n} gamma {gamma} C {C} eps {eps}: {m.n_iter_} steps, objective '
          f'{m.objective_} against {f_ref}: {abs(m.objective_ - f_ref) / bound:.3g}'
          ' of the bound')
    assert abs(m.objective_ - f_ref) <= bound


@pytest.mark.parametrize('n', [65, 257])
@pytest.mark.parametrize('gamma,C,eps', SETTINGS)
def test_svr_predictions_against_scikit_learn(gamma, C, eps, n):
    """Assertion 4: every training point and every new one within 4 x the
    reference's own difference between tol and tol / 1000."""
    K, Ks, z, z_new = data(n, gamma)
    Z = np.concatenate((K, Ks))
    want, delta = delta_svr(K, Z, z, C, eps, (n, gamma))
    m = svr(C=C, epsilon=eps).fit(K, z)
    got = m.predict(Z)
    assert got.shape == want.shape == (n + NEW,)
    off = np.abs(got - want).max()
    print(f'n {n} gamma {gamma} C {C} eps {eps}: off by {off:.3g}, '
          f'{off / delta:.3g} x the unscaled delta {delta:.3g}; intercept '
          f'{m.intercept_} against {sk_svr(K, z, C, eps, TOL, (n, gamma)).intercept_[0]}')
    assert delta > 0 and off <= 4 * delta
    r2 = 1 - ((z_new - got[n:]) ** 2).sum() / ((z_new - z_new.mean()) ** 2).sum()
    assert abs(m.score(Ks, z_new) - r2) <= 1e-12
    assert m.last_timing['fused'] is False and m.last_timing['adopted'] is False


def test_svr_cross_val_score_against_a_loop_of_fits():
    """Assertion 5: 3 C x 2 eps x 5 folds at n = 257 against the host model
    on the sub-matrices.  Predictions within d of one another move R^2 = 1 -
    sum (r + e)^2 / SS_tot, |e| <= d, by at most sum(2 |r| d + d^2) / SS_tot;
    d is the delta of assertion 4 for the fold's problem."""
    from graphdot_amd.model.svm import KernelSVC
    n, gamma = 257, 0.05
    K, _, z, _ = data(n, gamma)
    Cs, es = [0.3, 1.0, 3.0], [0.05, 0.3]
    m = svr()
    got = m.cross_val_score(K, z, Cs, es, cv=5, random_state=1)
    assert got.shape == (3, 2, 5) and not hasattr(m, 'dual_coef_')
    assert m.last_timing['problems'] == 30 and m.last_timing['steps'] > 30
    folds = KernelSVC._folds(np.zeros(n, dtype=np.int64), 5, 1)
    assert np.array_equal(np.sort(np.concatenate([t for _, t in folds])),
                          np.arange(n))
    worst = 0.0
    for a, C in enumerate(Cs):
        for e, eps in enumerate(es):
            for f, (train, test) in enumerate(folds):
                sub = np.ascontiguousarray(K[np.ix_(train, train)])
                cross = np.ascontiguousarray(K[np.ix_(test, train)])
                one = svr(C=C, epsilon=eps).fit(sub, z[train])
                _, d = delta_svr(sub, np.concatenate((sub, cross)), z[train],
                                 C, eps)
                d *= 4
                r = z[test] - one.predict(cross)
                total = ((z[test] - z[test].mean()) ** 2).sum()
                bound = (2 * np.abs(r) * d + d * d).sum() / total
                want = one.score(cross, z[test])
                worst = max(worst, abs(got[a, e, f] - want) / bound)
                assert abs(got[a, e, f] - want) <= bound, (C, eps, f)
    print(f'largest share of the propagated bound: {worst:.3g}')
    again = svr().cross_val_score(K, z, Cs, es, cv=folds)
    assert np.array_equal(again, got)
    with pytest.raises(ValueError, match='trains on'):
        svr().cross_val_score(K, z, Cs, es, cv=[(np.arange(n), np.arange(5))])
    with pytest.raises(ValueError, match='index arrays'):
        svr().cross_val_score(K, z, Cs, es, cv=[(np.arange(n + 1), [0])])
    with pytest.raises(ValueError, match='two folds'):
        svr().cross_val_score(K, z, Cs, es, cv=1)
    with pytest.raises(ValueError, match='Cs'):
        svr().cross_val_score(K, z, [0.0], es)
    with pytest.raises(ValueError, match='epsilons'):
        svr().cross_val_score(K, z, Cs, [-0.1])


def test_svr_batch_and_membership():
    """`smo2_torch` on a batch whose problems differ in C, epsilon, targets
    and members: each is solved as if alone, and a problem whose last third
    has U = 0 is the problem on the sub-matrix, bit for bit."""
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    n = 65
    K, _, z, _ = data(n, 0.05)
    U = np.ones((3, n)) * np.array([1.0, 10.0, 1.0])[:, None]
    U[2, 40:] = 0
    zs = np.stack((z, -2 * z, z))
    eps = np.array([0.1, 0.05, 0.1])
    r = _smo.smo2_torch(_t(K), _t(U), _t(zs), _t(eps), TOL)
    info = r.info.numpy()
    assert info[:, 3].tolist() == [0, 0, 0]
    check2(K, zs, eps, U, r.alpha.numpy(), TOL)
    for p in range(2):
        alone = _smo.smo2_torch(_t(K), _t(U[p:p + 1]), _t(zs[p:p + 1]),
                                _t(eps[p:p + 1]), TOL)
        assert torch.equal(alone.alpha[0], r.alpha[p])
        assert torch.equal(alone.info[0], r.info[p])
    sub = _smo.smo2_torch(_t(K[:40, :40]), _t(U[2:, :40]), _t(zs[2:, :40]),
                          _t(eps[2:]), TOL)
    a = r.alpha[2].reshape(2, n)
    assert torch.all(a[:, 40:] == 0)
    assert torch.equal(sub.alpha[0].reshape(2, 40), a[:, :40])
    bad = K.copy()
    bad[50, :] = bad[:, 50] = np.nan
    bad[50, 50] = 1.0
    r = _smo.smo2_torch(_t(bad), _t(U), _t(zs), _t(eps), TOL)
    assert r.info.numpy()[:, 3].tolist() == [1, 1, 1]
    assert _smo.NMAX2 == _smo.NMAX // 2 == 2032
    assert _smo.NMAX2 * 32 + 512 <= 65536


# -- one class -----------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('gamma,nu', NU_SETTINGS)
def test_one_class_feasible_optimal_and_objective(gamma, nu, n):
    """Assertions 1 to 3: ``0 <= a <= 1``, ``sum a = nu n``, the gap from
    ``G = K a`` (`gap_of` adds a constant to every G, which m - M does not
    see), the objective within ``tol n`` of scikit-learn's."""
    K, _, _, _ = data(n, gamma)
    m = one_class(nu=nu).fit(K)
    a = m.dual_coef_
    assert a.shape == (n,) and np.all(a >= 0) and np.all(a <= 1)
    assert abs(a.sum() - nu * n) <= 4 * n * EPS * nu * n
    ones = np.ones(n)
    gap, slack = gap_of(K, ones, ones, a)
    assert gap <= TOL + slack and m.gap_ < TOL
    f = 0.5 * a @ K @ a
    assert abs(m.objective_ - f) <= 8 * n * EPS * abs(f)
    assert np.array_equal(m.support_, np.flatnonzero(a))
    ref = sk_one(K, nu, TOL, (n, gamma))
    c = sk_coef(ref, n)
    f_ref = 0.5 * c @ K @ c
    print(f'n {n} gamma {gamma} nu {nu}: {m.n_iter_} steps, objective '
          f'{m.objective_} against {f_ref}: '
          f'{abs(m.objective_ - f_ref) / (TOL * n):.3g} of the bound')
    assert abs(m.objective_ - f_ref) <= TOL * n


@pytest.mark.parametrize('n', [65, 257])
@pytest.mark.parametrize('gamma,nu', NU_SETTINGS)
def test_one_class_decisions_against_scikit_learn(gamma, nu, n):
    """Assertion 4 for the decision values; the labels are checked against
    the model's own decision values only (a free support vector lies on the
    boundary in any correct solution)."""
    K, Ks, _, _ = data(n, gamma)
    Z = np.concatenate((K, Ks))
    want, delta = delta_one(K, Z, nu, (n, gamma))
    m = one_class(nu=nu).fit(K)
    got = m.decision_function(Z)
    off = np.abs(got - want).max()
    print(f'n {n} gamma {gamma} nu {nu}: off by {off:.3g}, {off / delta:.3g} '
          f'x the unscaled delta {delta:.3g}; intercept {m.intercept_} against '
          f'{sk_one(K, nu, TOL, (n, gamma)).intercept_[0]}')
    assert delta > 0 and off <= 4 * delta
    assert np.array_equal(m.predict(Z), np.where(got > 0, 1, -1))
    assert np.array_equal(m.score_samples(Z), got - m.intercept_)


def test_one_class_start():
    """libsvm's start on the members in index order, G0 = K a0."""
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    n = 65
    K, _, _, _ = data(n, 0.05)
    U = np.ones((3, n))
    U[1, ::3] = 0
    nu = np.array([0.2, 0.5, 1.0])
    state, info = _smo.one_class_start(_t(K), _t(nu), _t(U))
    a0, G0 = state[:, 0].numpy(), state[:, 1].numpy()
    assert info.numpy().tolist() == [[0, np.inf, -np.inf, 0]] * 3
    assert a0[0].tolist() == [1.0] * 13 + [0.0] * 52
    members = np.flatnonzero(U[1])
    assert len(members) == 43 and np.all(a0[1, ::3] == 0)
    assert a0[1, members].tolist() == [1.0] * 21 + [0.5] + [0.0] * 21
    assert np.all(a0[2] == 1)
    for p in range(3):
        assert abs(a0[p].sum() - nu[p] * U[p].sum()) <= 4 * n * EPS * n
    assert np.all(np.abs(G0 - a0 @ K) <= 2 * n * EPS * (a0 @ np.abs(K)))
    y = torch.ones((3, n), dtype=torch.int8)
    r = _smo.smo_torch_from(_t(K), y, _t(U), state, info, TOL)
    a = r.alpha.numpy()
    assert np.all(a[1, ::3] == 0) and np.all(a >= 0) and np.all(a <= U)
    assert np.all(np.abs(a.sum(1) - nu * U.sum(1)) <= 4 * n * EPS * n)
    for p in range(3):
        gap, slack = gap_of(K, np.ones(n), U[p], a[p])
        assert gap <= TOL + slack
    assert r.info.numpy()[2, 0] == 0                    # (nu = 1: nothing moves)
    with pytest.raises(ValueError, match='nu'):
        _smo.one_class_start(_t(K), _t(np.array([0.0, 0.5, 1.0])), _t(U))
    with pytest.raises(TypeError, match='nu'):
        _smo.one_class_start(_t(K), _t(nu[:2]), _t(U))
    with pytest.raises(TypeError, match='U'):
        _smo.one_class_start(_t(K), _t(nu), _t(U[:, :-1]))
    with pytest.raises(TypeError, match='K'):
        _smo.one_class_start(_t(K[:-1]), _t(nu), _t(U))


# -- both -----------------------------------------------------------------------------
def test_graph_kernel_without_a_device_path():
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.model.svm import KernelOneClassSVM, KernelSVR
    G = np.asarray(cases.config3_graphs(14, seed=3), dtype=object)
    knode, kedge, q = cases.config3_kernels()
    mgk = MarginalizedGraphKernel(knode, kedge, q=q, backend=OracleBackend())
    # (the oracle backend solves pairs only: the self-similarities of Z as
    # the diagonal of its Gram matrix)
    mgk.diag = lambda Z: mgk(Z).diagonal()
    X, Z = G[:10], G[10:]
    z = np.array([float(len(g.nodes)) for g in X])
    kernel = Normalization(mgk)
    K = np.asarray(kernel(X), dtype=np.float64)
    Ks = np.asarray(kernel(Z, X), dtype=np.float64)
    want = svr(C=10.0).fit(K, z)
    m = KernelSVR(kernel, C=10.0, tol=TOL, device='cpu').fit(X, z)
    assert m.last_timing['adopted'] is False
    assert m.last_timing['fused'] is False
    for name in ('dual_coef_', 'intercept_', 'support_', 'n_iter_',
                 'objective_', 'gap_'):
        assert np.array_equal(getattr(m, name), getattr(want, name)), name
    assert np.array_equal(m.predict(Z), want.predict(Ks))
    zz = np.array([float(len(g.nodes)) for g in Z])
    assert m.score(Z, zz) == want.score(Ks, zz)
    assert np.array_equal(
        KernelSVR(kernel, tol=TOL, device='cpu').cross_val_score(
            X, z, [1.0, 10.0], [0.1], cv=2),
        svr().cross_val_score(K, z, [1.0, 10.0], [0.1], cv=2))
    want = one_class(nu=0.3).fit(K)
    m = KernelOneClassSVM(kernel, nu=0.3, tol=TOL, device='cpu').fit(X)
    assert m.last_timing['adopted'] is False
    assert m.last_timing['fused'] is False
    for name in ('dual_coef_', 'intercept_', 'support_', 'n_iter_',
                 'objective_', 'gap_'):
        assert np.array_equal(getattr(m, name), getattr(want, name)), name
    assert np.array_equal(m.decision_function(Z), want.decision_function(Ks))
    assert np.array_equal(m.predict(Z), want.predict(Ks))


def test_errors_and_warnings():
    from graphdot_amd.model.svm import KernelOneClassSVM, KernelSVR
    K, Ks, z, _ = data(65, 0.05)
    with pytest.raises(ValueError, match='square'):
        svr().fit(K[:8], z[:8])
    with pytest.raises(ValueError, match='targets expected'):
        svr().fit(K, z[:-1])
    for value in (np.nan, np.inf):
        bad = z.copy()
        bad[3] = value
        with pytest.raises(ValueError, match='finite targets'):
            svr().fit(K, bad)
        bad = K.copy()
        bad[3, 5] = bad[5, 3] = value
        with pytest.raises(ValueError, match='not finite'):
            svr().fit(bad, z)
        with pytest.raises(ValueError, match='not finite'):
            one_class().fit(bad)
        with pytest.raises(ValueError, match='not finite'):
            svr().cross_val_score(bad, z, [1.0], [0.1])
    for make in (svr, one_class):
        for name in ('predict', 'decision_function', 'score_samples'):
            if hasattr(make(), name):
                with pytest.raises(ValueError, match='before fit'):
                    getattr(make(), name)(Ks)
    with pytest.raises(ValueError, match='before fit'):
        svr().score(Ks, z[:NEW])
    with pytest.warns(UserWarning, match='KernelSVR: 1 of 1 problems'):
        m = svr(max_iter=3).fit(K, z)
    assert m.n_iter_ == 3 and m.gap_ >= TOL
    with pytest.warns(UserWarning, match='KernelOneClassSVM: 1 of 1 problems'):
        m = one_class(max_iter=3).fit(K)
    assert m.n_iter_ == 3 and m.gap_ >= TOL
    with pytest.warns(UserWarning, match='2 of 2 problems'):
        svr(max_iter=3).cross_val_score(K, z, [1.0], [0.1], cv=2)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = svr().fit(K, z)
        o = one_class().fit(K)
    for fitted in (m, o):
        with pytest.raises(ValueError):
            fitted.predict(Ks[:, :-1])
    with pytest.raises(ValueError):
        m.score(Ks, z[:3])
    for kwargs in ({'C': 0}, {'epsilon': -1e-9}, {'tol': 0}, {'max_iter': 0}):
        with pytest.raises(ValueError, match=list(kwargs)[0]):
            KernelSVR('precomputed', **kwargs)
    for kwargs in ({'nu': 0}, {'nu': 1.5}, {'tol': 0}, {'max_iter': 0}):
        with pytest.raises(ValueError, match=list(kwargs)[0]):
            KernelOneClassSVM('precomputed', **kwargs)
    assert svr(epsilon=0.0).fit(K, z).gap_ < TOL


def test_the_host_launches_check_their_arguments():
    from graphdot_amd.model.svm import _smo
    K, _, z, _ = data(65, 0.05)
    U, zs, eps = np.ones((1, 65)), z[None], np.array([0.1])
    with pytest.raises(TypeError, match='U'):
        _smo.smo2_torch(_t(K), _t(U[:, :-1]), _t(zs), _t(eps))
    with pytest.raises(TypeError, match='U'):
        _smo.smo2_torch(_t(K), _t(U.astype(np.float32)), _t(zs), _t(eps))
    with pytest.raises(TypeError, match='z'):
        _smo.smo2_torch(_t(K), _t(U), _t(zs[:, :-1]), _t(eps))
    with pytest.raises(TypeError, match='eps'):
        _smo.smo2_torch(_t(K), _t(U), _t(zs), _t(np.array([0.1, 0.2])))
    with pytest.raises(ValueError, match='eps'):
        _smo.smo2_torch(_t(K), _t(U), _t(zs), _t(np.array([-0.1])))
    with pytest.raises(ValueError, match='tol'):
        _smo.smo2_torch(_t(K), _t(U), _t(zs), _t(eps), tol=0.0)
    with pytest.raises(ValueError, match='max_iter'):
        _smo.smo2_torch(_t(K), _t(U), _t(zs), _t(eps), max_iter=0)
    state, info = _smo.start2(_t(zs), _t(eps), 'cpu')
    assert state.shape == (1, 2, 130) and info.tolist() == [
        [0, np.inf, -np.inf, 0]]
    assert np.array_equal(state[0, 1].numpy(),
                          np.concatenate((0.1 - z, 0.1 + z)))
    assert np.all(state[0, 0].numpy() == 0)


def test_precomputed_accepts_numpy_and_torch():
    torch = _torch()
    K, Ks, z, _ = data(65, 0.05)
    want = svr().fit(K, z)
    for given, cross in ((torch.from_numpy(K), torch.from_numpy(Ks)),
                         (torch.from_numpy(K).t().contiguous().t(), Ks)):
        m = svr().fit(given, list(z))
        assert np.array_equal(m.dual_coef_, want.dual_coef_)
        assert np.array_equal(m.predict(cross), want.predict(Ks))
    m = svr().fit(K.astype(np.float32), z)
    assert m.gap_ < TOL
    o = one_class(nu=0.2).fit(K.astype(np.float32))
    assert o.gap_ < TOL and abs(o.dual_coef_.sum() - 13) <= 1e-12
