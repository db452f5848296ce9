"""KernelSVC without a GPU: the host chain (`_smo.smo_torch`, the restatement
of smo.hip) on the definitions of the dual problem -- feasibility, the
optimality gap recomputed in numpy -- and against scikit-learn's
``SVC(kernel='precomputed')`` (libsvm): the objective within the bound that
convexity gives, the labels wherever the reference's own decision values are
further from zero than the reference's own sensitivity to its tolerance; the
class weights, the one-vs-one votes, `cross_val_score` against a loop of fits
on the sub-matrices, a graph kernel on the host, the errors and the warnings.

The matrices are ``exp(-gamma |x - x'|^2)`` on 4-dimensional Gaussian features
with noisy linear labels.  Nothing here is compared with a second SMO written
in the test: the yardsticks are the definitions and scikit-learn."""
import warnings
import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
#: (gamma, C)
SETTINGS = [(0.05, 1.0), (0.5, 10.0), (0.02, 100.0)]
SIZES = [2, 3, 65, 257]
TOL = 1e-3
NEW = 50            # new points for the predictions
LEFT_OUT = 0.05     # the share of points the delta rule may leave out
DIM = 4


def _torch():
    import torch
    import graphdot_amd.model.svm  # noqa: F401 (torch first)
    return torch


_cases = {}


def data(n, gamma, k=2, seed=0):
    """(K (n, n), Ks (NEW, n), labels (n,), labels of the new points):
    computed once and left unchanged.  The first k samples carry the k
    classes, so that none is empty."""
    key = (n, gamma, k, seed)
    if key not in _cases:
        rng = np.random.default_rng(1000 * seed + 10 * n + k)
        X = rng.normal(size=(n + NEW, DIM))
        W = rng.normal(size=(DIM, k))
        lab = (X @ W + 0.5 * rng.normal(size=(n + NEW, k))).argmax(1)
        lab[:k] = np.arange(k)
        d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
        K = np.exp(-gamma * d2)
        assert np.array_equal(K, K.T)
        _cases[key] = (np.ascontiguousarray(K[:n, :n]),
                       np.ascontiguousarray(K[n:, :n]), lab[:n], lab[n:])
    return _cases[key]


def model(**kwargs):
    from graphdot_amd.model.svm import KernelSVC
    kwargs.setdefault('device', 'cpu')
    kwargs.setdefault('tol', TOL)
    return KernelSVC('precomputed', **kwargs)


def check_feasible(y, U, alpha):
    """Assertion 1 on (P, n) arrays: the box exactly, the equality
    constraint to the rounding of a sum of n terms."""
    n = y.shape[1]
    assert np.all(alpha >= 0) and np.all(alpha <= U)
    assert np.all(np.abs((y * alpha).sum(1)) <= 4 * n * EPS * alpha.sum(1))


def gap_of(K, y, U, alpha):
    """(m - M, its rounding bound) of one problem, from the definitions in
    numpy double: ``G = Q alpha - 1``, ``v = -y G``."""
    n = len(y)
    yf = y.astype(np.float64)
    G = yf * (K @ (yf * alpha)) - 1.0
    v = -yf * G
    up = np.where(yf > 0, alpha < U, alpha > 0)
    low = np.where(yf > 0, alpha > 0, alpha < U)
    if not up.any() or not low.any():
        return -np.inf, 0.0
    return v[up].max() - v[low].min(), \
        4 * n * EPS * (np.abs(K) @ np.abs(alpha)).max()


def check_optimal(K, y, U, alpha, tol):
    """Assertion 2 on (P, n) arrays."""
    for p in range(len(y)):
        gap, slack = gap_of(K, y[p], U[p], alpha[p])
        assert gap <= tol + slack, (p, gap, tol, slack)


def objective_of(K, coef):
    """``f = 1/2 c^T K c - sum |c|`` of the signed coefficients c."""
    return 0.5 * coef @ K @ coef - np.abs(coef).sum()


def sk_binary(K, lab, C, tol, class_weight=None):
    svm = pytest.importorskip('sklearn.svm')
    return svm.SVC(C=C, kernel='precomputed', tol=tol, class_weight=class_weight,
                   decision_function_shape='ovo', cache_size=50).fit(K, lab)


def sk_objective(ref, K):
    coef = np.zeros(len(K))
    coef[ref.support_] = ref.dual_coef_[0]
    return objective_of(K, coef)


def problems_of(m, lab):
    """(y, U, alpha) (P, n) of a fitted model, rebuilt from its attributes."""
    codes = np.searchsorted(m.classes_, lab)
    first = codes[None, :] == m.pairs_[:, :1]
    inside = first | (codes[None, :] == m.pairs_[:, 1:])
    y = np.where(first, 1, -1)
    w = m._weights(list(m.classes_), codes, np.ones(len(lab), dtype=bool))
    U = np.where(inside, m.C * w[codes][None, :], 0.0)
    assert np.all(m.dual_coef_[~inside] == 0)          # zero outside the pair
    assert np.all(np.sign(m.dual_coef_) * y >= 0)
    return y, U, np.abs(m.dual_coef_)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('gamma,C', SETTINGS)
def test_feasible_optimal_and_objective(gamma, C, n):
    """Assertions 1 to 3.  Any feasible alpha with gap e has ``f(alpha) - f*
    <= e sum U`` (convexity: each term of ``-grad f^T (alpha* - alpha)`` is at
    most ``(m - M) |alpha*_t - alpha_t|``), and so has scikit-learn's at the
    same tol: the two objectives differ by at most ``tol sum U``."""
    K, _, lab, _ = data(n, gamma)
    m = model(C=C).fit(K, lab)
    y, U, alpha = problems_of(m, lab)
    check_feasible(y, U, alpha)
    check_optimal(K, y, U, alpha, TOL)
    assert m.gap_[0] < TOL and m.n_iter_[0] >= 1
    f = objective_of(K, m.dual_coef_[0])
    assert abs(m.objective_[0] - f) <= 8 * n * EPS * (abs(f) + alpha.sum())
    ref = sk_binary(K, lab, C, TOL)
    f_ref = sk_objective(ref, K)
    print(f'n {n} gamma {gamma} C {C}: {m.n_iter_[0]} steps, objective '
          f'{m.objective_[0]} against {f_ref} (bound {TOL * U.sum():.3g})')
    assert abs(m.objective_[0] - f_ref) <= TOL * U.sum()
    assert np.array_equal(m.n_support_, np.bincount(
        np.searchsorted(m.classes_, lab)[m.support_], minlength=2))
    assert np.array_equal(m.support_, np.flatnonzero(alpha[0] > 0))


def test_a_tighter_tolerance():
    K, _, lab, _ = data(65, 0.5)
    m = model(C=10.0, tol=1e-8).fit(K, lab)
    y, U, alpha = problems_of(m, lab)
    check_feasible(y, U, alpha)
    check_optimal(K, y, U, alpha, 1e-8)
    f_ref = sk_objective(sk_binary(K, lab, 10.0, 1e-8), K)
    assert abs(m.objective_[0] - f_ref) <= 1e-8 * U.sum()


def delta_rule(K, Ks, lab, C, class_weight, what):
    """(scikit-learn's labels on the training set and the new points, which
    of them are sure, its decision values): delta is measured from the
    reference alone, for each pair problem 4 x the largest difference between
    its decision values at tol and at tol / 1000; a point is sure where every
    pairwise |decision| exceeds the delta of its problem.  (On these inputs
    the reference leaves out at most 4.6 % of the points, in the 5-class
    cases with their ten pairs.)"""
    Z = np.concatenate((K, Ks))
    ref = sk_binary(K, lab, C, TOL, class_weight)
    fine = sk_binary(K, lab, C, TOL / 1000, class_weight)
    D = ref.decision_function(Z)
    flat = D.reshape(len(Z), -1)
    delta = 4 * np.abs(flat - fine.decision_function(Z).reshape(flat.shape)) \
        .max(0)
    sure = (np.abs(flat) > delta).all(1)
    print(f'{what}: delta {delta.max():.3g}, {int((~sure).sum())} of '
          f'{len(sure)} points left out')
    assert (~sure).mean() <= LEFT_OUT
    return ref.predict(Z), sure, D


WEIGHTS = [None, 'balanced', 'dict']


@pytest.mark.parametrize('weights', WEIGHTS)
@pytest.mark.parametrize('k', [2, 3, 5])
@pytest.mark.parametrize('gamma,C', SETTINGS)
def test_labels_against_scikit_learn(gamma, C, k, weights):
    n = 257 if k > 2 else 65
    K, Ks, lab, _ = data(n, gamma, k)
    lab = lab * 3 - 1                          # (labels that are not 0..k-1)
    cw = {int(c): 1.0 + 0.5 * t for t, c in enumerate(np.unique(lab))} \
        if weights == 'dict' else weights
    want, sure, D = delta_rule(K, Ks, lab, C, cw, f'k {k} {weights}')
    m = model(C=C, class_weight=cw).fit(K, lab)
    Z = np.concatenate((K, Ks))
    got = m.predict(Z)
    assert got.shape == want.shape
    assert np.array_equal(got[sure], want[sure])
    F = m.decision_function(Z)
    assert F.shape == D.shape == ((n + NEW,) if k == 2
                                  else (n + NEW, k * (k - 1) // 2))
    assert np.all((np.sign(F) == np.sign(D)).reshape(len(Z), -1)[sure])
    y, U, alpha = problems_of(m, lab)
    check_feasible(y, U, alpha)
    check_optimal(K, y, U, alpha, TOL)
    assert m.pairs_.tolist() == [[a, b] for a in range(k)
                                 for b in range(a + 1, k)]
    assert abs(m.score(Z[:n], lab) - (got[:n] == lab).mean()) < 1e-15


def test_cross_val_score_equals_a_loop_of_fits():
    """Exact equality.  The problem of a fold inside the batch is the problem
    on the fold's sub-matrix with the other samples given U = 0: such a sample
    is in neither I_up nor I_low, is never chosen and keeps alpha = 0, so it
    adds exact zeros to no G that is looked at; the members keep their
    relative index order, so every argmax and argmin with its lowest-index tie
    picks the same sample, every update is the same arithmetic on the same
    numbers, the free samples are added up in the same order, and
    `decide_torch` adds its terms one after the other in index order, the
    excluded ones being exact zeros."""
    Cs = [0.5, 5.0, 50.0]
    for k, n in ((2, 65), (3, 65)):
        K, _, lab, _ = data(n, 0.05, k, seed=1)
        rng = np.random.default_rng(k)
        fold = rng.permutation(n) % 3
        # (the first k samples carry the classes: every fold trains on them)
        fold[:k] = 3
        cv = [(np.flatnonzero(fold != f), np.flatnonzero(fold == f))
              for f in range(3)]
        for cw in (None, 'balanced'):
            got = model(class_weight=cw).cross_val_score(K, lab, Cs, cv=cv)
            assert got.shape == (3, 3)
            for a, C in enumerate(Cs):
                for f, (train, test) in enumerate(cv):
                    m = model(C=C, class_weight=cw).fit(
                        K[np.ix_(train, train)], lab[train])
                    assert got[a, f] == m.score(K[np.ix_(test, train)],
                                                lab[test])
    with pytest.raises(ValueError, match='every class'):
        model().cross_val_score(K, lab, Cs, cv=[(np.arange(2), np.arange(2, n))])
    with pytest.raises(ValueError, match='trains on'):
        model().cross_val_score(K, lab, Cs, cv=[(np.arange(n), np.arange(5))])


def test_stratified_folds():
    from graphdot_amd.model.svm import KernelSVC
    K, _, lab, _ = data(257, 0.05, 3)
    codes = np.searchsorted(np.unique(lab), lab)
    folds = KernelSVC._folds(codes, 5, 0)
    assert len(folds) == 5
    assert np.array_equal(np.sort(np.concatenate([t for _, t in folds])),
                          np.arange(257))
    for train, test in folds:
        assert not set(train) & set(test) and len(train) + len(test) == 257
        # each class is dealt out in turn: its share differs by at most one
        for c in range(3):
            assert abs((codes[test] == c).sum() - (codes == c).sum() / 5) < 1
    again = KernelSVC._folds(codes, 5, 0)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(folds, again))
    acc = model().cross_val_score(K, lab, [1.0, 10.0], cv=5)
    assert acc.shape == (2, 5) and np.all((acc > 0.5) & (acc <= 1))


def test_graph_kernel_without_a_device_path():
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.model.svm import KernelSVC
    G = np.asarray(cases.config3_graphs(14, seed=3), dtype=object)
    knode, kedge, q = cases.config3_kernels()
    mgk = MarginalizedGraphKernel(knode, kedge, q=q, backend=OracleBackend())
    # (the oracle backend solves pairs only: the self-similarities of Z as
    # the diagonal of its Gram matrix)
    mgk.diag = lambda Z: mgk(Z).diagonal()
    X, Z = G[:10], G[10:]
    lab = np.array(['a', 'b', 'c'])[np.arange(10) % 3]
    for kernel in (mgk, Normalization(mgk)):
        K = np.asarray(kernel(X), dtype=np.float64)
        Ks = np.asarray(kernel(Z, X), dtype=np.float64)
        want = model(C=10.0).fit(K, lab)
        m = KernelSVC(kernel, C=10.0, tol=TOL, device='cpu').fit(X, lab)
        assert m.last_timing['adopted'] is False
        assert m.last_timing['fused'] is False
        for name in ('classes_', 'pairs_', 'dual_coef_', 'intercept_',
                     'support_', 'n_support_', 'n_iter_', 'objective_',
                     'gap_'):
            assert np.array_equal(getattr(m, name), getattr(want, name)), name
        assert np.array_equal(m.predict(Z), want.predict(Ks))
        assert np.array_equal(m.decision_function(Z),
                              want.decision_function(Ks))
        assert m.score(X, lab) == want.score(K, lab)
        assert np.array_equal(
            KernelSVC(kernel, tol=TOL, device='cpu').cross_val_score(
                X, lab, [1.0, 10.0], cv=2),
            model().cross_val_score(K, lab, [1.0, 10.0], cv=2))


def test_errors_and_warnings():
    from graphdot_amd.model.svm import KernelSVC
    K, Ks, lab, _ = data(65, 0.05)
    with pytest.raises(ValueError, match='two distinct labels'):
        model().fit(K, np.zeros(65))
    with pytest.raises(ValueError, match='square'):
        model().fit(K[:8], lab[:8])
    with pytest.raises(ValueError, match='labels expected'):
        model().fit(K, lab[:-1])
    bad = K.copy()
    bad[3, 5] = bad[5, 3] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        model().fit(bad, lab)
    bad[3, 5] = bad[5, 3] = np.inf
    with pytest.raises(ValueError, match='not finite'):
        model().fit(bad, lab)
    for name in ('predict', 'decision_function'):
        with pytest.raises(ValueError, match='before fit'):
            getattr(model(), name)(Ks)
    with pytest.raises(ValueError, match='before fit'):
        model().score(Ks, lab[:NEW])
    with pytest.warns(UserWarning, match='1 of 1 problems'):
        m = model(max_iter=3).fit(K, lab)
    assert m.n_iter_.tolist() == [3] and m.gap_[0] >= TOL
    check_feasible(*problems_of(m, lab))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = model().fit(K, lab)
    with pytest.raises(ValueError):
        m.predict(Ks[:, :-1])
    with pytest.raises(ValueError):
        m.score(Ks, lab[:3])
    for kwargs in ({'C': 0}, {'tol': 0}, {'max_iter': 0},
                   {'class_weight': 'even'}):
        with pytest.raises(ValueError, match=list(kwargs)[0]):
            KernelSVC('precomputed', **kwargs)
    with pytest.raises(ValueError, match='class_weight'):
        model(class_weight={7: 2.0}).fit(K, lab)


def test_the_solver_states_its_status():
    """`smo_torch` on the batch itself: a NaN met on the way sets the status;
    a problem whose last third has U = 0 is the problem on the sub-matrix."""
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    K, _, lab, _ = data(65, 0.05)
    y = np.where(lab == lab[0], 1, -1).astype(np.int8)
    U = np.ones((2, 65))
    U[1, 40:] = 0
    bad = K.copy()
    bad[50, :] = bad[:, 50] = np.nan
    bad[50, 50] = 1.0
    ys = torch.from_numpy(np.stack((y, y)))
    r = _smo.smo_torch(torch.from_numpy(bad), ys, torch.from_numpy(U), TOL,
                       10 ** 6)
    assert r.info.numpy()[:, 3].tolist() == [1, 1]
    r = _smo.smo_torch(torch.from_numpy(K), ys, torch.from_numpy(U), TOL,
                       10 ** 6)
    info = r.info.numpy()
    assert info[:, 3].tolist() == [0, 0]
    assert np.all(info[:, 1] - info[:, 2] < TOL)
    sub = _smo.smo_torch(torch.from_numpy(K[:40, :40]),
                         torch.from_numpy(y[None, :40].copy()),
                         torch.ones((1, 40), dtype=torch.float64), TOL, 10 ** 6)
    assert torch.equal(sub.alpha[0], r.alpha[1, :40])
    assert torch.all(r.alpha[1, 40:] == 0)
    assert _smo.NMAX >= 2048 and _smo.NMAX * 16 + 512 <= 65536


def test_precomputed_accepts_numpy_and_torch():
    torch = _torch()
    K, Ks, lab, _ = data(65, 0.05, 3)
    want = model().fit(K, lab)
    for given, cross in ((torch.from_numpy(K), torch.from_numpy(Ks)),
                         (torch.from_numpy(K).t().contiguous().t(), Ks)):
        m = model().fit(given, list(lab))
        assert np.array_equal(m.dual_coef_, want.dual_coef_)
        assert np.array_equal(m.predict(cross), want.predict(Ks))
    m = model().fit(K.astype(np.float32), lab)
    assert np.all(m.gap_ < TOL)
    check_feasible(*problems_of(m, lab))
