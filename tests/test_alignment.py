"""KernelTargetAlignment without a GPU: the host chain
(`_align.alignment_torch`, the restatement of alignment.hip) against the
definition of the centred alignment in numpy double with an explicit centring
matrix ``H = I - 11^T / n``; the invariances of the alignment; the gradient of
a graph kernel's alignment against central differences; `fit` with an
optimizer; the errors, the task rule and `score`.

The matrices are the RBF matrices ``v exp(-gamma |x - x'|^2)`` of test_svc.py
at v = 1 with their analytic planes w.r.t. v and gamma, and further planes
made as symmetric random matrices.  Nothing here is compared with a second
copy of the code under test.

The rounding bound of each of the sums a, b, g_p, h_p is ``4 n^2 eps sum_ij
|x_ij| z_ij`` with x the factor read from memory (K_c or dK_p) and z the
magnitude of the other one: ``|w_ij|``, or, where that is K_c, ``|K_ij| +
(|r_i| + |r_j|) / n + |s| / n^2``: a fixed-order double sum of n^2 terms whose
factors are themselves sums of n and n^2 terms."""
import numpy as np
import pytest

import test_svc as svc

EPS = svc.EPS
GAMMA = 0.05
SIZES = [2, 3, 65, 257]
PLANES = [0, 1, 3, 17]
COLUMNS = [1, 2, 16, 17]


def _torch():
    import torch
    import graphdot_amd.model.alignment  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


# -- the data and the definition -----------------------------------------------------
_inputs, _definitions = {}, {}


def inputs(n, m, k):
    """(K (n, n), P (n, n, m), T (n, k)) in double: computed once and left
    unchanged.  Planes 0 and 1 are dK / dv = exp(-gamma d^2) and dK / dgamma
    = -d^2 K at v = 1, the others symmetric random matrices; two target
    columns are the one-hot labels of test_svc.data, any other number normal
    regression targets."""
    key = (n, m, k)
    if key not in _inputs:
        K, _, lab, _ = svc.data(n, GAMMA)
        rng = np.random.default_rng(7 * n + 3 * m + k)
        P = np.empty((n, n, m))
        for p in range(m):
            if p == 0:
                P[:, :, p] = K
            elif p == 1:
                P[:, :, p] = K * np.log(K) / GAMMA        # -d^2 K
            else:
                R = rng.normal(size=(n, n))
                P[:, :, p] = R + R.T
        if k == 2:
            T = np.stack((lab == 0, lab == 1), axis=1).astype(np.float64)
        else:
            T = rng.normal(size=(n, k))
        _inputs[key] = (K, P, T)
    return _inputs[key]


def stored(n, m, k, dtype):
    """`inputs` rounded to `dtype` and widened to double again: what the
    code under test reads."""
    K, P, T = inputs(n, m, k)
    return (K.astype(dtype).astype(np.float64),
            P.astype(dtype).astype(np.float64), T)


def define(K, P, T):
    """(sums [a, b, g, h], their rounding bounds, A, dA) from the definition
    in numpy double with an explicit H; K, P, T in double."""
    n, m = len(K), P.shape[2]
    H = np.eye(n) - np.ones((n, n)) / n
    Tc = H @ T
    Lc = Tc @ Tc.T
    Kc = H @ K @ H
    r = np.abs(K.sum(1))
    zk = np.abs(K) + (r[:, None] + r[None, :]) / n + abs(K.sum()) / n ** 2
    zw = np.abs(Lc)
    sums, bound = np.empty(2 + 2 * m), np.empty(2 + 2 * m)
    sums[0], bound[0] = (Kc * Lc).sum(), (np.abs(Kc) * zw).sum()
    sums[1], bound[1] = (Kc * Kc).sum(), (np.abs(Kc) * zk).sum()
    for p in range(m):
        D = P[:, :, p]
        Dc = H @ D @ H
        sums[2 + p], bound[2 + p] = (Dc * Lc).sum(), (np.abs(D) * zw).sum()
        sums[2 + m + p] = (Dc * Kc).sum()
        bound[2 + m + p] = (np.abs(D) * zk).sum()
    Kn, Ln = np.linalg.norm(Kc), np.linalg.norm(Lc)
    A = sums[0] / (Kn * Ln)
    dA = sums[2:2 + m] / (Kn * Ln) - A * sums[2 + m:] / Kn ** 2
    return sums, 4 * n ** 2 * EPS * bound, A, dA


def definition(n, m, k, dtype=np.float64):
    """`define` of `stored`: computed once and left unchanged."""
    key = (n, m, k, np.dtype(dtype).name)
    if key not in _definitions:
        _definitions[key] = define(*stored(n, m, k, dtype))
    return _definitions[key]


def centred(T):
    return np.ascontiguousarray(T - T.mean(0))


def matrix(K, dtype, layout):
    """K stored as `dtype`, contiguous along the index `layout` names."""
    A = _t(K.astype(dtype))
    return A.t().contiguous().t() if layout == 'column-major' else A


def planes_along(P, dtype, axis):
    """The (n, n, m) planes stored as `dtype`, contiguous along `axis`."""
    A = _t(P.astype(dtype))
    order = [d for d in range(3) if d != axis] + [axis]
    back = [order.index(d) for d in range(3)]
    return A.permute(*order).contiguous().permute(*back)


def worst(got, want, bound):
    """The largest share of its bound any sum is off by (0 / 0 = 0)."""
    err = np.abs(np.asarray(got) - want)
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300),
                                 0.0), initial=0.0))


# -- the restatement against the definition ------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_restatement_against_the_definition(n):
    from graphdot_amd.model.alignment import _align
    share = 0.0
    for m in PLANES:
        for k in COLUMNS:
            K, P, T = inputs(n, m, k)
            want, bound, A, dA = definition(n, m, k)
            Tc = _t(centred(T))
            for layout in ('row-major', 'column-major'):
                got = _align.alignment_torch(
                    matrix(K, np.float64, layout), Tc,
                    planes_along(P, np.float64, 2 * (layout == 'row-major')),
                    np.arange(m)).numpy()
                assert got.shape == (2 + 2 * m,)
                share = max(share, worst(got, want, bound))
                assert np.all(np.abs(got - want) <= bound), (m, k, layout)
                val, grad = _align.value_and_gradient(
                    got[0], got[1], got[2:2 + m], got[2 + m:],
                    np.linalg.norm(centred(T).T @ centred(T)))
                assert -1 <= val <= 1
                # (the quotients of sums within their bounds)
                assert val == pytest.approx(A, rel=1e-9, abs=1e-12)
                assert np.allclose(grad, dA, rtol=1e-7,
                                   atol=1e-9 * (1 + np.abs(dA).max(initial=0)))
    print(f'n {n}: the sums are off by at most {share:.3g} of their bounds')


def test_restatement_selects_and_reorders_planes():
    from graphdot_amd.model.alignment import _align
    n, m, k = 65, 17, 2
    K, P, T = inputs(n, m, k)
    want, bound, _, _ = definition(n, m, k)
    pick = np.array([16, 0, 5, 1])
    got = _align.alignment_torch(_t(K), _t(centred(T)), _t(P), pick).numpy()
    idx = np.concatenate(([0, 1], 2 + pick, 2 + m + pick))
    assert np.all(np.abs(got - want[idx]) <= bound[idx])


# -- invariances -------------------------------------------------------------------
def _model(**kwargs):
    from graphdot_amd.model.alignment import KernelTargetAlignment
    kwargs.setdefault('device', 'cpu')
    return KernelTargetAlignment('precomputed', **kwargs)


@pytest.mark.parametrize('n', [3, 65, 257])
def test_invariances(n):
    K, _, lab, _ = svc.data(n, GAMMA, k=3)
    z = np.random.default_rng(n).normal(size=n)
    m = _model()
    A = m.fit(K, lab).alignment_
    assert m.task_ == 'classification' and -1 <= A <= 1
    assert m.last_timing['fused'] is False
    assert m.last_timing['adopted'] is False
    assert A == pytest.approx(define(K, np.empty((n, n, 0)),
                                     np.eye(3)[lab])[2], rel=1e-12)
    # A(c K + d 11^T) = A(K) for c > 0
    for c, d in ((3.0, 0.0), (1.0, -0.7), (0.25, 5.0)):
        assert m.alignment(X=c * K + d, y=lab) == pytest.approx(A, rel=1e-10)
    # the names of the classes do not matter
    names = np.array(['b', 'c', 'a'])[lab].tolist()
    assert _model().fit(K, names).alignment_ == pytest.approx(A, rel=1e-12)
    swapped = _model().fit(K, [(2 - v, 'x') for v in lab.tolist()])
    assert swapped.alignment_ == pytest.approx(A, rel=1e-12)
    # A(L_c) = 1, for labels and for regression targets
    onehot = np.eye(3)[lab]
    Tc = centred(onehot)
    assert _model().fit(Tc @ Tc.T, lab).alignment_ == pytest.approx(
        1.0, abs=1e-12)
    zc = z - z.mean()
    r = _model().fit(np.outer(zc, zc), z)
    assert r.task_ == 'regression'
    assert r.alignment_ == pytest.approx(1.0, abs=1e-12)
    assert _model().fit(-np.outer(zc, zc), z).alignment_ == pytest.approx(
        -1.0, abs=1e-12)
    # +-1 regression targets are the two-class one-hot targets
    two = svc.data(n, GAMMA, k=2)[2]
    assert _model().fit(K, two).alignment_ == pytest.approx(
        _model().fit(K, np.where(two == 0, 1.0, -1.0)).alignment_, rel=1e-12)


# -- a graph kernel on the host --------------------------------------------------------
_graph_case = {}


def graph_case():
    """(kernel, 10 graphs, labels, regression targets), built once."""
    if not _graph_case:
        import cases
        from oracle_backend import OracleBackend
        from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
        from graphdot_amd.kernel.fix import Normalization
        G = np.asarray(cases.config3_graphs(10, seed=3), dtype=object)
        knode, kedge, q = cases.config3_fit_kernels()
        mgk = MarginalizedGraphKernel(knode, kedge, q=q, q_bounds=(1e-3, 0.5),
                                      backend=OracleBackend(tol=1e-13))
        size = np.array([float(len(g.nodes)) for g in G])
        _graph_case['case'] = (Normalization(mgk), G,
                               (size > np.median(size)).astype(int), size)
    return _graph_case['case']


@pytest.mark.parametrize('task', ['classification', 'regression'])
def test_gradient_against_central_differences(task):
    """Central differences of step h = 1e-3 in log-theta, as
    test_gpc.py takes them of its likelihood: truncation ``h^2 |A'''| / 6``
    with third derivatives of the order of the gradient itself, and the noise
    of the value solves (1e-13) over h far below that, within ``1e-6 (1 +
    max |gradient|)``."""
    from graphdot_amd.model.alignment import KernelTargetAlignment
    h = 1e-3
    kernel, G, lab, size = graph_case()
    y = lab if task == 'classification' else size
    kta = KernelTargetAlignment(kernel, device='cpu')
    theta = np.array(kernel.theta)
    value, grad = kta.alignment(theta, X=G, y=y, eval_gradient=True)
    assert len(grad) == len(theta) >= 5
    assert value == pytest.approx(kta.alignment(theta, X=G, y=y), rel=1e-9)
    numeric = np.empty_like(grad)
    for k in range(len(theta)):
        e = np.zeros_like(theta)
        e[k] = h
        numeric[k] = (kta.alignment(theta + e, X=G, y=y)
                      - kta.alignment(theta - e, X=G, y=y)) / (2 * h)
    err = np.abs(numeric - grad).max()
    print(f'{task}: central differences {err:.3g}, gradient '
          f'{np.abs(grad).max():.3g}')
    assert np.array_equal(kernel.theta, theta)
    assert err <= 1e-6 * (1 + np.abs(grad).max())


def test_fit_with_an_optimizer():
    from graphdot_amd.model.alignment import KernelTargetAlignment
    kernel, G, lab, _ = graph_case()
    theta0 = np.array(kernel.theta)
    plain = KernelTargetAlignment(kernel, device='cpu').fit(G, lab)
    assert np.array_equal(plain.theta_, theta0)
    assert plain.alignment_ == plain.alignment(theta0)
    kta = KernelTargetAlignment(kernel, optimizer=True, device='cpu')
    assert kta.optimizer == 'L-BFGS-B'
    kta.fit(G, lab, tol=1e-3)
    print(f'alignment {plain.alignment_:.6g} -> {kta.alignment_:.6g} in '
          f'{kta.optimization_result.nfev} evaluations')
    assert kta.alignment_ >= plain.alignment_
    lo, hi = np.asarray(kernel.bounds).T
    assert np.all(kta.theta_ >= lo) and np.all(kta.theta_ <= hi)
    assert np.array_equal(kernel.theta, theta0)           # never modified
    # (theta goes through exp and log on its way into the clone)
    assert np.allclose(kta.kernel_.theta, kta.theta_, rtol=0, atol=8 * EPS
                       * (1 + np.abs(kta.theta_).max()))
    again = KernelTargetAlignment(kta.kernel_, device='cpu').fit(G, lab)
    assert again.alignment_ == pytest.approx(kta.alignment_, rel=1e-12)
    assert kta.last_timing['fused'] is False
    assert kta.last_timing['adopted'] is False
    assert sorted(kta.classes_) == [0, 1]
    # score: the alignment of kernel_ on other graphs
    assert kta.score(G[:6], lab[:6]) == pytest.approx(
        KernelTargetAlignment(kta.kernel_, device='cpu').alignment(
            X=G[:6], y=lab[:6]), rel=1e-12)
    # a restart draws one further start and cannot do worse
    np.random.seed(0)
    more = KernelTargetAlignment(kernel, optimizer=True,
                                 n_restarts_optimizer=1, device='cpu')
    assert more.fit(G, lab, tol=1e-3).alignment_ >= kta.alignment_ - 1e-12
    assert np.array_equal(kernel.theta, theta0)


# -- errors, the task rule, score -----------------------------------------------------
def test_errors():
    from graphdot_amd.model.alignment import KernelTargetAlignment, _align
    n = 6
    K, _, lab, _ = svc.data(65, GAMMA)
    K, lab = K[:n, :n], lab[:n]
    with pytest.raises(ValueError, match='precomputed'):
        KernelTargetAlignment('precomputed', optimizer=True)
    with pytest.raises(ValueError, match='precomputed'):
        _model().alignment(X=K, y=lab, eval_gradient=True)
    with pytest.raises(ValueError, match='task'):
        _model(task='ranking')
    with pytest.raises(ValueError, match='two samples'):
        _model().fit(K[:1, :1], np.array([1.0]))
    with pytest.raises(ValueError, match='two distinct'):
        _model().fit(K, [1] * n)
    with pytest.raises(ValueError, match=r'\|\|L_c\|\| = 0'):
        _model().fit(K, np.ones(n))
    with pytest.raises(ValueError, match=r'\|\|K_c\|\| = 0'):
        _model().fit(np.ones((n, n)), lab)
    for bad in (np.nan, np.inf):
        Kb = K.copy()
        Kb[2, 3] = Kb[3, 2] = bad
        with pytest.raises(ValueError, match='not finite'):
            _model().fit(Kb, lab)
        with pytest.raises(ValueError, match='not finite'):
            _model().fit(K, np.where(np.arange(n) == 1, bad, 1.0))
    with pytest.raises(ValueError, match='square'):
        _model().fit(K[:, :4], lab)
    with pytest.raises(ValueError, match='targets expected'):
        _model().fit(K, lab[:4])
    with pytest.raises(ValueError, match='fit first'):
        _model().alignment()
    with pytest.raises(ValueError, match='before fit'):
        _model().score(K, lab)
    # the launches' host side checks its arguments on any device
    Kt, Tc = _t(K), _t(centred(np.eye(2)[lab]))
    P = _t(np.zeros((n, n, 2)))
    with pytest.raises(TypeError, match='CUDA'):
        _align.alignment(Kt, Tc)
    with pytest.raises(TypeError, match='K'):
        _align.alignment_torch(Kt[:, :4], Tc)
    with pytest.raises(TypeError, match='K'):
        _align.alignment_torch(Kt.to(_torch().float16), Tc)
    with pytest.raises(TypeError, match='Tc'):
        _align.alignment_torch(Kt, Tc.float())
    with pytest.raises(TypeError, match='Tc'):
        _align.alignment_torch(Kt, Tc[:4])
    with pytest.raises(TypeError, match='P'):
        _align.alignment_torch(Kt, Tc, None, [0])
    with pytest.raises(TypeError, match='P'):
        _align.alignment_torch(Kt, Tc, P[:4], [0])
    with pytest.raises(ValueError, match='out of range'):
        _align.alignment_torch(Kt, Tc, P, [2])
    with pytest.raises(ValueError, match='out of range'):
        _align.alignment_torch(Kt, Tc, P, [-1])
    with pytest.raises(ValueError, match=r'\|\|K_c\|\| = 0'):
        _align.value_and_gradient(0.0, 0.0, [], [], 1.0)
    with pytest.raises(ValueError, match='not finite'):
        _align.value_and_gradient(0.0, 1.0, [np.nan], [0.0], 1.0)


def test_the_task_rule_and_score():
    n = 65
    K, Ks, lab, _ = svc.data(n, GAMMA)
    z = np.where(lab == 0, 1.0, -1.0)
    assert _model().fit(K, lab).task_ == 'classification'        # int array
    assert _model().fit(K, lab.tolist()).task_ == 'classification'
    assert _model().fit(K, z.tolist()).task_ == 'classification'  # a list
    assert _model().fit(K, z).task_ == 'regression'            # float array
    assert _model().fit(K, z.astype(np.float32)).task_ == 'regression'
    two = _model().fit(K, np.stack((z, z * z + lab), axis=1))
    assert two.task_ == 'regression' and not hasattr(two, 'classes_')
    assert _model(task='regression').fit(K, lab).task_ == 'regression'
    as_labels = _model(task='classification').fit(K, z)
    assert as_labels.task_ == 'classification'
    assert sorted(as_labels.classes_) == [-1.0, 1.0]
    mixed = _model().fit(K, [('a', 1) if v else None for v in lab])
    assert mixed.alignment_ == pytest.approx(as_labels.alignment_, rel=1e-12)
    # three float values as labels and as targets are different questions
    three = np.array([0.0, 1.0, 5.0])[svc.data(n, GAMMA, k=3)[2]]
    assert _model(task='classification').fit(K, three).alignment_ != \
        _model().fit(K, three).alignment_
    # score: the alignment of the same (precomputed) kernel elsewhere
    m = _model().fit(K, lab)
    sub = np.ascontiguousarray(K[:40, :40])
    assert m.score(sub, lab[:40]) == _model().fit(sub, lab[:40]).alignment_
    assert m.alignment() == m.alignment_
    # float32 and tensors are worked on as they are
    A32 = _model().fit(_t(K.astype(np.float32)), lab).alignment_
    assert A32 == pytest.approx(m.alignment_, rel=1e-5)
