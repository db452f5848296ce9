"""KernelTSNE without a GPU: the host chain (`_tsne.*_torch`, the restatement of
model/manifold/tsne.h) against the definition of exact t-SNE written out below
in numpy, the definition against scikit-learn's own pieces, the model's
interface, a quality band against scikit-learn, and the kernels' file unit.

The data.  `points(n, seed)`: n points in six dimensions around four centres,
of which every seventh is an exact copy of its neighbour, so that ``d2 == 0``
off the diagonal; ``K = 1.5 exp(-0.05 |a_i - a_j|^2)``.  Shapes (n, perplexity)
below a wave (7), at a strip plus one (33), a tile plus one (65) and two tiles
plus two (130), and 257.

Rounding bounds.  ``EPS = np.finfo(float).eps``.  A component of the gradient
is a sum of n terms ``4 (a p_ij - q_ij) w_ij (y_i - y_j)``: n roundings allow
any order of the sum, 16 the dozen operations of a term with exp and log at 1
ulp, and two computed values differ by at most ``C_MEAN (n + 16) EPS sum_j
|term_ij|``, ``C_MEAN = 4`` as in test_neighbors.py.  The KL likewise over its
n (n - 1) terms.  A step multiplies the gradient's bound by ``learning_rate
gains`` and adds two roundings of its own."""
import json
import os
import warnings
import numpy as np
import pytest

from graphdot_amd.hip.source_module import FILE_UNITS

EPS = np.finfo(float).eps
C_MEAN = 4
SHAPES = [(7, 2.0), (33, 5.0), (65, 5.0), (130, 10.0), (257, 30.0)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _torch():
    import torch
    import graphdot_amd.model.manifold  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.array(a, order='C'))


# -- the data --------------------------------------------------------------------------
def points(n, seed):
    r = np.random.RandomState(seed)
    c = 2 * r.randn(4, 6)
    A = c[r.randint(0, 4, n)] + 0.5 * r.randn(n, 6)
    A[2::7] = A[1::7][:len(A[2::7])]
    return A


def kernel_matrix(A, dtype=np.float64):
    sq = np.zeros((len(A), len(A)))
    for c in range(A.shape[1]):             # (nothing of size n x n x 6)
        sq += (A[:, None, c] - A[None, :, c]) ** 2
    return (1.5 * np.exp(-0.05 * sq)).astype(dtype)


def duplicates(n):
    """(i, j) pairs of `points(n, .)` that are copies of each other."""
    j = np.arange(2, n, 7)
    return j - 1, j


# -- the definition --------------------------------------------------------------------
def define_d2(K):
    """d2 of the stored matrix widened to double, zero on the diagonal."""
    K = np.asarray(K, dtype=np.float64)
    d = K.diagonal()
    d2 = np.maximum(0.0, (d[:, None] + d[None, :]) - 2.0 * K)
    np.fill_diagonal(d2, 0.0)
    return d2


def define_entropy(row, beta):
    """(H, m, Z) of one row's d2 to the others."""
    m = row.min()
    r = row - m
    e = np.exp(-beta * r)
    Z = e.sum()
    return np.log(Z) + beta * (r * e).sum() / Z, m, Z


def define_calibrate(d2, perplexity):
    """(beta, m, 1 / Z, steps): scikit-learn's bisection in double with the
    shift; `steps` counts the evaluations that missed the tolerance."""
    n = len(d2)
    out = np.empty((4, n))
    target = np.log(perplexity)
    for i in range(n):
        row = np.delete(d2[i], i)
        beta, lo, hi, steps = 1.0, -np.inf, np.inf, 0
        while True:
            H, m, Z = define_entropy(row, beta)
            if abs(H - target) <= 1e-5:
                break
            steps += 1
            if steps == 100:
                break
            if H > target:
                lo = beta
                beta = beta * 2 if hi == np.inf else (beta + hi) / 2
            else:
                hi = beta
                beta = beta / 2 if lo == -np.inf else (beta + lo) / 2
        out[:, i] = beta, m, 1.0 / Z, steps
    return out[0], out[1], out[2], out[3].astype(np.int32)


def define_tables(d2, beta):
    """(beta, m, 1 / Z) of given beta."""
    rows = [define_entropy(np.delete(d2[i], i), b) for i, b in enumerate(beta)]
    return (np.asarray(beta), np.array([r[1] for r in rows]),
            1.0 / np.array([r[2] for r in rows]))


def define_P(d2, beta, m, rZ):
    """The joint probabilities, zero on the diagonal."""
    n = len(d2)
    r = d2 - m[:, None]
    np.fill_diagonal(r, 0.0)
    E = np.exp(-beta[:, None] * r) * rZ[:, None]
    np.fill_diagonal(E, 0.0)
    P = np.maximum((E + E.T) / (2.0 * n), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def bound(n):
    return C_MEAN * (n + 16) * EPS


def define_objective(P, Y, a):
    """(KL, grad, bound of KL, bound of grad) at exaggeration a."""
    n = len(Y)
    off = ~np.eye(n, dtype=bool)
    dY = Y[:, None, :] - Y[None, :, :]
    W = np.where(off, 1.0 / (1.0 + (dY ** 2).sum(2)), 0.0)
    Zq = W.sum()
    Q = np.maximum(W / Zq, EPS)
    aP = a * P
    T = np.where(off, aP * np.log(np.maximum(aP, EPS) / Q), 0.0)
    terms = 4.0 * (np.where(off, (aP - Q) * W, 0.0))[:, :, None] * dY
    return (T.sum(), terms.sum(1), bound(n) * np.abs(T).sum(),
            bound(n) * np.abs(terms).sum(1))


def define_step(Y, update, gains, grad, momentum, learning_rate):
    inc = update * grad < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    update = momentum * update - learning_rate * (gains * grad)
    return Y + update, update, gains


# -- shared cases ----------------------------------------------------------------------
_cases = {}


def case(n, perplexity, dtype=np.float64):
    """(K as stored, d2, (beta, m, rZ, steps) of the definition, P): computed
    once and shared, read-only."""
    key = (n, perplexity, np.dtype(dtype).name)
    if key not in _cases:
        K = kernel_matrix(points(n, n), dtype)
        d2 = define_d2(K)
        cal = define_calibrate(d2, perplexity)
        P = define_P(d2, *cal[:3])
        for a in (K, d2, P) + cal:
            a.setflags(write=False)
        _cases[key] = (K, d2, cal, P)
    return _cases[key]


def embedding(n, d, scale, seed=11, equal=True):
    """A (n, d) embedding at `scale` of which two points are equal."""
    Y = scale * np.random.RandomState(seed).standard_normal((n, d))
    if equal:
        Y[n - 1] = Y[0]
    return Y


def tables(cal, device='cpu'):
    return tuple(_t(np.asarray(c, dtype=np.float64)).to(device)
                 for c in cal[:3])


def check_calibration(got, d2, perplexity):
    """The output of a calibration against the definition of the entropy."""
    beta, m, rZ, steps = (np.asarray(g) for g in got)
    n = len(d2)
    assert np.isfinite(beta).all() and (beta > 0).all()
    worst = 0.0
    for i in range(n):
        H, mi, Z = define_entropy(np.delete(d2[i], i), beta[i])
        assert m[i] == mi
        assert abs(rZ[i] * Z - 1.0) <= bound(n)
        if steps[i] < 100:
            worst = max(worst, abs(H - np.log(perplexity)))
            assert abs(H - np.log(perplexity)) <= 1e-5 + 64 * n * EPS, i
    for i, j in zip(*duplicates(n)):
        assert (beta[i], m[i], rZ[i], steps[i]) == \
            (beta[j], m[j], rZ[j], steps[j]), (i, j)
    return worst


def check_objective(got_kl, got_grad, P, Y, a):
    """A computed (KL, grad) against the definition; the largest ratios of
    the differences to their bounds."""
    kl, grad, bkl, bgrad = define_objective(P, Y, a)
    dk = abs(float(got_kl) - kl)
    dg = np.abs(np.asarray(got_grad) - grad)
    ratio = max(dk / bkl, float(np.max(dg / np.maximum(bgrad, 1e-300))))
    assert dk <= bkl, (dk, bkl)
    assert np.all(dg <= bgrad), float(np.max(dg / np.maximum(bgrad, 1e-300)))
    return ratio


# -- 1. the calibration ----------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n, perplexity', SHAPES)
def test_calibration_against_the_definition(n, perplexity, dtype):
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    K = kernel_matrix(points(n, n), dtype)
    d2 = define_d2(K)
    for Kt in (_t(K), _t(K).t().contiguous().t()):
        diag = Kt.diagonal().to(torch.float64)
        beta, m, rZ, steps, flag = _tsne.calibrate_torch(Kt, diag, perplexity)
        assert int(flag) == 0 and steps.dtype == torch.int32
        worst = check_calibration((beta, m, rZ, steps), d2, perplexity)
    print(f'n = {n}: entropy within {worst:.2e} of log(perplexity)')


@pytest.mark.parametrize('n, perplexity', [s for s in SHAPES if s[0] != 65])
def test_joint_probabilities_against_scikit_learn(n, perplexity):
    """The dense P of the calibration against scikit-learn's, which searches
    in float32 without the shift: within 1e-6 max(P) (measured: at most 6.8e-8
    max(P) on these shapes)."""
    pytest.importorskip('sklearn.manifold')
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _joint_probabilities
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    K, d2, cal, P = case(n, perplexity)
    want = squareform(_joint_probabilities(d2.astype(np.float32), perplexity,
                                           0))
    Kt = _t(K)
    beta, m, rZ, steps, _ = _tsne.calibrate_torch(
        Kt, Kt.diagonal().to(torch.float64), perplexity)
    for got in (P, define_P(d2, beta.numpy(), m.numpy(), rZ.numpy())):
        worst = np.abs(got - want).max() / want.max()
        assert worst <= 1e-6
    print(f'n = {n}: P within {worst:.2e} max(P) of scikit-learn')


# -- 2. equal off-diagonal entries -----------------------------------------------------
def test_equal_entries_cannot_be_calibrated():
    torch = _torch()
    from graphdot_amd.model.manifold import KernelTSNE, _tsne
    n = 33
    K = np.full((n, n), 0.3) + 0.7 * np.eye(n)
    Kt = _t(K)
    diag = Kt.diagonal().to(torch.float64)
    beta, m, rZ, steps, flag = _tsne.calibrate_torch(Kt, diag, 5.0)
    assert int(flag) == 0
    assert (steps == 100).all() and torch.isfinite(beta).all()
    P = define_P(define_d2(K), beta.numpy(), m.numpy(), rZ.numpy())
    off = ~np.eye(n, dtype=bool)
    assert np.abs(P[off] * (n * (n - 1)) - 1.0).max() <= bound(n)
    model = KernelTSNE('precomputed', perplexity=5.0, init='random',
                       max_iter=50, device='cpu')
    with pytest.warns(UserWarning, match='bisection of 33 of 33 rows'):
        model.fit(K)
    assert model.n_uncalibrated_ == n and np.isfinite(model.embedding_).all()


# -- 3. the objective ------------------------------------------------------------------
@pytest.mark.parametrize('n, perplexity', SHAPES)
def test_objective_against_the_definition(n, perplexity):
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    K, d2, cal, P = case(n, perplexity)
    Kt = _t(K)
    diag = Kt.diagonal().to(torch.float64)
    worst = 0.0
    for a in (1.0, 12.0):
        for d in (2, 3):
            for scale in (1e-4, 10.0):
                Y = embedding(n, d, scale)
                kl, grad = _tsne.objective_torch(Kt, diag, *tables(cal),
                                                 _t(Y), a)
                worst = max(worst, check_objective(kl, grad, P, Y, a))
    print(f'n = {n}: at most {worst:.3f} of the bound')


@pytest.mark.parametrize('n, perplexity', SHAPES[:4])
def test_definition_against_scikit_learn(n, perplexity):
    pytest.importorskip('sklearn.manifold')
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _kl_divergence
    K, d2, cal, P = case(n, perplexity)
    for a in (1.0, 12.0):
        for d in (2, 3):
            for scale in (1e-4, 10.0):
                Y = embedding(n, d, scale)
                kl, grad = _kl_divergence(Y.ravel(), squareform(a * P), 1, n,
                                          d)
                check_objective(kl, grad.reshape(n, d), P, Y, a)


def test_the_clamp_of_q():
    """One far outlier: w / Zq < eps for its pairs, and only there does the
    clamp of q change the gradient -- by more than the bound."""
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    n, perplexity = 33, 5.0
    K, d2, cal, P = case(n, perplexity)
    Kt = _t(K)
    Y = outlier_embedding(n, 2)
    kl, grad = _tsne.objective_torch(Kt, Kt.diagonal().to(torch.float64),
                                     *tables(cal), _t(Y), 1.0)
    check_objective(kl, grad, P, Y, 1.0)
    assert clamp_matters(P, Y)


def outlier_embedding(n, d):
    Y = embedding(n, d, 10.0)
    Y[3] = 1e9
    return Y


def clamp_matters(P, Y):
    """Does the gradient without the clamp of q miss the bound?"""
    n = len(Y)
    kl, grad, bkl, bgrad = define_objective(P, Y, 1.0)
    dY = Y[:, None, :] - Y[None, :, :]
    W = 1.0 / (1.0 + (dY ** 2).sum(2))
    np.fill_diagonal(W, 0.0)
    assert (W[3, :3] / W.sum() < EPS).all()
    free = (4.0 * ((P - W / W.sum()) * W)[:, :, None] * dY).sum(1)
    return bool(np.any(np.abs(free - grad) > bgrad))


# -- 4. the step -----------------------------------------------------------------------
_states = {}


def states(n=33, perplexity=5.0):
    """[(Y, update, gains, a, momentum, learning_rate)] of a torch run: the
    start, the first step of phase 2 and step 600."""
    if not _states:
        torch = _torch()
        from graphdot_amd.model.manifold import _tsne
        K, d2, cal, P = case(n, perplexity)
        Kt = _t(K)
        diag = Kt.diagonal().to(torch.float64)
        tab = tables(cal)
        lr = max(n / 12.0 / 4.0, 50.0)
        state = _tsne.State(_t(embedding(n, 2, 1e-4, equal=False)))
        out = []
        for it in range(601):
            if it == 250:
                state.restart()
            a, mom = (12.0, 0.5) if it < 250 else (1.0, 0.8)
            if it in (0, 250, 600):
                out.append((state.Y.numpy().copy(),
                            state.update.numpy().copy(),
                            state.gains.numpy().copy(), a, mom, lr))
            F = _tsne.forces_torch(Kt, diag, *tab, state.Y)
            _tsne.step_torch(state, F, a, mom, lr)
        _states[(n, perplexity)] = out
    return _states[(n, perplexity)]


def check_step(got, P, Y, update, gains, a, momentum, lr):
    """The (Y, update, gains) a step computed against the numpy step."""
    kl, grad, _, bgrad = define_objective(P, Y, a)
    wY, wu, wg = define_step(Y, update, gains, grad, momentum, lr)
    gY, gu, gg = (np.asarray(g) for g in got)
    sure = np.abs(update * grad) > np.abs(update) * bgrad
    assert np.array_equal(gg[sure], wg[sure])
    same = gg == wg
    tol = lr * wg * bgrad + 4 * EPS * (np.abs(wu) + np.abs(wY))
    assert np.all(np.abs(gu - wu)[same] <= tol[same])
    assert np.all(np.abs(gY - wY)[same] <= tol[same])
    return int(sure.sum()), int(same.sum())


def check_norms(g2, gains, P, Y, a):
    """The squared norms of the rows of the gains-scaled gradient."""
    _, grad, _, bgrad = define_objective(P, Y, a)
    gains = np.asarray(gains)
    want = ((gains * grad) ** 2).sum(1)
    tol = 2 * (gains ** 2 * np.abs(grad) * bgrad).sum(1) + 8 * EPS * want
    assert np.all(np.abs(np.asarray(g2) - want) <= tol)


def test_step_against_the_definition():
    from graphdot_amd.model.manifold import _tsne
    torch = _torch()
    n, perplexity = 33, 5.0
    K, d2, cal, P = case(n, perplexity)
    Kt = _t(K)
    diag = Kt.diagonal().to(torch.float64)
    for Y, update, gains, a, mom, lr in states(n, perplexity):
        state = _tsne.State(_t(Y))
        state.update, state.gains = _t(update).clone(), _t(gains).clone()
        F = _tsne.forces_torch(Kt, diag, *tables(cal), state.Y)
        g2 = torch.empty(n, dtype=torch.float64)
        _tsne.step_torch(state, F, a, mom, lr, g2)
        sure, same = check_step((state.Y, state.update, state.gains), P, Y,
                                update, gains, a, mom, lr)
        # (update == 0 at a start: every gain falls, whatever the gradient)
        assert same >= 2 * n - 2 and (sure >= 2 * n - 2 or not update.any())
        check_norms(g2, state.gains, P, Y, a)


# -- 5. the model ----------------------------------------------------------------------
N_MODEL, PERPLEXITY_MODEL = 130, 10.0


def model_kernel():
    return kernel_matrix(points(N_MODEL, 5))


def check_model(model, K, n_iter=None):
    """The attributes of a fitted model; its KL against the definition."""
    n = len(K)
    d = model.n_components
    assert model.embedding_.shape == (n, d)
    assert model.embedding_.dtype == np.float64
    assert model.beta_.shape == (n,) and model.n_uncalibrated_ == 0
    assert isinstance(model.kl_divergence_, float)
    if n_iter is not None:
        assert model.n_iter_ == n_iter
    assert set(model.last_timing) == {'kernel', 'linalg', 'n_iter', 'looks',
                                      'stopped', 'adopted', 'fused'}
    d2 = define_d2(K)
    cal = define_calibrate(d2, model.perplexity)
    assert np.allclose(model.beta_, cal[0], rtol=1e-4, atol=0)
    # the KL of the embedding under the definition's P of the model's beta
    P = define_P(d2, *define_tables(d2, model.beta_))
    kl, _, bkl, _ = define_objective(P, model.embedding_, 1.0)
    assert abs(model.kl_divergence_ - kl) <= bkl
    return kl


def test_model_on_a_precomputed_matrix():
    from graphdot_amd.model.manifold import KernelTSNE
    K = model_kernel()
    K0 = K.copy()
    kw = dict(perplexity=PERPLEXITY_MODEL, device='cpu')
    model = KernelTSNE('precomputed', max_iter=300, **kw)
    Y = model.fit_transform(K)
    assert Y is model.embedding_
    check_model(model, K, 300)
    assert model.last_timing['fused'] is False
    assert model.last_timing['adopted'] is False
    assert model.last_timing['looks'] == 7 and model.learning_rate_ == 50.0
    again = KernelTSNE('precomputed', max_iter=300, **kw).fit(K)
    assert np.array_equal(again.embedding_, Y)
    assert again.kl_divergence_ == model.kl_divergence_
    assert np.array_equal(again.beta_, model.beta_)
    assert np.array_equal(K, K0)
    # the starts
    init = embedding(N_MODEL, 2, 1e-4, seed=3, equal=False)
    for start in (init, 'random', 'kpca'):
        for max_iter in (0, 100, 250):
            m = KernelTSNE('precomputed', init=start, max_iter=max_iter,
                           **kw).fit(K)
            check_model(m, K, max_iter)
            assert m.last_timing['looks'] == max_iter // 50 + 1
        if isinstance(start, np.ndarray):
            zero = KernelTSNE('precomputed', init=start, max_iter=0,
                              **kw).fit(K)
            assert np.array_equal(zero.embedding_, init)
    rnd = KernelTSNE('precomputed', init='random', max_iter=0, random_state=4,
                     **kw).fit(K)
    assert np.array_equal(rnd.embedding_, 1e-4 * np.random.RandomState(
        4).standard_normal((N_MODEL, 2)))
    pca = KernelTSNE('precomputed', init='kpca', max_iter=0, **kw).fit(K)
    assert pca.embedding_[:, 0].std() == pytest.approx(1e-4, rel=1e-12)
    assert pca.embedding_[:, 1].std() < 1e-4
    # three components, and one that only the torch chain has
    for d in (3, 4):
        m = KernelTSNE('precomputed', n_components=d, max_iter=100,
                       **kw).fit(K)
        check_model(m, K, 100)


def test_model_phases_and_early_stop():
    from graphdot_amd.model.manifold import KernelTSNE
    K = model_kernel()
    kw = dict(perplexity=PERPLEXITY_MODEL, device='cpu', init='random')
    # the second phase starts anew at step 250: 251 steps differ from 250
    # steps and one more of the first phase
    a = KernelTSNE('precomputed', max_iter=250, **kw).fit(K)
    b = KernelTSNE('precomputed', max_iter=251, **kw).fit(K)
    assert (a.n_iter_, b.n_iter_) == (250, 251)
    assert a.last_timing['stopped'] is None
    step = np.abs(b.embedding_ - a.embedding_).max()
    assert 0 < step < 0.1 * np.abs(a.embedding_).max()
    stop = KernelTSNE('precomputed', min_grad_norm=np.inf, **kw).fit(K)
    assert stop.n_iter_ == 50 and stop.last_timing['stopped'] == 'gradient norm'
    assert stop.last_timing['looks'] == 2
    short = KernelTSNE('precomputed', max_iter=100, **kw).fit(K)
    assert short.n_iter_ == 100
    same = KernelTSNE('precomputed', max_iter=100, min_grad_norm=0.0,
                      n_iter_without_progress=0, **kw).fit(K)
    assert np.array_equal(same.embedding_, short.embedding_)


def test_errors():
    from graphdot_amd.model.manifold import KernelTSNE
    K = kernel_matrix(points(33, 33))
    kw = dict(device='cpu', max_iter=50)
    for perplexity in (33.0, 40.0):
        with pytest.raises(ValueError, match='perplexity'):
            KernelTSNE('precomputed', perplexity=perplexity, **kw).fit(K)
    with pytest.raises(ValueError, match='perplexity'):
        KernelTSNE('precomputed', perplexity=0.0)
    for d in (0, 1.5, True):
        with pytest.raises(ValueError, match='n_components'):
            KernelTSNE('precomputed', n_components=d)
    with pytest.raises(ValueError, match='init'):
        KernelTSNE('precomputed', init='pca')
    with pytest.raises(ValueError, match='learning_rate'):
        KernelTSNE('precomputed', learning_rate='fast')
    for init in (np.zeros((33, 3)), np.zeros((32, 2)), np.zeros(33)):
        with pytest.raises(ValueError, match='init'):
            KernelTSNE('precomputed', perplexity=5.0, init=init, **kw).fit(K)
    with pytest.raises(ValueError, match='square'):
        KernelTSNE('precomputed', perplexity=5.0, **kw).fit(K[:, :20])
    for bad in (np.nan, np.inf, -np.inf):
        for init in ('random', 'kpca'):
            B = K.copy()
            B[4, 9] = B[9, 4] = bad
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                with pytest.raises(ValueError, match='not finite'):
                    KernelTSNE('precomputed', perplexity=5.0, init=init,
                               **kw).fit(B)
    one = KernelTSNE('precomputed', n_components=1, perplexity=5.0,
                     **kw).fit(K)
    assert one.embedding_.shape == (33, 1)


# -- 6. the quality band ---------------------------------------------------------------
def bands():
    """(least trustworthiness, most KL) a fit must reach: scikit-learn's own
    extremes over five starts, widened by their spread."""
    with open(os.path.join(GOLDEN, 'tsne_bands.json')) as f:
        g = json.load(f)
    assert (g['n'], g['seed'], g['perplexity']) == (N_MODEL, 5,
                                                    PERPLEXITY_MODEL)
    t, k = g['trustworthiness'], g['kl_divergence']
    return g, min(t) - (max(t) - min(t)), max(k) + (max(k) - min(k))


def check_bands(fit):
    """`fit(K, init)` -> model, from the starts s = 5..9."""
    sk = pytest.importorskip('sklearn.manifold')
    g, least, most = bands()
    K = model_kernel()
    D = np.sqrt(define_d2(K))
    for s in range(5, 10):
        init = 1e-4 * np.random.RandomState(s).standard_normal((N_MODEL, 2))
        model = fit(K, init)
        trust = sk.trustworthiness(D, model.embedding_,
                                   n_neighbors=g['n_neighbors'],
                                   metric='precomputed')
        print(f'start {s}: trustworthiness {trust:.4f} (>= {least:.4f}), '
              f'KL {model.kl_divergence_:.4f} (<= {most:.4f}), '
              f'{model.n_iter_} steps')
        assert trust >= least and model.kl_divergence_ <= most


def test_quality_band_of_scikit_learn():
    from graphdot_amd.model.manifold import KernelTSNE
    check_bands(lambda K, init: KernelTSNE(
        'precomputed', perplexity=PERPLEXITY_MODEL, init=init,
        device='cpu').fit(K))


# -- 7. a graph kernel -----------------------------------------------------------------
def test_model_on_graphs_leaves_the_kernel_alone():
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.model.manifold import KernelTSNE
    G = np.asarray(cases.config3_graphs(12, seed=3), dtype=object)
    knode, kedge, q = cases.config3_kernels()
    kernel = MarginalizedGraphKernel(knode, kedge, q=q,
                                     backend=OracleBackend())
    theta0 = np.array(kernel.theta)
    K = np.asarray(kernel(G), dtype=np.float64)
    kw = dict(perplexity=3.0, max_iter=300, device='cpu')
    m = KernelTSNE(kernel, **kw)
    Y = m.fit_transform(G)
    p = KernelTSNE('precomputed', **kw).fit(K)
    assert np.array_equal(kernel.theta, theta0)
    assert m.last_timing['adopted'] is False
    assert m.last_timing['fused'] is False
    assert np.array_equal(Y, p.embedding_)
    assert m.kl_divergence_ == p.kl_divergence_ and m.n_iter_ == 300


# -- 8. the kernels' file unit ---------------------------------------------------------
def test_file_unit_compiles_for_gfx950():
    from graphdot_amd.hip import jit, source_module
    from graphdot_amd.model.manifold import _tsne
    assert list(FILE_UNITS) == ['tsne']
    assert 'tsne' not in source_module.STATIC
    assert 'tsne' not in source_module.TEXT_UNITS
    module = FILE_UNITS['tsne']
    path = os.path.join(os.path.dirname(source_module.__file__), '..',
                        'model', 'manifold', 'tsne.h')
    with open(path) as f:
        assert module.path is None and module.source == f.read()
    assert module.flags == source_module.DENSE_FLAGS
    assert '#include "dense_reduce.h"' in module.source
    assert _tsne._module is module
    image = jit.load_image(module.precompile())
    names = jit.entry_points(module.source)
    assert sorted(names) == sorted(_tsne.ENTRY_POINTS) and len(names) == 14
    for kernel in names:
        assert kernel.encode() in image, kernel


def test_the_file_keys_its_own_unit_alone(tmp_path, monkeypatch):
    """An edit of model/manifold/tsne.h gives its unit a new cache key and
    no other source: the file is no header of csrc/device."""
    import shutil
    from graphdot_amd.hip import jit, source_module
    from graphdot_amd.hip.source_module import STATIC, TEXT_UNITS
    tsne, knn, mmd = FILE_UNITS['tsne'], TEXT_UNITS['knn'], STATIC['mmd.hip']
    relative = source_module.FILE_UNIT_SOURCES['tsne']
    assert relative == 'model/manifold/tsne.h'
    assert not os.path.exists(os.path.join(jit.DEVICE_INCLUDE, 'tsne.h'))

    def keys():
        monkeypatch.setattr(jit, '_hdr_digest', None)
        unit = source_module.SourceModule(source=source_module._text(relative))
        return (unit.key, jit.cache_key(knn.source, knn.flags),
                jit.cache_key(mmd.source, mmd.flags))
    before = keys()
    assert before == (tsne.key, knn.key, mmd.key)
    copy = tmp_path / 'package'
    os.makedirs(copy / 'model')
    shutil.copytree(os.path.join(source_module._PACKAGE, 'model', 'manifold'),
                    copy / 'model' / 'manifold')
    monkeypatch.setattr(source_module, '_PACKAGE', str(copy))
    assert keys() == before
    with open(copy / relative, 'a') as f:
        f.write('// edited\n')
    edited = keys()
    assert edited[0] != before[0] and edited[1:] == before[1:]


def test_the_split_of_the_columns_is_a_function_of_the_shape():
    from graphdot_amd.model.manifold import _tsne
    assert _tsne.parts_for(1000) == 16          # 32 strips, 16 tiles
    assert _tsne.parts_for(4000) == 5           # 125 strips
    assert _tsne.parts_for(64) == 1 and _tsne.parts_for(65) == 2
    assert _tsne.parts_for(130) == 3 and _tsne.parts_for(257) == 5
    assert _tsne.parts_for(100000) == 1
    assert _tsne.parts_for(5, 7) == 7
    for parts in (0, _tsne.PARTS_MOST + 1, 1.5):
        with pytest.raises(ValueError, match='parts'):
            _tsne.parts_for(5, parts)
