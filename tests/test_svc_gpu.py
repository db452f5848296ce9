"""The device path of KernelSVC on an MI355X: `svm_smo` on the definitions
(feasibility, the optimality gap recomputed in numpy double from the stored
matrix, the objective against scikit-learn's within ``tol sum U``), repeats and
slices bit for bit, a problem with a third of its samples left out against the
problem on the sub-matrix, `svm_decide` against `decide_torch` in double on
the CPU, the edge of the fused path at n = NMAX, the model on the HIP backend
against the host model given the downloaded matrix -- no host kernel
evaluation, no n x n download -- and `cross_val_score` as one batch of 120
problems.

The bound of the decision sums: either side's sum of n terms is within ``(n -
1) eps sum |terms|`` of the exact one whatever its order (contraction to FMA
only removes roundings), so two sides differ by ``2 n eps sum |terms|``."""
import numpy as np
import pytest

import test_svc as cpu

pytestmark = pytest.mark.gpu

EPS = cpu.EPS
TOL = cpu.TOL
SIZES = [2, 3, 63, 64, 65, 257, 1000]
BATCHES = [1, 3, 45]
GAMMA = 0.05
CS = [1.0, 10.0, 100.0]


def _torch():
    import torch
    import graphdot_amd.model.svm  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


def _matrix(K, dtype, layout):
    """K stored as `dtype`, contiguous along the index `layout` names."""
    A = _t(K.astype(dtype))
    return A.t().contiguous().t() if layout == 'column-major' else A


_batches = {}


def _batch(n, P):
    """(K, y (P, n) int8, U (P, n)): problem p has its own noisy linear
    labels and C = 1, 10, 100 in turn -- computed once."""
    if (n, P) not in _batches:
        K = cpu.data(n, GAMMA)[0]
        rng = np.random.default_rng(7 * n + P)
        X = rng.normal(size=(n, cpu.DIM))
        y = np.where(X @ rng.normal(size=(cpu.DIM, P))
                     + 0.5 * rng.normal(size=(n, P)) > 0, 1, -1).T
        y[:, 0], y[:, 1] = 1, -1
        U = np.ones((P, n)) * np.array(CS)[np.arange(P) % 3][:, None]
        _batches[n, P] = (K, np.ascontiguousarray(y.astype(np.int8)), U)
    return _batches[n, P]


_objectives = {}


def _sk_objectives(n, P, dtype, stored):
    """scikit-learn's objective of every problem of the batch on the stored
    matrix -- computed once for both layouts."""
    key = (n, P, np.dtype(dtype).name)
    if key not in _objectives:
        _, y, U = _batch(n, P)
        _objectives[key] = np.array([cpu.sk_objective(
            cpu.sk_binary(stored, y[p], U[p, 0], TOL), stored)
            for p in range(P)])
    return _objectives[key]


def _solve(K, y, U, **kwargs):
    from graphdot_amd.model.svm import _smo
    r = _smo.smo(K, _t(y).cuda(), _t(U).cuda(), TOL, **kwargs)
    _torch().cuda.synchronize()
    return r


@pytest.mark.parametrize('layout', ['row-major', 'column-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('P', BATCHES)
@pytest.mark.parametrize('n', SIZES)
def test_smo_on_the_definitions(n, P, dtype, layout):
    """Assertions 1 to 3 of test_svc.py on the downloaded alpha, against the
    stored matrix widened to double; two launches give the same bits."""
    torch = _torch()
    K, y, U = _batch(n, P)
    Kt = _matrix(K, dtype, layout)
    stored = Kt.to(torch.float64).numpy()
    a, b = (_solve(Kt.cuda(), y, U) for _ in range(2))
    for name in ('alpha', 'G', 'info'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    alpha, G, info = (x.cpu().numpy() for x in (a.alpha, a.G, a.info))
    assert np.all(info[:, 3] == 0) and np.all(info[:, 1] - info[:, 2] < TOL)
    cpu.check_feasible(y, U, alpha)
    cpu.check_optimal(stored, y, U, alpha, TOL)
    f = 0.5 * (alpha * (G - 1.0)).sum(1)
    f_ref = _sk_objectives(n, P, dtype, stored)
    print(f'n {n} P {P}: steps {info[:, 0].min():.0f} to {info[:, 0].max():.0f}'
          f', slices {a.slices}, objective off by '
          f'{(np.abs(f - f_ref) / (TOL * U.sum(1))).max():.3g} of the bound')
    assert np.all(np.abs(f - f_ref) <= TOL * U.sum(1))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n,P', [(3, 1), (65, 3), (257, 3), (1000, 45)])
def test_slices(n, P, dtype):
    """7 steps per launch against one long slice: the state's round trip
    through the workspace loses nothing, and a problem that has stopped is
    left as it is by the launches the others still need."""
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    K, y, U = _batch(n, P)
    Kd = _matrix(K, dtype, 'row-major').cuda()
    whole = _solve(Kd, y, U, steps=10 ** 6)
    assert whole.slices == 1
    short = _solve(Kd, y, U, steps=7)
    steps = whole.info[:, 0].cpu().numpy()
    assert short.slices == max(1, int(-(-(steps.max() + 1) // 7))) \
        or short.slices == max(1, int(-(-steps.max() // 7)))
    for name in ('alpha', 'G', 'info'):
        assert torch.equal(getattr(whole, name), getattr(short, name)), name
    if P == 1:
        return
    # by hand: what a stopped problem holds when it is first seen stopped
    yd, Ud = _t(y).cuda(), _t(U).cuda()
    state, info = _smo.start(P, n, Kd.device)
    seen = {}
    for _ in range(short.slices):
        _smo.smo_slice(Kd, yd, Ud, state, info, TOL, 7, 10 ** 6)
        h = info.cpu().numpy()
        for p in np.flatnonzero(_smo.stopped(h, TOL, 10 ** 6)):
            seen.setdefault(int(p), (state[p].clone(), info[p].clone()))
    assert len(seen) == P
    assert steps.max() - steps.min() >= 14 or n < 257      # (slices apart)
    for p, (s, i) in seen.items():
        assert torch.equal(s, state[p]) and torch.equal(i, info[p])
    assert torch.equal(state[:, 0], whole.alpha)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [3, 65, 257, 1000])
def test_membership(n, dtype):
    """Problem 1 is problem 0 with a third of the samples given U = 0: their
    coefficients are exactly 0, and the rest is a solution of the problem on
    the sub-matrix within the bounds of the assertions 1 to 3."""
    torch = _torch()
    K, y, U = _batch(n, 1)
    out = np.arange(n) % 3 == 2
    y2, U2 = np.concatenate((y, y)), np.concatenate((U, U))
    U2[1, out] = 0.0
    Kt = _matrix(K, dtype, 'row-major')
    stored = Kt.to(torch.float64).numpy()
    r = _solve(Kt.cuda(), y2, U2)
    alpha, G = r.alpha.cpu().numpy(), r.G.cpu().numpy()
    assert np.all(alpha[1, out] == 0)
    keep = ~out
    sub = np.ascontiguousarray(stored[np.ix_(keep, keep)])
    ys, Us = y[:, keep], U[:, keep]
    cpu.check_feasible(ys, Us, alpha[1:, keep])
    cpu.check_optimal(sub, ys, Us, alpha[1:, keep], TOL)
    alone = _solve(_t(sub.astype(dtype)).cuda(), ys, Us)
    f = 0.5 * (alpha[1] * (G[1] - 1.0))[keep].sum()
    f_alone = 0.5 * float((alone.alpha * (alone.G - 1.0)).sum())
    f_ref = cpu.sk_objective(cpu.sk_binary(sub, ys[0], Us[0, 0], TOL), sub)
    assert abs(f - f_alone) <= TOL * Us.sum()
    assert abs(f - f_ref) <= TOL * Us.sum()
    print(f'n {n}: the same bits as the solve alone: '
          f'{np.array_equal(alone.alpha.cpu().numpy()[0], alpha[1, keep])}')


@pytest.mark.parametrize('layout', ['row-major', 'column-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('P', [1, 2, 9, 16, 17, 45])
@pytest.mark.parametrize('b', [1, 65, 257])
def test_decide_against_restatement(b, P, dtype, layout):
    """``|out - ref| <= 2 n eps sum_j |Ks_rj coef_pj|``."""
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    n = 257
    rng = np.random.default_rng(100 * b + P)
    Ks = rng.normal(size=(b, n)) + 0.7
    coef = rng.normal(size=(P, n)) * (rng.random((P, n)) < 0.6)
    icpt = rng.normal(size=P)
    Kt = _t(Ks.astype(dtype))
    if layout == 'column-major':               # r + j b, as the solver leaves it
        Kt = Kt.t().contiguous().t()
    stored = Kt.to(torch.float64)
    ref = _smo.decide_torch(stored, _t(coef), _t(icpt)).numpy()
    a, c = (_smo.decide(Kt.cuda(), _t(coef).cuda(), _t(icpt).cuda())
            for _ in range(2))
    torch.cuda.synchronize()
    assert torch.equal(a, c)                  # bit-identical repeats
    out = a.cpu().numpy()
    assert out.shape == ref.shape == (P, b)
    size = np.abs(coef) @ np.abs(stored.numpy()).T
    assert np.all(np.abs(out - ref) <= 2 * n * EPS * size)


def test_launches_check_their_arguments():
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    n = 8
    K = torch.eye(n, dtype=torch.float64, device='cuda')
    y = torch.ones((1, n), dtype=torch.int8, device='cuda')
    U = torch.ones((1, n), dtype=torch.float64, device='cuda')
    with pytest.raises(TypeError):
        _smo.smo(K.cpu(), y, U)
    with pytest.raises(TypeError):
        _smo.smo(K, y.int(), U)
    with pytest.raises(TypeError):
        _smo.smo(K, y, U[:, :4])
    with pytest.raises(ValueError):
        _smo.smo(K, y, U, tol=0.0)
    with pytest.raises(ValueError):
        _smo.smo(K, y, U, steps=0)
    with pytest.raises(ValueError):
        _smo.smo(K[:, ::2][:4], y[:, :4], U[:, :4])      # strided
    with pytest.raises(TypeError):
        _smo.decide(K, U.cpu(), U[0, :1])
    out = _smo.decide(K[:0], U, U[0, :1].contiguous())
    assert out.shape == (1, 0)
    # one class only: I_low is empty, nothing moves
    r = _smo.smo(K, y, U)
    assert r.info.cpu().numpy()[0].tolist() == [0, 1, np.inf, 0]
    assert torch.all(r.alpha == 0)
    bad = K.clone()
    bad[2, 2] = float('nan')
    y[0, 1] = -1
    assert _smo.smo(bad, y, U).info.cpu().numpy()[0, 3] == 1


# -- the edge of the fused path ----------------------------------------------------
_edge = {}


def _blobs():
    """Two well-separated blobs, NMAX + 1 training points and NEW new ones."""
    from graphdot_amd.model.svm import _smo
    if not _edge:
        n = _smo.NMAX + 1
        rng = np.random.default_rng(0)
        lab = np.arange(n + cpu.NEW) % 2
        X = rng.normal(size=(n + cpu.NEW, cpu.DIM))
        X[:, 0] += np.where(lab > 0, 3.0, -3.0)
        sq = (X * X).sum(1)
        K = np.exp(-GAMMA * np.maximum(
            sq[:, None] + sq[None, :] - 2 * X @ X.T, 0))
        _edge['K'], _edge['lab'] = (K + K.T) / 2, lab
    return _edge['K'], _edge['lab']


@pytest.mark.parametrize('over', [0, 1])
def test_the_edge_of_the_fused_path(over):
    """n = NMAX runs fused, n = NMAX + 1 through `smo_torch` on the device;
    both give scikit-learn's labels under the delta rule.  With C = 1 the
    restatement needs 82 steps on the CPU for either size (two blobs six
    standard deviations apart), so neither path runs long."""
    from graphdot_amd.model.svm import KernelSVC, _smo
    torch = _torch()
    K, lab = _blobs()
    n = _smo.NMAX + over
    Kn = np.ascontiguousarray(K[:n, :n])
    Ks = np.ascontiguousarray(K[-cpu.NEW:, :n])
    want, sure, D = cpu.delta_rule(Kn, Ks, lab[:n], 1.0, None, f'n {n}')
    Z = torch.from_numpy(np.concatenate((Kn, Ks))).cuda()
    m = KernelSVC('precomputed', C=1.0, tol=TOL, device='cuda').fit(
        Z[:n], lab[:n])
    assert m.last_timing['fused'] is (over == 0)
    assert m.n_iter_[0] < 1000 and m.gap_[0] < TOL
    got = m.predict(Z)
    assert np.array_equal(got[sure], want[sure])
    assert np.all((np.sign(m.decision_function(Z)) == np.sign(D))[sure])
    y, U, alpha = cpu.problems_of(m, lab[:n])
    cpu.check_feasible(y, U, alpha)


# -- the model on QM7-like graphs ---------------------------------------------------
N_TRAIN, N_HELD_OUT = 40, 8


def _graphs():
    import cases
    G = np.asarray(list(cases.config3_graphs(N_TRAIN + N_HELD_OUT, seed=29)),
                   dtype=object)
    return G[:N_TRAIN], G[N_TRAIN:]


def _kernel(real):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    knode, kedge, q = cases.config3_fit_kernels()
    return Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, q_bounds=(1e-3, 0.5), backend=HIPBackend(real=real),
        ftol=1e-13 if real is np.float64 else 1e-8))


@pytest.mark.parametrize('real', [np.float32, np.float64])
def test_device_matches_host(real, monkeypatch):
    """The model on the device path against the host model on the very
    matrices the device path worked on (downloaded here, for the test)."""
    from graphdot_amd.model.svm import KernelSVC
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G, Z = _graphs()
    n, C = N_TRAIN, 10.0
    kernel = _kernel(real)
    # three classes by the number of atoms, a property the kernel sees
    size = np.array([len(g.nodes) for g in G])
    lab = np.searchsorted(np.quantile(size, [1 / 3, 2 / 3]), size)
    assert len(np.unique(lab)) == 3
    K = torch.as_tensor(kernel.device_gram(G), device='cuda').cpu().numpy() \
        .astype(np.float64)
    Ks = torch.as_tensor(kernel.device_cross_gram(Z, G),
                         device='cuda').cpu().numpy().astype(np.float64)
    host = cpu.model(C=C).fit(K, lab)
    want, sure, D = cpu.delta_rule(K, Ks, lab, C, None, real.__name__)
    calls, downloads = [], []

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
        monkeypatch.setattr(cls, 'diag', counting)
    to_host = torch.Tensor.cpu

    def cpu_counting(self, *args, **kwargs):
        if self.is_cuda and self.numel() >= n * n:
            downloads.append(tuple(self.shape))
        return to_host(self, *args, **kwargs)
    monkeypatch.setattr(torch.Tensor, 'cpu', cpu_counting)
    dev = KernelSVC(kernel, C=C, tol=TOL, device='cuda').fit(G, lab)
    got = np.concatenate((dev.predict(G), dev.predict(Z)))
    F = dev.decision_function(Z)
    assert dev.last_timing['adopted'] is True
    assert dev.last_timing['fused'] is True
    assert calls == [] and downloads == []
    assert np.array_equal(got[sure], want[sure])
    assert F.shape == (N_HELD_OUT, 3)
    y, U, alpha = cpu.problems_of(dev, lab)
    cpu.check_feasible(y, U, alpha)
    cpu.check_optimal(K, y, U, alpha, TOL)
    print(f'{real.__name__}: steps {dev.n_iter_} against {host.n_iter_}, '
          f'objective {dev.objective_} against {host.objective_}')
    assert np.all(np.abs(dev.objective_ - host.objective_) <= TOL * U.sum(1))
    assert np.array_equal(dev.pairs_, host.pairs_)


def test_cross_val_score_on_the_device():
    """8 values of C x 5 folds x 3 class pairs = 120 problems in one batch
    against the host chain.  A held-out point is sure where every pairwise
    decision of scikit-learn on the fold exceeds the delta of its problem
    (test_svc.delta_rule); the accuracies of a fold may differ by the share
    of its points that are not, and at most 5 % of all held-out points are
    not."""
    from graphdot_amd.model.svm import KernelSVC
    torch = _torch()
    n = 257
    K, _, lab, _ = cpu.data(n, GAMMA, 3)
    Cs = [0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    host = cpu.model().cross_val_score(K, lab, Cs, cv=5, random_state=3)
    m = KernelSVC('precomputed', tol=TOL, device='cuda')
    got = m.cross_val_score(torch.from_numpy(K).cuda(), lab, Cs, cv=5,
                            random_state=3)
    assert m.last_timing['fused'] is True
    assert m.last_timing['problems'] == 120
    assert got.shape == host.shape == (8, 5)
    codes = np.searchsorted(np.unique(lab), lab)
    folds = KernelSVC._folds(codes, 5, 3)
    unsure = np.zeros((8, 5))
    for a, C in enumerate(Cs):
        for f, (train, test) in enumerate(folds):
            sub = np.ascontiguousarray(K[np.ix_(train, train)])
            ref = cpu.sk_binary(sub, lab[train], C, TOL)
            fine = cpu.sk_binary(sub, lab[train], C, TOL / 1000)
            D = ref.decision_function(K[np.ix_(test, train)])
            delta = 4 * np.abs(
                D - fine.decision_function(K[np.ix_(test, train)])).max(0)
            unsure[a, f] = (np.abs(D) <= delta).any(1).sum()
    sizes = np.array([len(test) for _, test in folds])
    print(f'{int(unsure.sum())} of {8 * n} held-out points left out; largest '
          f'difference {np.abs(got - host).max():.3g}')
    assert unsure.sum() <= cpu.LEFT_OUT * 8 * n
    assert np.all(np.abs(got - host) <= (unsure + 1e-9) / sizes[None, :])
