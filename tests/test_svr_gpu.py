"""The device path of KernelSVR and KernelOneClassSVM on an MI355X: `svm_smo2`
on the definitions (feasibility, the optimality gap recomputed in numpy double
from the stored matrix, the objective against scikit-learn's within ``tol 2 sum
U``), repeats and slices bit for bit, a problem with a third of its samples
left out against the problem on the sub-matrix, the one-class problems through
`svm_smo` from `one_class_start`, the edge of the fused path at n = NMAX2, the
models on the HIP backend against the host models given the downloaded matrix
-- no host kernel evaluation, no n x n download -- and `cross_val_score` as
one batch of 40 problems.

The bounds are those of test_svr.py; the bound of the decision sums is that
of test_svc_gpu.py (``2 n eps sum |terms|``)."""
import numpy as np
import pytest

import test_svc as svc
import test_svr as cpu

pytestmark = pytest.mark.gpu

EPS = svc.EPS
TOL = svc.TOL
NEW = svc.NEW
SIZES = [2, 3, 63, 64, 65, 257, 1000, 1025]
BATCHES = [1, 3, 24]
GAMMA = 0.05
#: (C, epsilon) of problem p: ``COMBOS[p % 4]``
COMBOS = [(1.0, 0.05), (10.0, 0.3), (1.0, 0.3), (10.0, 0.05)]
NUS = [0.2, 0.5, 0.05]


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


def _batch(n, P):
    """(K, U (P, n), z (P, n), eps (P,)): the first P problems of a batch of
    24 over the one matrix; problem p has C and epsilon in turn and the
    targets scaled by 1, -1.25, 1.5, ... (its own every four)."""
    K, _, z, _ = cpu.data(n, GAMMA)
    p = np.arange(P)
    C = np.array([COMBOS[q % 4][0] for q in p])
    eps = np.array([COMBOS[q % 4][1] for q in p])
    scale = (1 + 0.25 * (p // 4)) * np.where((p // 4) % 2, -1.0, 1.0)
    return K, np.ones((P, n)) * C[:, None], scale[:, None] * z[None, :], eps


_objectives = {}


def _sk_objectives(n, P, dtype, stored):
    """scikit-learn's objective of the first P problems on the stored matrix
    -- each computed once for all batch sizes and both layouts."""
    _, U, z, eps = _batch(n, P)
    out = np.empty(P)
    for p in range(P):
        key = (n, p, np.dtype(dtype).name)
        if key not in _objectives:
            _objectives[key] = cpu.sk_objective2(
                cpu.sk_svr(stored, z[p], U[p, 0], eps[p], TOL), stored, z[p],
                eps[p])
        out[p] = _objectives[key]
    return out


def _solve(K, U, z, eps, **kwargs):
    from graphdot_amd.model.svm import _smo
    r = _smo.smo2(K, _t(U).cuda(), _t(z), _t(eps), TOL, **kwargs)
    _torch().cuda.synchronize()
    return r


def _objective(alpha, G, z, eps):
    p = np.concatenate((eps[:, None] - z, eps[:, None] + z), axis=1)
    return 0.5 * (alpha * (G + p)).sum(1)


@pytest.mark.parametrize('layout', ['row-major', 'column-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('P', BATCHES)
@pytest.mark.parametrize('n', SIZES)
def test_smo2_on_the_definitions(n, P, dtype, layout):
    """Assertions 1 to 3 of test_svr.py on the downloaded state, against the
    stored matrix widened to double; two runs give the same bits."""
    torch = _torch()
    K, U, z, eps = _batch(n, P)
    Kt = _matrix(K, dtype, layout)
    stored = Kt.to(torch.float64).numpy()
    a, b = (_solve(Kt.cuda(), U, z, eps) for _ in range(2))
    for name in ('alpha', 'G', 'info'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    alpha, G, info = (x.cpu().numpy() for x in (a.alpha, a.G, a.info))
    assert alpha.shape == G.shape == (P, 2 * n)
    assert np.all(info[:, 3] == 0) and np.all(info[:, 1] - info[:, 2] < TOL)
    cpu.check2(stored, z, eps, U, alpha, TOL)
    f = _objective(alpha, G, z, eps)
    f_ref = _sk_objectives(n, P, dtype, stored)
    bound = TOL * 2 * U.sum(1)
    print(f'n {n} P {P}: steps {info[:, 0].min():.0f} to {info[:, 0].max():.0f}'
          f', slices {a.slices}, objective off by '
          f'{(np.abs(f - f_ref) / bound).max():.3g} of the bound')
    assert np.all(np.abs(f - f_ref) <= bound)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n,P', [(3, 1), (65, 3), (257, 3), (1000, 24)])
def test_slices(n, P, dtype):
    """7 steps per launch against one long slice: the state's round trip
    through the workspace loses nothing, and a problem that has stopped is
    left as it is by the launches the others still need."""
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    K, U, z, eps = _batch(n, P)
    Kd = _matrix(K, dtype, 'row-major').cuda()
    whole = _solve(Kd, U, z, eps, steps=10 ** 6)
    assert whole.slices == 1
    short = _solve(Kd, U, z, eps, steps=7)
    steps = whole.info[:, 0].cpu().numpy()
    assert short.slices == max(1, int(-(-(steps.max() + 1) // 7))) \
        or short.slices == max(1, int(-(-steps.max() // 7)))
    for name in ('alpha', 'G', 'info'):
        assert torch.equal(getattr(whole, name), getattr(short, name)), name
    if P == 1:
        return
    # by hand: what a stopped problem holds when it is first seen stopped
    Ud = _t(U).cuda()
    state, info = _smo.start2(_t(z), _t(eps), Kd.device)
    seen = {}
    for _ in range(short.slices):
        _smo.smo2_slice(Kd, Ud, state, info, TOL, 7, 10 ** 6)
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
    """Problem 1 is problem 0 with a third of the samples given U = 0: both
    of their variables are exactly 0, and the rest is a solution of the
    problem on the sub-matrix within the bounds of the assertions 1 to 3."""
    torch = _torch()
    K, U, z, eps = _batch(n, 1)
    out = np.arange(n) % 3 == 2
    U2, z2, eps2 = (np.concatenate((x, x)) for x in (U, z, eps))
    U2[1, out] = 0.0
    Kt = _matrix(K, dtype, 'row-major')
    stored = Kt.to(torch.float64).numpy()
    r = _solve(Kt.cuda(), U2, z2, eps2)
    alpha, G = r.alpha.cpu().numpy(), r.G.cpu().numpy()
    both = np.tile(out, 2)
    assert np.all(alpha[1, both] == 0)
    keep = ~out
    sub = np.ascontiguousarray(stored[np.ix_(keep, keep)])
    Us, zs = U[:, keep], z[:, keep]
    a1, G1 = alpha[1:, ~both], G[1:, ~both]
    cpu.check2(sub, zs, eps, Us, a1, TOL)
    f = _objective(a1, G1, zs, eps)[0]
    f_ref = cpu.sk_objective2(cpu.sk_svr(sub, zs[0], Us[0, 0], eps[0], TOL),
                              sub, zs[0], eps[0])
    assert abs(f - f_ref) <= TOL * 2 * Us.sum()
    alone = _solve(_t(sub.astype(dtype)).cuda(), Us, zs, eps)
    print(f'n {n}: the same bits as the solve alone: '
          f'{np.array_equal(alone.alpha.cpu().numpy(), a1)}')
    f_alone = _objective(alone.alpha.cpu().numpy(), alone.G.cpu().numpy(),
                         zs, eps)[0]
    assert abs(f - f_alone) <= TOL * 2 * Us.sum()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [3, 65, 257, 1000])
def test_one_class_through_svm_smo(n, dtype):
    """A batch of three values of nu from `one_class_start`: G0 of the decide
    launch against ``K a0`` in numpy double, then the assertions 1 to 3."""
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    K = cpu.data(n, GAMMA)[0]
    Kt = _matrix(K, dtype, 'row-major')
    stored = Kt.to(torch.float64).numpy()
    nu = np.array(NUS)
    Kd = Kt.cuda()
    U = torch.ones((3, n), dtype=torch.float64, device='cuda')
    y = torch.ones((3, n), dtype=torch.int8, device='cuda')
    state, info = _smo.one_class_start(Kd, _t(nu), U)
    assert state.is_cuda and info.cpu().numpy().tolist() == [
        [0, np.inf, -np.inf, 0]] * 3
    a0, G0 = state[:, 0].cpu().numpy(), state[:, 1].cpu().numpy()
    for p in range(3):
        full = int(nu[p] * n)
        assert np.all(a0[p, :full] == 1) and np.all(a0[p, full + 1:] == 0)
    assert np.all(np.abs(G0 - a0 @ stored) <= 2 * n * EPS * (a0 @ np.abs(stored)))
    r = _smo.smo_from(Kd, y, U, state, info, TOL)
    torch.cuda.synchronize()
    a, G, h = (x.cpu().numpy() for x in (r.alpha, r.G, r.info))
    assert np.all(h[:, 3] == 0) and np.all(h[:, 1] - h[:, 2] < TOL)
    assert np.all(a >= 0) and np.all(a <= 1)
    assert np.all(np.abs(a.sum(1) - nu * n) <= 4 * n * EPS * nu * n)
    ones = np.ones(n)
    for p in range(3):
        gap, slack = svc.gap_of(stored, ones, ones, a[p])
        assert gap <= TOL + slack, (p, gap, slack)
        c = cpu.sk_coef(cpu.sk_one(stored, nu[p], TOL), n)
        f, f_ref = 0.5 * (a[p] * G[p]).sum(), 0.5 * c @ stored @ c
        print(f'n {n} nu {nu[p]}: {h[p, 0]:.0f} steps, objective off by '
              f'{abs(f - f_ref) / (TOL * n):.3g} of the bound')
        assert abs(f - f_ref) <= TOL * n


def test_launches_check_their_arguments():
    from graphdot_amd.model.svm import _smo
    torch = _torch()
    n = 8
    K = torch.eye(n, dtype=torch.float64, device='cuda')
    U = torch.ones((1, n), dtype=torch.float64, device='cuda')
    z = torch.arange(n, dtype=torch.float64)[None] / n
    eps = torch.tensor([0.1], dtype=torch.float64)
    y = torch.ones((1, n), dtype=torch.int8, device='cuda')
    with pytest.raises(TypeError):
        _smo.smo2(K.cpu(), U, z, eps)
    with pytest.raises(TypeError):
        _smo.smo2(K, U.float(), z, eps)
    with pytest.raises(TypeError):
        _smo.smo2(K, U[:, :4], z, eps)
    with pytest.raises(TypeError):
        _smo.smo2(K, U, z[:, :4], eps)
    with pytest.raises(TypeError):
        _smo.smo2(K, U, z, eps.float())
    with pytest.raises(ValueError):
        _smo.smo2(K, U, z, -eps)
    with pytest.raises(ValueError):
        _smo.smo2(K, U, z, eps, tol=0.0)
    with pytest.raises(ValueError):
        _smo.smo2(K, U, z, eps, steps=0)
    with pytest.raises(ValueError):
        _smo.smo2(K[:, ::2][:4], U[:, :4], z[:, :4], eps)      # strided
    with pytest.raises(ValueError):
        _smo.smo2(K, U.cpu(), z, eps)
    state, info = _smo.start2(z, eps, K.device)
    with pytest.raises(TypeError):
        _smo.smo2_slice(K, U, state[:, :, :n], info, TOL, 7, 100)
    with pytest.raises(TypeError):
        _smo.smo2_slice(K, U, state, info[:, :3], TOL, 7, 100)
    with pytest.raises(TypeError):
        _smo.smo_from(K, y, U, state, info)                 # (2n: not n)
    big = torch.zeros((_smo.NMAX2 + 1,) * 2, dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match='NMAX2'):
        _smo.smo2_slice(big, U, state, info, TOL, 7, 100)
    # epsilon above every |z|: nothing is in I_low, nothing moves
    wide = 2 * 0.1 + 1
    r = _smo.smo2(K, U, z, 2 * eps + 1)
    assert r.info.cpu().numpy()[0].tolist() == [0, -(wide - 7 / 8), wide, 0]
    assert torch.all(r.alpha == 0)
    bad = K.clone()
    bad[2, 2] = float('nan')
    assert _smo.smo2(bad, U, z, eps).info.cpu().numpy()[0, 3] == 1


# -- the edge of the fused path ----------------------------------------------------
_edge = {}


def _smooth():
    """A smooth target on NMAX2 + 1 training points and NEW new ones."""
    from graphdot_amd.model.svm import _smo
    if not _edge:
        n = _smo.NMAX2 + 1
        rng = np.random.default_rng(0)
        X = rng.normal(size=(n + NEW, cpu.DIM))
        sq = (X * X).sum(1)
        K = np.exp(-GAMMA * np.maximum(
            sq[:, None] + sq[None, :] - 2 * X @ X.T, 0))
        _edge['K'], _edge['z'] = (K + K.T) / 2, np.sin(X[:, 0])
    return _edge['K'], _edge['z']


@pytest.mark.parametrize('over', [0, 1])
def test_the_edge_of_the_fused_path(over):
    """n = NMAX2 runs fused, n = NMAX2 + 1 through `smo2_torch` on the
    device; both within the delta of scikit-learn's predictions.  With C = 1
    and epsilon = 0.3 the restatement needs 666 steps on the CPU for n =
    NMAX2 + 1 (scikit-learn: 653 for either size), so neither path runs
    long."""
    from graphdot_amd.model.svm import KernelSVR, _smo
    torch = _torch()
    K, z = _smooth()
    n = _smo.NMAX2 + over
    Kn = np.ascontiguousarray(K[:n, :n])
    Ks = np.ascontiguousarray(K[-NEW:, :n])
    Zh = np.concatenate((Kn, Ks))
    want, delta = cpu.delta_svr(Kn, Zh, z[:n], 1.0, 0.3)
    Z = torch.from_numpy(Zh).cuda()
    # assertions 1 and 2 on the solver's own 2n variables
    U, zs, eps = np.ones((1, n)), z[None, :n], np.array([0.3])
    r, fused = _smo.solve2(Z[:n], _t(U), _t(zs), _t(eps), TOL, 10 ** 6)
    assert fused is (over == 0) and r.alpha.is_cuda
    cpu.check2(Kn, zs, eps, U, r.alpha.cpu().numpy(), TOL)
    m = KernelSVR('precomputed', C=1.0, epsilon=0.3, tol=TOL,
                  device='cuda').fit(Z[:n], z[:n])
    assert m.last_timing['fused'] is (over == 0)
    assert m._state[0].is_cuda
    assert m.n_iter_ == r.info[0, 0] < 1000 and m.gap_ < TOL
    got = m.predict(Z)
    off = np.abs(got - want).max()
    print(f'n {n}: {m.n_iter_} steps, off by {off:.3g}, {off / delta:.3g} x '
          f'the unscaled delta {delta:.3g}')
    assert delta > 0 and off <= 4 * delta


# -- the models on QM7-like graphs ---------------------------------------------------
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
    """The models on the device path against the host models on the very
    matrices the device path worked on (downloaded here, for the test)."""
    from graphdot_amd.model.svm import KernelOneClassSVM, KernelSVR
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G, Z = _graphs()
    # (nu = 0.3: at 0.2 scikit-learn's decision values at tol and at tol /
    # 1000 are the same bits on these matrices, and the delta rule is void)
    n, C, eps, nu = N_TRAIN, 10.0, 0.1, 0.3
    kernel = _kernel(real)
    # the number of atoms, a property the kernel sees, standardised
    size = np.array([float(len(g.nodes)) for g in G])
    z = (size - size.mean()) / size.std()
    K = torch.as_tensor(kernel.device_gram(G), device='cuda').cpu().numpy() \
        .astype(np.float64)
    Ks = torch.as_tensor(kernel.device_cross_gram(Z, G),
                         device='cuda').cpu().numpy().astype(np.float64)
    both = np.concatenate((K, Ks))
    host = cpu.svr(C=C, epsilon=eps).fit(K, z)
    host1 = cpu.one_class(nu=nu).fit(K)
    want, delta = cpu.delta_svr(K, both, z, C, eps)
    want1, delta1 = cpu.delta_one(K, both, nu)
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
    dev = KernelSVR(kernel, C=C, epsilon=eps, tol=TOL, device='cuda').fit(G, z)
    got = np.concatenate((dev.predict(G), dev.predict(Z)))
    assert dev.last_timing['adopted'] is True
    assert dev.last_timing['fused'] is True
    dev1 = KernelOneClassSVM(kernel, nu=nu, tol=TOL, device='cuda').fit(G)
    got1 = np.concatenate((dev1.decision_function(G),
                           dev1.decision_function(Z)))
    assert dev1.last_timing['adopted'] is True
    assert dev1.last_timing['fused'] is True
    assert calls == [] and downloads == []
    print(f'{real.__name__}: SVR steps {dev.n_iter_} against {host.n_iter_}, '
          f'objective {dev.objective_} against {host.objective_}, predictions '
          f'{np.abs(got - want).max() / delta:.3g} x the unscaled delta; '
          f'one-class steps {dev1.n_iter_} against {host1.n_iter_}, objective '
          f'{dev1.objective_} against {host1.objective_}, decisions '
          f'{np.abs(got1 - want1).max() / delta1:.3g} x the unscaled delta')
    assert abs(dev.objective_ - host.objective_) <= TOL * 2 * C * n
    assert delta > 0 and np.abs(got - want).max() <= 4 * delta
    assert dev.gap_ < TOL and dev.dual_coef_.shape == (n,)
    assert np.all(np.abs(dev.dual_coef_) <= C)
    assert abs(dev.dual_coef_.sum()) <= 4 * 2 * n * EPS * np.abs(
        dev.dual_coef_).sum()
    assert abs(dev1.objective_ - host1.objective_) <= TOL * n
    assert delta1 > 0 and np.abs(got1 - want1).max() <= 4 * delta1
    a = dev1.dual_coef_
    assert np.all(a >= 0) and np.all(a <= 1)
    assert abs(a.sum() - nu * n) <= 4 * n * EPS * nu * n
    gap, slack = svc.gap_of(K, np.ones(n), np.ones(n), a)
    assert gap <= TOL + slack
    assert np.array_equal(dev1.predict(Z), np.where(got1[n:] > 0, 1, -1))


def test_cross_val_score_on_the_device():
    """4 values of C x 2 of epsilon x 5 folds = 40 problems in one batch
    against the host chain, within the propagated bound of
    test_svr.test_svr_cross_val_score_against_a_loop_of_fits."""
    from graphdot_amd.model.svm import KernelSVC, KernelSVR
    torch = _torch()
    n = 257
    K, _, z, _ = cpu.data(n, GAMMA)
    # (C from 0.5: at C = 0.0625 one fold's predictions of scikit-learn at
    # tol and at tol / 1000 are the same bits, and the delta rule is void)
    Cs, es = [0.5, 1.0, 2.0, 3.0], [0.05, 0.3]
    host = cpu.svr().cross_val_score(K, z, Cs, es, cv=5, random_state=3)
    m = KernelSVR('precomputed', tol=TOL, device='cuda')
    got = m.cross_val_score(torch.from_numpy(K).cuda(), z, Cs, es, cv=5,
                            random_state=3)
    assert m.last_timing['fused'] is True
    assert m.last_timing['problems'] == 40
    assert got.shape == host.shape == (4, 2, 5)
    folds = KernelSVC._folds(np.zeros(n, dtype=np.int64), 5, 3)
    worst = 0.0
    for a, C in enumerate(Cs):
        for e, eps in enumerate(es):
            for f, (train, test) in enumerate(folds):
                sub = np.ascontiguousarray(K[np.ix_(train, train)])
                cross = np.ascontiguousarray(K[np.ix_(test, train)])
                one = cpu.svr(C=C, epsilon=eps).fit(sub, z[train])
                _, d = cpu.delta_svr(sub, np.concatenate((sub, cross)),
                                     z[train], C, eps)
                assert d > 0, (C, eps, f)              # (or the rule is void)
                d *= 4
                r = z[test] - one.predict(cross)
                total = ((z[test] - z[test].mean()) ** 2).sum()
                bound = (2 * np.abs(r) * d + d * d).sum() / total
                off = abs(got[a, e, f] - host[a, e, f])
                print(f'C {C} eps {eps} fold {f}: off by {off:.3g}, '
                      f'{off / bound:.3g} of the bound {bound:.3g}')
                worst = max(worst, off / bound)
    print(f'largest difference {np.abs(got - host).max():.3g}, largest share '
          f'of the propagated bound {worst:.3g}')
    assert worst <= 1
