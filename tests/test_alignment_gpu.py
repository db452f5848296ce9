"""The device path of KernelTargetAlignment on an MI355X: the launches of
alignment.hip against the definition of the centred alignment in numpy double
(test_alignment.py: its data, its definition and its rounding bound) on the
stored matrix and planes widened to double, for float and double storage,
both layouts of the matrix and the planes contiguous along each of their
axes, a plane list that selects and reorders, repeats bit for bit; against
`alignment_torch` on the same device tensors; the edge of the fused path at
17 target columns; and the model on the HIP backend against the definition on
the very matrix and planes it worked on -- no host kernel evaluation -- with
a short `fit`.

Sizes: one tile (2, 3, 63, 64), the tile edge on both sides (63, 64, 65), a
diagonal plus off-diagonal tiles (65, 129, 257); 17 planes are two chunks."""
import numpy as np
import pytest

import test_alignment as cpu

pytestmark = pytest.mark.gpu

EPS = cpu.EPS
SIZES = [2, 3, 63, 64, 65, 129, 257]
PLANES = cpu.PLANES
COLUMNS = [1, 2, 16]
#: a plane list that selects and reorders, per number of planes
PICKS = {3: [2, 0], 17: [16, 0, 5, 1, 9]}


def _torch():
    import torch
    import graphdot_amd.model.alignment  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


def _rows(m, pick):
    """Where the sums of the planes `pick` lie in the definition's 2 + 2 m."""
    pick = np.asarray(pick, dtype=np.int64)
    return np.concatenate(([0, 1], 2 + pick, 2 + m + pick))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', SIZES)
def test_fused_against_the_definition(n, dtype):
    from graphdot_amd.model.alignment import _align
    torch = _torch()
    share = 0.0
    for m in PLANES:
        for k in COLUMNS:
            K, P, T = cpu.inputs(n, m, k)
            want, bound, _, _ = cpu.definition(n, m, k, dtype)
            Tc = _t(cpu.centred(T)).cuda()
            lists = [np.arange(m)] + ([PICKS[m]] if m in PICKS else [])
            for layout in ('row-major', 'column-major'):
                Kd = cpu.matrix(K, dtype, layout).cuda()
                assert Kd.stride() == cpu.matrix(K, dtype, layout).stride()
                for axis in range(3 if m else 1):
                    Pd = cpu.planes_along(P, dtype, axis).cuda()
                    for pick in lists:
                        a, b = (_align.alignment(Kd, Tc, Pd, pick)
                                for _ in range(2))
                        assert a.is_cuda and a.dtype == torch.float64
                        assert torch.equal(a, b), (m, k, layout, axis)
                        got, rows = a.cpu().numpy(), _rows(m, pick)
                        assert got.shape == rows.shape
                        share = max(share, cpu.worst(got, want[rows],
                                                     bound[rows]))
                        assert np.all(np.abs(got - want[rows])
                                      <= bound[rows]), (m, k, layout, axis)
    print(f'n {n} {np.dtype(dtype).name}: the sums are off by at most '
          f'{share:.3g} of their bounds')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [3, 65, 257])
def test_fused_against_the_restatement(n, dtype):
    """Both chains on the same device tensors: each within the bound of the
    definition, so within twice the bound of each other."""
    from graphdot_amd.model.alignment import _align
    share = 0.0
    for m in PLANES:
        for k in COLUMNS:
            K, P, T = cpu.inputs(n, m, k)
            want, bound, _, _ = cpu.definition(n, m, k, dtype)
            Tc = _t(cpu.centred(T)).cuda()
            Kd = cpu.matrix(K, dtype, 'column-major').cuda()
            Pd = cpu.planes_along(P, dtype, 0).cuda()
            fused, said = _align.solve(Kd, Tc, Pd, np.arange(m))
            assert said is True
            restated = _align.alignment_torch(Kd, Tc, Pd, np.arange(m))
            assert restated.is_cuda
            fused, restated = fused.cpu().numpy(), restated.cpu().numpy()
            share = max(share, cpu.worst(restated, want, bound))
            assert np.all(np.abs(restated - want) <= bound), (m, k)
            assert np.all(np.abs(fused - restated) <= 2 * bound), (m, k)
    print(f'n {n} {np.dtype(dtype).name}: the restatement on the device is '
          f'off by at most {share:.3g} of the bounds')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_seventeen_columns_take_the_torch_chain(dtype):
    from graphdot_amd.model.alignment import _align
    n, m, k = 65, 3, 17
    K, P, T = cpu.inputs(n, m, k)
    want, bound, _, _ = cpu.definition(n, m, k, dtype)
    Tc = _t(cpu.centred(T)).cuda()
    Kd = cpu.matrix(K, dtype, 'row-major').cuda()
    Pd = cpu.planes_along(P, dtype, 0).cuda()
    got, fused = _align.solve(Kd, Tc, Pd, np.arange(m))
    assert fused is False and got.is_cuda
    assert np.all(np.abs(got.cpu().numpy() - want) <= bound)
    with pytest.raises(TypeError, match='KMAX'):
        _align.alignment(Kd, Tc, Pd, np.arange(m))
    assert _align.solve(Kd, Tc[:, :16].contiguous(), Pd, np.arange(m))[1] \
        is True


def test_launches_check_their_arguments():
    from graphdot_amd.model.alignment import _align
    torch = _torch()
    n = 8
    K = torch.eye(n, dtype=torch.float64, device='cuda')
    Tc = _t(cpu.centred(np.eye(2)[np.arange(n) % 2])).cuda()
    P = torch.zeros((n, n, 2), dtype=torch.float64, device='cuda')
    with pytest.raises(TypeError, match='CUDA'):
        _align.alignment(K.cpu(), Tc)
    with pytest.raises(TypeError, match='K'):
        _align.alignment(K[:, :4], Tc)
    with pytest.raises(TypeError, match='Tc'):
        _align.alignment(K, Tc.float())
    with pytest.raises(TypeError, match='Tc'):
        _align.alignment(K, Tc[:4])
    with pytest.raises(TypeError, match='P'):
        _align.alignment(K, Tc, P.cpu(), [0])
    with pytest.raises(TypeError, match='type of K'):
        _align.alignment(K, Tc, P.float(), [0])
    with pytest.raises(ValueError, match='out of range'):
        _align.alignment(K, Tc, P, [0, 2])
    # planes of another type take the torch chain; targets from the host and
    # a strided matrix are read as they are
    assert _align.solve(K, Tc, P.float(), [0])[1] is False
    big = torch.zeros((2 * n, 2 * n), dtype=torch.float64, device='cuda')
    big[::2, ::2] = K
    assert torch.equal(_align.alignment(big[::2, ::2], Tc.cpu(), P, [1, 0]),
                       _align.alignment(K, Tc, P, [1, 0]))
    out = _align.alignment(K, Tc, P, [1, 0]).cpu().numpy()
    # K_c = I - 11^T / n, w_ij = +-1/2: a = trace w = n / 2, b = n - 1
    assert out.tolist() == [n / 2, n - 1, 0, 0, 0, 0]


# -- the model on QM7-like graphs -----------------------------------------------------
N_GRAPHS = 12


def _graphs():
    import cases
    G = np.asarray(list(cases.config3_graphs(N_GRAPHS, seed=23)), dtype=object)
    size = np.array([float(len(g.nodes)) for g in G])
    return G, (size > np.median(size)).astype(int), size


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


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('transform', ['plain', 'normalized'])
def test_model_on_the_device_path(real, transform, monkeypatch):
    """The model's sums against the definition on the very tensors it handed
    to the launches (downloaded here, for the test), and its alignment and
    gradient against the formulas on the definition's sums.  With the sums
    within ``da, db, dg, dh`` of the definition's and ``N = sqrt(b) ||L_c||``,
    to first order ``|dA| <= da / N + |A| db / (2 b)`` and ``|d grad_p| <=
    dg_p / N + |g_p| db / (2 b N) + (|h_p| da + |a| dh_p) / (b N) + 3 |a h_p|
    db / (2 b^2 N)``; the test allows twice that for the higher orders and
    the roundings of the quotients themselves, times ``exp(theta)`` for the
    gradient."""
    from graphdot_amd.model.alignment import KernelTargetAlignment, _align
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G, lab, size = _graphs()
    kernel = _kernel(real, transform)
    theta0 = np.array(kernel.theta)
    loose = 1e-3 if real is np.float32 else 1e-8
    seen, calls = [], []
    solve = _align.solve

    def recording(K, Tc, P=None, planes=()):
        out, fused = solve(K, Tc, P, planes)
        seen.append((K.to(torch.float64).cpu().numpy(), K.dtype,
                     None if P is None else P[:, :, torch.as_tensor(
                         planes, device=P.device)].to(torch.float64).cpu()
                     .numpy(), out.cpu().numpy()))
        return out, fused

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    monkeypatch.setattr(_align, 'solve', recording)
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
        monkeypatch.setattr(cls, 'diag', counting)
    for y in (lab, size):
        kta = KernelTargetAlignment(kernel, device='cuda')
        A, grad = kta.alignment(theta0, X=G, y=y, eval_gradient=True)
        assert kta.last_timing['adopted'] is True
        assert kta.last_timing['fused'] is True
        K, stored_as, P, sums = seen[-1]
        m = len(theta0)
        assert P.shape == (N_GRAPHS, N_GRAPHS, m) and sums.shape == (2 + 2 * m,)
        assert stored_as == (torch.float64 if transform == 'normalized'
                             or real is np.float64 else torch.float32)
        T = np.eye(2)[y] if y is lab else y[:, None]
        want, bound, A_def, dA_def = cpu.define(K, P, T)
        print(f'{real.__name__} {transform}: A {A:.6g}, the sums are off by '
              f'at most {cpu.worst(sums, want, bound):.3g} of their bounds')
        assert np.all(np.abs(sums - want) <= bound)
        a, b, g, h = want[0], want[1], want[2:2 + m], want[2 + m:]
        da, db, dg, dh = bound[0], bound[1], bound[2:2 + m], bound[2 + m:]
        Tc = cpu.centred(T)
        N = np.sqrt(b) * np.linalg.norm(Tc.T @ Tc)
        assert abs(A - A_def) <= 2 * (da / N + abs(A_def) * db / (2 * b))
        dgrad = dg / N + np.abs(g) * db / (2 * b * N) \
            + (np.abs(h) * da + abs(a) * dh) / (b * N) \
            + 3 * np.abs(a * h) * db / (2 * b * b * N)
        assert np.all(np.abs(grad - dA_def * np.exp(theta0))
                      <= 2 * dgrad * np.exp(theta0))
        # (the value alone comes from the value solver, which stops at its
        # own ftol: 1e-13 in double, 1e-8 in float)
        assert kta.alignment(theta0, X=G, y=y) == pytest.approx(A, rel=loose)
    # a short fit does not lower the alignment and leaves the kernel alone
    kta = KernelTargetAlignment(kernel, optimizer=True, device='cuda')
    start = kta.alignment(X=G, y=lab)
    kta.fit(G, lab, tol=1e-3)
    print(f'alignment {start:.6g} -> {kta.alignment_:.6g} in '
          f'{kta.optimization_result.nfev} evaluations')
    assert kta.alignment_ >= start
    assert kta.last_timing['adopted'] is True
    assert kta.last_timing['fused'] is True
    assert np.array_equal(kernel.theta, theta0)
    lo, hi = np.asarray(kernel.bounds).T
    assert np.all(kta.theta_ >= lo) and np.all(kta.theta_ <= hi)
    # (theta goes through exp and log on its way into a clone)
    assert kta.score(G[:8], lab[:8]) == pytest.approx(KernelTargetAlignment(
        kta.kernel_, device='cuda').alignment(X=G[:8], y=lab[:8]), rel=loose)
    assert calls == []


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_entries_that_are_not_finite(bad):
    from graphdot_amd.model.alignment import KernelTargetAlignment
    n = 65
    K, _, lab, _ = cpu.svc.data(n, cpu.GAMMA)
    good = KernelTargetAlignment('precomputed', device='cuda')
    A = good.fit(_t(K).cuda(), lab).alignment_
    assert good.last_timing['fused'] is True
    assert A == pytest.approx(cpu.definition(n, 0, 2)[2], rel=1e-12)
    Kb = K.copy()
    Kb[40, 3] = Kb[3, 40] = bad
    with pytest.raises(ValueError, match='not finite'):
        KernelTargetAlignment('precomputed', device='cuda').fit(
            _t(Kb).cuda(), lab)
