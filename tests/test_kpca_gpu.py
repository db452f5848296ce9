"""The device path of KernelPCA on an MI355X: every launch of subspace.hip
against its torch restatement (run in double on the CPU) on the same stored
inputs (tile and wave edges, every register chunk and the two-pass block, f32 /
f64 matrices in both layouts, bit-identical repeats), the Ritz kernel on the
defining properties of its outputs, the whole fit against ``numpy.linalg.eigh``
with the assertions and matrices of test_kpca.py, its fallbacks, and the model
on the HIP backend against the same model forced to its host path, with no
host kernel evaluation and no n x n download on the device path.

The margins of device against host are ten times the largest differences
measured on an MI355X, relative to the largest host magnitude of the quantity,
over the four kernels (float / double, plain / normalised): see the constants,
which carry the measured figures."""
import warnings
import numpy as np
import pytest

import test_kpca as cpu

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SIZES = [2, 3, 63, 64, 65, 257, 1000]
WIDTHS = [1, 2, 9, 12, 16, 32]
#: (the block is never wider than n - 1: n = 2 and 3 take the widths they can)
NM = [(n, m) for n in SIZES for m in WIDTHS if m <= n - 1]


def _torch():
    import torch
    import graphdot_amd.model.decomposition  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


def _matrix(K, dtype, layout):
    """K stored as `dtype`, contiguous along the index `layout` names; the
    values both sides then work on."""
    A = _t(K.astype(dtype))
    return A.t().contiguous().t() if layout == 'column-major' else A


_blocks = {}


def _block(n, m):
    """(K, V, vpart) -- computed once: a matrix that is far from centred (its
    mean is of the size of its entries) and a block that is neither centred
    nor normalised, with statistics in three partial blocks."""
    if (n, m) not in _blocks:
        rng = np.random.default_rng(1000 * n + m)
        K = cpu.case(n, n, 0.7) + 0.5
        V = rng.normal(size=(n, m)) * rng.uniform(0.5, 3.0, size=m) + 0.3
        sq, sm = (V * V).sum(0), V.sum(0)
        share = np.array([0.5, 0.25, 0.25])
        vpart = np.concatenate((sq[:, None] * share, sm[:, None] * share))
        _blocks[n, m] = (K, V, vpart)
    return _blocks[n, m]


def _twice(fn, *args):
    torch = _torch()
    a, b = fn(*args), fn(*args)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)                  # bit-identical repeats
    return [x.cpu().numpy() for x in a]


# -- the launches against their restatements ------------------------------------------
@pytest.mark.parametrize('layout', ['row-major', 'column-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n,m', NM)
def test_apply_against_restatement(n, m, dtype, layout):
    """Both sides work in double on the same stored values.  An entry of
    the centred block ``u = V s - vmean`` carries 4 eps of ``|V s| +
    |vmean|`` on either side (the scale's sum of squares, root and quotient,
    the mean's sum and quotient, relative, with n eps for the sums: ``(n +
    4) eps``), and either side's sum of n products differs from the exact one
    by ``(n - 1) eps sum |terms|`` whatever its order.  Two sides: ``Z``
    within ``c (n + c') eps |K| (|V s| + |vmean|)`` with c = 4, c' = 4.  The
    products ``V^T V`` and ``V^T Z`` add one more sum of n terms over
    inputs that carry the errors above: c = 8, the same c'; ``1^T Z``
    likewise."""
    from graphdot_amd.model.decomposition import _subspace
    K, V, vpart = _block(n, m)
    Kt = _matrix(K, dtype, layout)
    assert n == 1 or Kt.stride(0 if layout == 'column-major' else 1) == 1
    stored = Kt.to(_torch().float64).numpy()
    rZ, rpart = (x.numpy() for x in _subspace.apply_torch(
        _t(stored), _t(V), _t(vpart)))
    Z, part = _twice(_subspace.apply, Kt.cuda(), _t(V).cuda(),
                     _t(vpart).cuda())
    assert Z.shape == (n, m) and part.shape == (-(-n // 16), 2 * m * m + m)
    scale, vsum = (x.numpy() for x in _subspace.col_stats_torch(_t(vpart), m))
    Vs = np.abs(V * scale)
    u = Vs + np.abs(vsum / n)
    c4, c8 = 4 * (n + 4) * EPS, 8 * (n + 4) * EPS
    size_Z = np.abs(stored) @ u
    assert np.all(np.abs(Z - rZ) <= c4 * size_Z)
    mm = m * m
    tot, rtot = part.sum(0), rpart[0]
    assert np.all(np.abs(tot[:mm] - rtot[:mm]).reshape(m, m)
                  <= c8 * (Vs.T @ Vs))
    assert np.all(np.abs(tot[mm:2 * mm] - rtot[mm:2 * mm]).reshape(m, m)
                  <= c8 * (Vs.T @ size_Z))
    assert np.all(np.abs(tot[2 * mm:] - rtot[2 * mm:]) <= c8 * size_Z.sum(0))


@pytest.mark.parametrize('n,m', NM)
def test_ritz_properties(n, m):
    """``R^T S R = I`` and ``R^T G R = diag(w)`` with w descending, for S
    and G as numpy forms them from the partial sums the kernel was given.
    The factorisation, the two triangular solves, the Jacobi sweeps (which
    stop at ``off(T) <= eps |T|_F``) and the back substitution are each
    backward stable with a constant of a few m: ``c m eps`` of ``|R|^2 |S|``
    (of ``|R|^2 |G|``), c = 16."""
    from graphdot_amd.model.decomposition import _subspace
    K, V, vpart = _block(n, m)
    Z, part = _subspace.apply_torch(_t(K), _t(V), _t(vpart))
    # (three row blocks, as the apply leaves them)
    part = (part * _t(np.array([0.5, 0.25, 0.25]))[:, None]).contiguous()
    R, info, cols = _twice(_subspace.ritz, part.cuda(), _t(vpart).cuda(),
                           n, m)
    assert info[2 * m] == 0
    w = info[:m]
    assert np.all(np.diff(w) <= 0)
    mm = m * m
    tot = part.sum(0).numpy()
    scale, vsum = (x.numpy() for x in _subspace.col_stats_torch(_t(vpart), m))
    S = tot[:mm].reshape(m, m)
    zmean = tot[2 * mm:] / n
    G = tot[mm:2 * mm].reshape(m, m) - np.outer(vsum, zmean)
    G = 0.5 * (G + G.T)
    np.testing.assert_allclose(cols, np.concatenate((scale, vsum, zmean)),
                               rtol=8 * EPS, atol=0)
    c = 16 * m * EPS
    nR = np.linalg.norm(R, 2) ** 2
    assert np.abs(R.T @ S @ R - np.eye(m)).max() \
        <= c * nR * np.linalg.norm(S, 2)
    assert np.abs(R.T @ G @ R - np.diag(w)).max() \
        <= c * nR * np.linalg.norm(G, 2)
    # and the values are those of the restatement's pencil
    rw = _subspace.ritz_torch(part, _t(vpart), n, m)[1][:m].numpy()
    assert np.abs(w - rw).max() <= c * nR * np.linalg.norm(G, 2)


@pytest.mark.parametrize('n,m', NM)
def test_rotate_against_restatement(n, m):
    """``Vr = (V s) R`` and ``Yr = (Z - zmean) R`` are sums of m products
    (``2 (m + 2) eps`` of their terms over both sides, the scaling and the
    centring included); the column sums over n rows add ``(n - 1) eps`` per
    side on inputs that carry the above: ``c (n + c') eps sum |terms|`` with
    c = 4 and c' = m + 4, twice that for the squares."""
    from graphdot_amd.model.decomposition import _subspace
    K, V, vpart = _block(n, m)
    Z, part = _subspace.apply_torch(_t(K), _t(V), _t(vpart))
    R, info, cols = _subspace.ritz_torch(part, _t(vpart), n, m)
    args = (_t(V), Z, R, info, cols)
    rVr, rY, rp = (x.numpy() for x in _subspace.rotate_torch(*args))
    Vr, Y, rpart = _twice(_subspace.rotate, *(x.cuda() for x in args))
    nb = -(-n // 64)
    assert rpart.shape == (3 * m, nb)
    aR = np.abs(R.numpy())
    aV = np.abs(V * cols[:m].numpy()) @ aR
    aY = (np.abs(Z.numpy()) + np.abs(cols[2 * m:].numpy())) @ aR
    cm = 2 * (m + 2) * EPS
    assert np.all(np.abs(Vr - rVr) <= cm * aV)
    assert np.all(np.abs(Y - rY) <= cm * aY)
    c = 4 * (n + m + 4) * EPS
    got = rpart.sum(1)
    aD = aY + np.abs(info[:m].numpy()) * aV
    assert np.all(np.abs(got[:m] - rp[:m, 0]) <= 2 * c * (aY * aY).sum(0))
    assert np.all(np.abs(got[m:2 * m] - rp[m:2 * m, 0]) <= c * aY.sum(0))
    assert np.all(np.abs(got[2 * m:] - rp[2 * m:, 0])
                  <= 2 * c * (aD * aD).sum(0))
    # the residual norms: the second stage on the device
    dev = _torch().zeros(2 * m + 1, dtype=_torch().float64, device='cuda')
    res, = _twice(lambda p: (_subspace.residuals(p, dev).clone(),),
                  _t(rpart).cuda())
    assert np.all(np.abs(res[m:2 * m] - rp[2 * m:, 0])
                  <= 2 * c * (aD * aD).sum(0))


@pytest.mark.parametrize('layout', ['row-major', 'column-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', SIZES)
def test_sums_against_restatement(n, dtype, layout):
    from graphdot_amd.model.decomposition import _subspace
    Kt = _matrix(_block(n, 1)[0], dtype, layout)
    rc, rt = (x.numpy() for x in _subspace.sums_torch(Kt))
    colsum, tot = _twice(_subspace.sums, Kt.cuda())
    a = np.abs(Kt.to(_torch().float64).numpy())
    c = 2 * n * EPS
    assert np.all(np.abs(colsum - rc) <= c * a.sum(0))
    assert abs(tot[0] - rt[0]) <= 2 * c * a.sum()
    assert abs(tot[1] - rt[1]) <= c * np.trace(a)


@pytest.mark.parametrize('layout', ['column-major', 'row-major'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('k', [1, 2, 16])
@pytest.mark.parametrize('b', [1, 5, 64, 65])
def test_project_against_restatement(b, k, dtype, layout):
    """``out = sum_i (Ks - colmean)_ci A_il - (rowmean_c - gmean) sum_i
    A_il``: three sums of n terms per side, on differences that carry an
    eps of their two terms: ``4 (n + 4) eps`` of ``(|Ks| + |colmean|) |A| +
    (|rowmean| + |gmean|) 1^T |A|``."""
    from graphdot_amd.model.decomposition import _subspace
    n = 257
    rng = np.random.default_rng(100 * b + k)
    Ks = rng.normal(size=(b, n)) + 0.7
    A = rng.normal(size=(n, k)) + 0.2          # (columns do not sum to zero)
    colmean = rng.normal(size=n) + 0.5
    gmean = 0.45
    Kt = _t(Ks.astype(dtype))
    if layout == 'column-major':               # c + i b, as the solver leaves it
        Kt = Kt.t().contiguous().t()
    stored = Kt.to(_torch().float64).numpy()
    ref = _subspace.project_torch(_t(stored), _t(A), _t(colmean),
                                  gmean).numpy()
    out, = _twice(lambda *a: (_subspace.project(*a),), Kt.cuda(),
                  _t(A).cuda(), _t(colmean).cuda(), gmean)
    assert out.shape == ref.shape == (b, k)
    aA = np.abs(A)
    size = (np.abs(stored) + np.abs(colmean)) @ aA + (
        np.abs(stored).mean(1, keepdims=True) + abs(gmean)) * aA.sum(0)
    assert np.all(np.abs(out - ref) <= 4 * (n + 4) * EPS * size)


def test_launches_check_their_arguments():
    torch = _torch()
    from graphdot_amd.model.decomposition import _subspace
    n, m = 8, 3
    K = torch.eye(n, dtype=torch.float64, device='cuda')
    V = torch.ones((n, m), dtype=torch.float64, device='cuda')
    vpart = torch.ones((2 * m, 1), dtype=torch.float64, device='cuda')
    with pytest.raises(TypeError):
        _subspace.apply(K.cpu(), V, vpart)
    with pytest.raises(TypeError):
        _subspace.apply(K.to(torch.float16), V, vpart)
    with pytest.raises(ValueError):
        _subspace.apply(K[:, ::2][:4], V[:4], vpart)      # strided
    with pytest.raises(ValueError):
        _subspace.apply(K, torch.ones((n, 33), dtype=torch.float64,
                                      device='cuda'), vpart)
    with pytest.raises(TypeError):
        _subspace.apply(K, V.to(torch.float32), vpart)
    with pytest.raises(ValueError):
        _subspace.apply(K, V, vpart[:m])
    with pytest.raises(ValueError):
        _subspace.project(K.cpu(), V, V[:, 0], 0.0)
    with pytest.raises(TypeError):
        _subspace.project(K, V, V[:, 0].cpu(), 0.0)
    empty = torch.zeros((0, n), dtype=torch.float64, device='cuda')
    assert _subspace.project(empty, V, V[:, 0].contiguous(), 0.0).shape \
        == (0, m)


# -- the whole fit ------------------------------------------------------------------
def _model(k, solver='subspace', **kwargs):
    from graphdot_amd.model.decomposition import KernelPCA
    return KernelPCA('precomputed', k, eigen_solver=solver, **kwargs)


@pytest.mark.parametrize('n,k', cpu.NK)
def test_subspace_fit_against_numpy(n, k):
    K = cpu.reference(n)[0]
    pca = _model(k)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        pca.fit(_t(K).cuda())
    assert pca.eigen_solver_ == 'subspace'
    assert 1 <= pca.n_iter_ <= 20
    assert np.all(pca.residuals_ <= 1e-10 * pca.eigenvalues_[0])
    cpu.check_eigenpairs(pca, n, k)


def test_auto_and_transform_on_the_device():
    n, k = 257, 4
    K, _, w, _ = cpu.reference(n)
    pca = _model(k, 'auto')
    xy = pca.fit_transform(_t(K.astype(np.float32)).cuda())
    assert pca.eigen_solver_ == 'subspace'
    again = pca.transform(_t(K.astype(np.float32)).cuda())
    assert np.all(np.abs(again - xy).max(0)
                  <= (8 * n * EPS * w[0] + 1e-10 * w[0]) / np.sqrt(w[:k]))
    host = cpu.model(k, 'dense').fit(K.astype(np.float32))
    np.testing.assert_allclose(pca.eigenvalues_, host.eigenvalues_, rtol=0,
                               atol=8 * n * EPS * w[0])


def test_flat_spectrum_falls_back_on_the_device():
    n, k = 257, 4
    K = _t(cpu.case(n, n, 0.999)).cuda()
    want = _model(k, 'dense').fit_transform(K)
    pca = _model(k)
    with pytest.warns(UserWarning, match='worst residual'):
        got = pca.fit_transform(K)
    assert pca.eigen_solver_ == 'dense' and pca.n_iter_ == 100
    assert np.array_equal(got, want)


def test_status_word_of_a_singular_block_is_honoured():
    """A start block with two equal columns: ``S = V^T V`` is singular, the
    Ritz kernel says so in its status word and the fit finishes with
    'dense'."""
    from graphdot_amd.model.decomposition import _subspace
    n, k = 65, 2
    K = cpu.reference(n)[0]
    m = _subspace.block_width(n, k)
    v0 = np.random.default_rng(1).normal(size=(n, m))
    v0[:, 3] = v0[:, 1]
    V, vpart = _subspace.start_block(n, m, v0=v0)
    Z, part = _subspace.apply(_t(K).cuda(), V.cuda(), vpart.cuda())
    R, info, _ = _subspace.ritz(part, vpart.cuda(), n, m)
    assert int(info[2 * m]) == 1 and bool(_torch().isnan(R).all())
    pca = _model(k)
    with pytest.warns(UserWarning, match='not positive definite'):
        got = pca.fit_transform(_t(K).cuda(), v0=v0)
    assert pca.eigen_solver_ == 'dense'
    assert pca.n_iter_ == _subspace.CHECK_EVERY
    assert np.array_equal(got, _model(k, 'dense').fit_transform(_t(K).cuda()))


# -- the model on QM7-like graphs ---------------------------------------------------
#: device against host, relative to the largest host magnitude of the
#: quantity: ten times the largest difference measured on an MI355X over the
#: four kernels.  The host path runs 'dense' and the
#: device path 'subspace' with tol = 1e-10: the coordinates carry the
#: iteration's residual over the gap, largest under `Normalization` (plain:
#: 1.2e-13 and 7.1e-15); the eigenvalues are second order in it.
RTOL_EIGENVALUES = 5.5e-15   # measured 5.53e-16 (double, plain)
RTOL_EMBEDDING = 3.8e-10     # measured 3.78e-11 (float and double, normalised)
RTOL_TRANSFORM = 6.3e-11     # measured 6.30e-12 (float and double, normalised)

N_TRAIN, N_HELD_OUT, K_GRAPHS = 40, 8, 3


def _graphs():
    import cases
    G = np.asarray(list(cases.config3_graphs(N_TRAIN + N_HELD_OUT, seed=29)),
                   dtype=object)
    return G[:N_TRAIN], G[N_TRAIN:]


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


def _close(triples):
    """Every (name, got, want, rtol): all figures are printed before the
    first is asserted."""
    errs = []
    for name, got, want, rtol in triples:
        got, want = np.asarray(got, float), np.asarray(want, float)
        assert got.shape == want.shape and np.all(np.isfinite(got))
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f'{name}: largest difference {err:.3g} of the largest '
              'magnitude')
        errs.append((name, err, rtol))
    for name, err, rtol in errs:
        assert err <= rtol, (name, err, rtol)


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('transform', ['plain', 'normalized'])
def test_device_matches_host(real, transform, monkeypatch):
    from graphdot_amd.model.decomposition import KernelPCA
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G, Z = _graphs()
    kernel = _kernel(real, transform)
    host = KernelPCA(kernel, K_GRAPHS, device='cpu')
    xy_h = host.fit_transform(G)
    t_h = host.transform(Z)
    assert host.last_timing['adopted'] is False
    # the device path: no host kernel evaluation, no n x n download
    calls, downloads = [], []

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
    to_host = torch.Tensor.cpu

    def cpu_counting(self, *args, **kwargs):
        if self.is_cuda and self.numel() >= N_TRAIN * N_TRAIN:
            downloads.append(tuple(self.shape))
        return to_host(self, *args, **kwargs)
    monkeypatch.setattr(torch.Tensor, 'cpu', cpu_counting)
    dev = KernelPCA(kernel, K_GRAPHS, device='cuda')
    xy_d = dev.fit_transform(G)
    t_d = dev.transform(Z)
    assert dev.last_timing['adopted'] is True
    assert calls == [] and downloads == []
    print(f'{real.__name__} {transform}: {dev.eigen_solver_}, '
          f'iterations {dev.n_iter_}, '
          f'eigenvalues {host.eigenvalues_}')
    _close((('eigenvalues', dev.eigenvalues_, host.eigenvalues_,
             RTOL_EIGENVALUES),
            ('fit_transform', xy_d, xy_h, RTOL_EMBEDDING),
            ('transform', t_d, t_h, RTOL_TRANSFORM)))
    assert t_d.shape == (N_HELD_OUT, K_GRAPHS)


class _HostOnly:
    """A kernel that offers the protocol's host methods alone."""

    def __init__(self, kernel):
        self.kernel = kernel

    def __call__(self, X, Y=None, **options):
        return self.kernel(X, Y, **options)


@pytest.mark.parametrize('how', ['no device_gram', 'kernel_options'])
def test_host_path_where_the_device_path_does_not_apply(how):
    from graphdot_amd.model.decomposition import KernelPCA
    G, Z = _graphs()
    kernel = _kernel(np.float64, 'normalized')
    dev = KernelPCA(kernel, K_GRAPHS, device='cuda')
    if how == 'no device_gram':
        other = KernelPCA(_HostOnly(kernel), K_GRAPHS, device='cuda')
    else:
        other = KernelPCA(kernel, K_GRAPHS, kernel_options={'lmin': 0},
                          device='cuda')
    out = []
    for m in (dev, other):
        xy = m.fit_transform(G)
        out.append((m.eigenvalues_, xy, m.transform(Z),
                    m.last_timing['adopted']))
    assert out[0][3] is True and out[1][3] is False
    _close((('eigenvalues', out[1][0], out[0][0], RTOL_EIGENVALUES),
            ('fit_transform', out[1][1], out[0][1], RTOL_EMBEDDING),
            ('transform', out[1][2], out[0][2], RTOL_TRANSFORM)))
