"""KernelPCA without a GPU: the blocked subspace iteration on its torch
restatements and the dense solver against ``numpy.linalg.eigh`` of the
explicitly centred matrix, `transform`, the explained variance, the fallback
for a flat spectrum, the dropped components of a rank-deficient matrix, the
argument checks, precomputed input as numpy and torch, and a graph kernel
without a device path.

The test matrices are ``case(n, seed, decay)``: ``K = Q diag(max(decay^i,
1e-6)) Q^T`` with Q from the QR factorisation of a normal (n, n) matrix.  With
``decay = 0.7`` neighbouring eigenvalues of the centred matrix are a ratio near
0.7 apart, the iteration contracts by about ``0.7^8 = 0.058`` per step (the
block is at least 8 wider than k) and meets ``tol = 1e-10`` after about 8
steps: 20 is the cap that a broken iteration does not pass by brute force."""
import warnings
import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
SIZES = [2, 3, 17, 63, 64, 65, 257, 1000]
COMPONENTS = [1, 2, 4, 16]
NK = [(n, k) for n in SIZES for k in COMPONENTS if k < n]


def case(n, seed, decay):
    Q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(n, n)))
    K = (Q * np.maximum(decay ** np.arange(n), 1e-6)) @ Q.T
    return 0.5 * (K + K.T)


def centred(K):
    n = len(K)
    H = np.eye(n) - 1.0 / n
    Kc = H @ K @ H
    return 0.5 * (Kc + Kc.T)


_reference = {}


def reference(n, decay=0.7):
    """(K, Kc, eigenvalues descending, eigenvectors) -- computed once."""
    if (n, decay) not in _reference:
        K = case(n, n, decay)
        Kc = centred(K)
        w, V = np.linalg.eigh(Kc)
        _reference[n, decay] = (K, Kc, w[::-1], V[:, ::-1])
    return _reference[n, decay]


def signed(V):
    lead = np.argmax(np.abs(V), axis=0)
    return V * np.where(V[lead, np.arange(V.shape[1])] < 0, -1.0, 1.0)


def model(k, solver, **kwargs):
    from graphdot_amd.model.decomposition import KernelPCA
    return KernelPCA('precomputed', k, eigen_solver=solver, device='cpu',
                     **kwargs)


def check_eigenpairs(pca, n, k):
    """The assertions the CPU and the GPU test of the whole fit share."""
    K, Kc, w, V = reference(n)
    assert pca.n_components_ == k
    assert pca.eigenvalues_.shape == (k,) and \
        pca.eigenvectors_.shape == (n, k)
    err = np.abs(pca.eigenvalues_ - w[:k]).max() / w[0]
    print(f'n {n} k {k}: eigenvalues within {err:.3g} (bound '
          f'{8 * n * EPS:.3g}), iterations {pca.n_iter_}')
    assert err <= 8 * n * EPS
    U = pca.eigenvectors_
    assert np.abs(U.T @ U - np.eye(k)).max() <= 8 * n * EPS
    ref = signed(V[:, :k])
    for j in range(k):
        # sin(angle) <= residual / gap for either vector against the exact
        # one (Davis-Kahan), and |u - v| <= 2 sin for unit vectors of one
        # sign; the reference's vector has a residual of its own, and two
        # unit vectors are each normalised to a few eps only
        gap = np.abs(np.delete(w, j) - w[j]).min()
        res = np.linalg.norm(Kc @ U[:, j] - pca.eigenvalues_[j] * U[:, j])
        res_ref = np.linalg.norm(Kc @ ref[:, j] - w[j] * ref[:, j])
        assert np.linalg.norm(U[:, j] - ref[:, j]) \
            <= 2 * (res + res_ref) / gap + 4 * EPS, (j, res, res_ref, gap)
        assert U[np.argmax(np.abs(U[:, j])), j] > 0


@pytest.mark.parametrize('n,k', NK)
def test_subspace_against_numpy(n, k):
    K = reference(n)[0]
    pca = model(k, 'subspace')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        pca.fit(K)
    assert pca.eigen_solver_ == 'subspace'          # converged: no fallback
    assert 1 <= pca.n_iter_ <= 20
    assert np.all(pca.residuals_ <= 1e-10 * pca.eigenvalues_[0])
    check_eigenpairs(pca, n, k)


@pytest.mark.parametrize('n,k', [(3, 2), (65, 4), (257, 16)])
def test_dense_and_subspace_agree(n, k):
    K, Kc, w, _ = reference(n)
    Ks = case(n + 5, 3 * n, 0.7)[:5, :n] if n > 3 else K[:2] + 0.25
    out = []
    for solver in ('dense', 'subspace'):
        pca = model(k, solver)
        xy = pca.fit_transform(K)
        assert pca.eigen_solver_ == solver
        check_eigenpairs(pca, n, k)
        out.append((xy, pca.transform(Ks), pca))
    # each side is within 2 res / gap of the reference's vectors; the
    # coordinates carry sqrt(w) and 1 / sqrt(w)
    gap = np.array([np.abs(np.delete(w, j) - w[j]).min() for j in range(k)])
    res = sum(np.linalg.norm(Kc @ p.eigenvectors_ - p.eigenvalues_
                             * p.eigenvectors_, axis=0) for *_, p in out)
    tol_v = 2 * res / gap + 8 * n * EPS
    (xa, ta, _), (xb, tb, _) = out
    assert np.all(np.abs(xa - xb).max(0) <= tol_v * np.sqrt(w[:k])
                  + 8 * n * EPS * np.sqrt(w[0]))
    rows = np.linalg.norm(centred_cross(Ks, K), axis=1).max()
    assert np.all(np.abs(ta - tb).max(0)
                  <= (tol_v + 8 * n * EPS * w[0] / w[:k]) * rows
                  / np.sqrt(w[:k]))


def centred_cross(Ks, K):
    return Ks - Ks.mean(1, keepdims=True) - K.mean(0) + K.mean()


@pytest.mark.parametrize('solver', ['dense', 'subspace'])
def test_transform_reproduces_fit_transform(solver):
    n, k = 65, 4
    K, _, w, _ = reference(n)
    pca = model(k, solver)
    xy = pca.fit_transform(K)
    again = pca.transform(K)
    # Kc v / sqrt(w) = sqrt(w) v up to the residual and n eps |Kc|
    assert np.all(np.abs(again - xy).max(0)
                  <= (8 * n * EPS * w[0] + 1e-10 * w[0]) / np.sqrt(w[:k]))


def test_explained_variance_ratio():
    n, k = 64, 4
    K, Kc, w, _ = reference(n)
    pca = model(k, 'subspace').fit(K)
    trace = np.trace(K) - K.sum() / n
    np.testing.assert_allclose(pca.explained_variance_ratio_,
                               pca.eigenvalues_ / trace, rtol=8 * n * EPS)
    np.testing.assert_allclose(pca.explained_variance_ratio_,
                               w[:k] / w.sum(), rtol=64 * n * EPS)
    assert pca.explained_variance_ratio_.sum() <= 1
    full = model(16, 'dense').fit(reference(17)[0])
    assert full.explained_variance_ratio_.sum() <= 1 + 8 * 17 * EPS


def test_flat_spectrum_falls_back_to_dense():
    n, k = 257, 4
    K = case(n, n, 0.999)
    dense = model(k, 'dense')
    want = dense.fit_transform(K)
    pca = model(k, 'subspace')
    with pytest.warns(UserWarning, match='worst residual'):
        got = pca.fit_transform(K)
    assert pca.eigen_solver_ == 'dense' and pca.n_iter_ == 100
    assert np.array_equal(got, want)
    assert np.array_equal(pca.eigenvalues_, dense.eigenvalues_)


def test_rank_deficient_matrix_drops_components():
    rng = np.random.default_rng(5)
    B = rng.normal(size=(7, 7))
    K = B @ B.T
    K = np.vstack((K, K[2]))                     # a duplicated row and column
    K = np.column_stack((K, K[:, 2]))
    n = len(K)                                   # Kc has rank n - 2 = 6
    pca = model(7, 'dense')
    with pytest.warns(UserWarning, match='dropped'):
        xy = pca.fit_transform(K)
    assert pca.n_components_ == 6 and xy.shape == (n, 6)
    assert pca.eigenvalues_.shape == (6,) and pca.eigenvectors_.shape == (n, 6)
    w = np.linalg.eigvalsh(centred(K))[::-1]
    np.testing.assert_allclose(pca.eigenvalues_, w[:6], rtol=0,
                               atol=8 * n * EPS * w[0])
    assert pca.transform(K[:3]).shape == (3, 6)
    np.testing.assert_allclose(xy[2], xy[n - 1], rtol=0,
                               atol=1e-6 * np.abs(xy).max())


def test_value_errors():
    from graphdot_amd.model.decomposition import KernelPCA
    K = reference(17)[0]
    for k in (0, 17, 1.5):
        with pytest.raises(ValueError):
            KernelPCA('precomputed', k)
    with pytest.raises(ValueError):
        KernelPCA('precomputed', 2, eigen_solver='lanczos')
    with pytest.raises(ValueError):
        model(16, 'dense').fit(K[:16, :16])      # k = n: beyond the rank
    with pytest.raises(ValueError):
        model(2, 'dense').fit(K[:2, :2])
    with pytest.raises(ValueError):
        model(2, 'dense').fit(K[:5])             # not square
    pca = model(2, 'dense').fit(K)
    with pytest.raises(ValueError):
        pca.transform(K[:, :5])
    with pytest.raises(ValueError):
        model(2, 'subspace').fit(K, v0=np.ones((17, 40)))
    with pytest.raises(RuntimeError):
        model(2, 'dense').transform(K)
    assert model(1, 'dense').fit(K[:2, :2]).n_components_ == 1


@pytest.mark.parametrize('solver', ['dense', 'subspace'])
def test_precomputed_accepts_numpy_and_torch(solver):
    import torch
    n, k = 63, 2
    K = reference(n)[0]
    want = model(k, solver).fit(K)
    for given in (torch.from_numpy(K.copy()), K.astype(np.float32),
                  torch.from_numpy(K.astype(np.float32)),
                  torch.from_numpy(K.copy()).t()):
        pca = model(k, solver)
        xy = pca.fit_transform(given)
        single = not torch.is_tensor(given) and given.dtype == np.float32 \
            or torch.is_tensor(given) and given.dtype == torch.float32
        # (a float matrix is another matrix: its eigenvalues move by its
        # rounding, |dK|_2 <= n eps32 |K|_max / 2)
        tol = n * np.finfo(np.float32).eps if single else 8 * n * EPS
        np.testing.assert_allclose(pca.eigenvalues_, want.eigenvalues_,
                                   rtol=0, atol=tol * want.eigenvalues_[0])
        assert xy.dtype == np.float64 and xy.shape == (n, k)
        rows = given[:3]
        assert pca.transform(rows).shape == (3, k)


def test_repeats_are_identical():
    K = reference(65)[0]
    a = model(4, 'subspace', random_state=3).fit_transform(K)
    b = model(4, 'subspace', random_state=3).fit_transform(K)
    assert np.array_equal(a, b)


def test_a_block_with_equal_columns_falls_back():
    """V^T V of a start block with two equal columns is singular: the Ritz
    step reports it and the fit finishes with 'dense'."""
    n, k = 17, 2
    K = reference(n)[0]
    from graphdot_amd.model.decomposition import _subspace
    m = _subspace.block_width(n, k)
    v0 = np.random.default_rng(1).normal(size=(n, m))
    v0[:, 3] = v0[:, 1]
    pca = model(k, 'subspace')
    with pytest.warns(UserWarning, match='not positive definite'):
        got = pca.fit_transform(K, v0=v0)
    assert pca.eigen_solver_ == 'dense'
    assert pca.n_iter_ == _subspace.CHECK_EVERY
    assert np.array_equal(got, model(k, 'dense').fit_transform(K))


def test_block_width_and_cadence():
    from graphdot_amd.model.decomposition import _subspace
    for n in SIZES:
        for k in COMPONENTS:
            if k < n:
                m = _subspace.block_width(n, k)
                assert k <= m <= min(32, n - 1)
                assert m == min(n - 1, max(2 * k, k + 8))
    assert _subspace.CHECK_EVERY == 4


def test_graph_kernel_without_a_device_path():
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.model.decomposition import KernelPCA
    G = np.asarray(cases.config3_graphs(12, seed=3), dtype=object)
    knode, kedge, q = cases.config3_kernels()
    mgk = MarginalizedGraphKernel(knode, kedge, q=q, backend=OracleBackend())
    # (the oracle backend solves pairs only: the self-similarities of Z as
    # the diagonal of its Gram matrix)
    mgk.diag = lambda Z: mgk(Z).diagonal()
    X, Z = G[:9], G[9:]
    n, k = len(X), 2
    for kernel in (mgk, Normalization(mgk)):
        K = np.asarray(kernel(X), dtype=np.float64)
        Ks = np.asarray(kernel(Z, X), dtype=np.float64)
        w, V = np.linalg.eigh(centred(K))
        w, V = w[::-1][:k], signed(V[:, ::-1][:, :k])
        for solver in ('auto', 'subspace'):
            pca = KernelPCA(kernel, k, eigen_solver=solver, device='cpu')
            xy = pca.fit_transform(X)
            assert pca.last_timing['adopted'] is False
            assert pca.eigen_solver_ == ('dense' if solver == 'auto'
                                         else 'subspace')
            gap = min(w[0] - w[1], w[1] - np.linalg.eigvalsh(
                centred(K))[::-1][2])
            tol = 1e-10 * w[0] / gap + 64 * n * EPS * w[0] / gap
            np.testing.assert_allclose(pca.eigenvalues_, w, rtol=0,
                                       atol=8 * n * EPS * w[0])
            np.testing.assert_allclose(xy, V * np.sqrt(w), rtol=0,
                                       atol=tol * np.sqrt(w[0]))
            np.testing.assert_allclose(
                pca.transform(Z), centred_cross(Ks, K) @ (V / np.sqrt(w)),
                rtol=0, atol=tol * np.abs(Ks).max() * np.sqrt(n / w[k - 1]))
