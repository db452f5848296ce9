"""The device side of the Nystrom regressor on the GPU: the cross-pair and
diagonal results of the marginalized graph kernel and its transformers left
on the device (`device_cross_gram`, `device_diag`, `LazyGradient`), the
gradient contraction of lowrank.hip, and LowRankApproximateGPR on graphs
with its algebra on the GPU against the same model on the CPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _backend(real):
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    return HIPBackend(real=np.float64) if real == 'f64' else HIPBackend()


def _graph_kernel(real='f64'):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    knode, kedge, _ = cases.config3_kernels()
    return MarginalizedGraphKernel(knode, kedge, q=0.05,
                                   backend=_backend(real))


def _kernel(kind, real):
    from graphdot_amd.kernel.fix import Normalization, Exponentiation
    k = _graph_kernel(real)
    return {'graph': lambda: k,
            'normalized': lambda: Normalization(k),
            'exponentiated': lambda: Exponentiation(k, xi=1.7),
            'normalized-exponentiated': lambda: Normalization(
                Exponentiation(k, xi=1.3)),
            'exponentiated-normalized': lambda: Exponentiation(
                Normalization(k), xi=2.1)}[kind]()


def _np(a):
    import torch
    from graphdot_amd.kernel.fix import LazyGradient
    if isinstance(a, LazyGradient):
        a = a.dense()
    return torch.as_tensor(a, device='cuda').double().cpu().numpy()


KINDS = ['graph', 'normalized', 'exponentiated', 'normalized-exponentiated',
         'exponentiated-normalized']


@pytest.mark.parametrize('real', ['f32', 'f64'])
@pytest.mark.parametrize('kind', KINDS)
def test_device_cross_gram_and_diag_match_the_host_calls(kind, real):
    import cases
    import torch
    G = cases.config3_graphs(29, seed=5)
    X, Y = G[:17], G[17:]
    kernel = _kernel(kind, real)
    tol = dict(rtol=2e-5, atol=1e-6) if real == 'f32' else \
        dict(rtol=1e-11, atol=1e-13)
    K, dK = kernel.device_cross_gram(X, Y, eval_gradient=True)
    Kh, dKh = kernel(X, Y, eval_gradient=True)
    assert tuple(K.shape) == (17, 12) and tuple(dK.shape)[:2] == (17, 12)
    np.testing.assert_allclose(_np(K), Kh, **tol)
    np.testing.assert_allclose(_np(dK), dKh, **tol)
    # (a value-only solve converges on its own: against the host's value-only
    # call)
    np.testing.assert_allclose(_np(kernel.device_cross_gram(X, Y)),
                               kernel(X, Y), **tol)
    # the contraction of the gradient, whatever form it comes in
    from graphdot_amd.kernel.fix import LazyGradient
    lazy = dK if isinstance(dK, LazyGradient) else LazyGradient(
        torch.as_tensor(dK, device='cuda'))
    W = torch.linspace(-1, 1, 17 * 12, dtype=torch.float64,
                       device='cuda').reshape(17, 12)
    np.testing.assert_allclose(lazy.contract(W).cpu().numpy(),
                               np.einsum('ic,ick->k', W.cpu().numpy(), dKh),
                               rtol=1e-9 if real == 'f64' else 1e-4,
                               atol=1e-9)
    rows = np.array([16, 0, 5, 5, 9])
    np.testing.assert_allclose(
        lazy.contract(W[:5], rows).cpu().numpy(),
        np.einsum('ic,ick->k', W[:5].cpu().numpy(), dKh[rows]),
        rtol=1e-9 if real == 'f64' else 1e-4, atol=1e-9)
    # the diagonal
    d, dd = kernel.device_diag(X, eval_gradient=True)
    if kind == 'graph':
        dh, ddh = kernel.diag(X, True, active_theta_only=False)
    else:
        dh, ddh = kernel.diag(X, True)
    np.testing.assert_allclose(_np(d), dh, **tol)
    np.testing.assert_allclose(_np(dd), ddh, **tol)
    np.testing.assert_allclose(_np(kernel.device_diag(X)), kernel.diag(X),
                               **tol)


@pytest.mark.parametrize('real', ['f32', 'f64'])
def test_device_views_outlive_later_evaluations(real):
    import cases
    G = cases.config3_graphs(24, seed=9)
    X, C = G[:15], G[15:]
    k = _graph_kernel(real)
    A, dA = k.device_cross_gram(X, C, eval_gradient=True)
    a, da = _np(A).copy(), _np(dA).copy()
    d, dd = k.device_diag(X, eval_gradient=True)
    d0, dd0 = _np(d).copy(), _np(dd).copy()
    # more evaluations on the same backend: another cross matrix, diagonals,
    # the symmetric device path and a host call
    B, dB = k.device_cross_gram(C, X, eval_gradient=True)
    k.device_diag(C, eval_gradient=True)
    k.device_gram(G, eval_gradient=True)
    k(G, eval_gradient=True)
    np.testing.assert_array_equal(_np(A), a)
    np.testing.assert_array_equal(_np(dA), da)
    np.testing.assert_array_equal(_np(d), d0)
    np.testing.assert_array_equal(_np(dd), dd0)
    # ((j, i) is a linear system of its own: equal to the solver's accuracy)
    np.testing.assert_allclose(_np(B), a.T, rtol=1e-4)


def test_device_methods_refuse_other_backends():
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    import cases
    knode, kedge, _ = cases.config3_kernels()

    class Plain:                  # a backend of the plugin seam without prepare
        pass
    k = MarginalizedGraphKernel(knode, kedge, backend=_backend('f32'))
    k.backend = Plain()
    G = cases.config3_graphs(3, seed=1)
    with pytest.raises(TypeError):
        k.device_cross_gram(G[:2], G[2:])
    with pytest.raises(TypeError):
        k.device_diag(G)


# -- lowrank.hip ---------------------------------------------------------------
def _planes(N, M, nt, dtype, seed):
    import torch
    g = torch.Generator(device='cpu').manual_seed(seed)
    P = torch.randn((nt, M, N), generator=g, dtype=torch.float64)
    P = P.to(dtype).to('cuda').permute(2, 1, 0)     # column-major (N, M, nt)
    W = torch.randn((N, M), generator=g, dtype=torch.float64).to('cuda')
    return P, W


SHAPES = [(1, 3, 2), (1, 1, 1), (37, 5, 3), (301, 1, 4), (129, 9, 16),
          (77, 6, 17), (20011, 50, 8), (2053, 31, 40), (64, 4, 1)]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('N, M, nt', SHAPES)
def test_lowrank_contraction_against_torch(N, M, nt, dtype):
    import torch
    from graphdot_amd.model.gaussian_process import _lowrank
    P, W = _planes(N, M, nt, getattr(torch, dtype), seed=N + M + nt)
    if N > 2:
        W[1::3] = 0.0                     # zero rows (masked targets)
    want = torch.einsum('ic,ick->k', W, P.double())
    got = _lowrank.contract(P, W)
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(),
                               rtol=1e-11, atol=1e-11 * float(
                                   (W.abs()[:, :, None] * P.abs().double()
                                    ).sum()))
    # the same bits on every call
    for _ in range(3):
        assert torch.equal(_lowrank.contract(P, W), got)
    # the torch route agrees
    np.testing.assert_allclose(_lowrank.contract_torch(P, W).cpu().numpy(),
                               got.cpu().numpy(), rtol=1e-10, atol=1e-9)
    # a row index list in place of the zero rows
    rows = np.array([i for i in range(N) if not (N > 2 and i % 3 == 1)])
    sub = _lowrank.contract(P, W[torch.as_tensor(rows, device='cuda')], rows)
    np.testing.assert_allclose(sub.cpu().numpy(), got.cpu().numpy(),
                               rtol=1e-10, atol=1e-9)


def test_lowrank_contraction_checks_its_arguments():
    import torch
    from graphdot_amd.model.gaussian_process import _lowrank
    P, W = _planes(10, 3, 2, torch.float32, seed=1)
    with pytest.raises(IndexError):
        _lowrank.contract(P, W[:2], rows=[0, 10])
    with pytest.raises(ValueError):
        _lowrank.contract(P.contiguous(), W)      # not column-major
    with pytest.raises(ValueError):
        _lowrank.contract(P, W[:, :2])
    assert torch.equal(_lowrank.contract(P[:0], W[:0]),
                       torch.zeros(2, dtype=torch.float64, device='cuda'))


# -- the regressor -----------------------------------------------------------------
def _targets(G, masked=False):
    y = np.array([len(g.nodes) + 0.3 * np.sin(i) for i, g in enumerate(G)],
                 dtype=float)
    if masked:
        y[[2, 11]] = np.nan
    return y


@pytest.mark.parametrize('masked', [False, True])
def test_device_model_matches_the_cpu_model(masked):
    import cases
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.model.gaussian_process import LowRankApproximateGPR
    G = cases.config3_graphs(70, seed=13)
    X, C, Z = G[:50], G[50:62], G[62:]
    y = _targets(X, masked)
    kernel = Normalization(_graph_kernel('f64'))
    models = [LowRankApproximateGPR(kernel, alpha=1e-6, normalize_y=True,
                                    device=d) for d in ('cuda', 'cpu')]
    out = []
    for m in models:
        m.C, m.X, m.y = C, X, y
        lml, grad = m.log_marginal_likelihood(eval_gradient=True)
        m.fit(C, X, y)
        mean, std = m.predict(Z, return_std=True)
        out.append((lml, grad, mean, std,
                    m.predict_loocv(Z, _targets(Z), method='gpr-like')))
    assert models[0].Ky.is_cuda and not models[1].Ky.is_cuda
    for a, b in zip(*out):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9)


class NoDownload:
    """The kernel with its host entry points disabled: only the device
    methods may be used."""

    def __init__(self, k):
        self.k = k

    def __getattr__(self, name):
        return getattr(self.k, name)

    def __call__(self, *args, **kwargs):
        raise AssertionError('a kernel matrix was downloaded')

    def diag(self, *args, **kwargs):
        raise AssertionError('a diagonal was downloaded')

    def clone_with_theta(self, theta):
        return NoDownload(self.k.clone_with_theta(theta))

    def device_cross_gram(self, *args, **kwargs):
        return self.k.device_cross_gram(*args, **kwargs)

    def device_gram(self, *args, **kwargs):
        return self.k.device_gram(*args, **kwargs)

    def device_diag(self, *args, **kwargs):
        return self.k.device_diag(*args, **kwargs)


@pytest.mark.parametrize('real', ['f32', 'f64'])
def test_no_download(real):
    import cases
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.model.gaussian_process import LowRankApproximateGPR
    G = cases.config3_graphs(60, seed=17)
    X, C, Z = G[:40], G[40:50], G[50:]
    y = _targets(X)
    k = Normalization(_graph_kernel(real))
    m = LowRankApproximateGPR(NoDownload(k), alpha=1e-5, device='cuda')
    m.C, m.X, m.y = C, X, y
    lml, grad = m.log_marginal_likelihood(eval_gradient=True)
    m.fit(C, X, y)
    mean, std = m.predict(Z, return_std=True)
    ref = LowRankApproximateGPR(k, alpha=1e-5, device='cpu')
    ref.C, ref.X, ref.y = C, X, y
    lml_h, grad_h = ref.log_marginal_likelihood(eval_gradient=True)
    tol = 1e-9 if real == 'f64' else 1e-3
    assert lml == pytest.approx(lml_h, rel=tol)
    np.testing.assert_allclose(grad, grad_h, rtol=tol, atol=tol)
    assert np.all(np.isfinite(mean)) and np.all(std >= 0)


def test_peak_memory_far_below_n_squared():
    import cases
    import torch
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.model.gaussian_process import LowRankApproximateGPR
    N, m = 20000, 50
    G = cases.config3_graphs(N + m, seed=23)
    X, C = G[:N], G[N:]
    y = _targets(X)
    model = LowRankApproximateGPR(Normalization(_graph_kernel('f64')),
                                  alpha=1e-6, device='cuda')
    model.C, model.X, model.y = C, X, y
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lml, grad = model.log_marginal_likelihood(eval_gradient=True)
    model.fit(C, X, y)
    model.predict(X[:500], return_std=True)
    peak = torch.cuda.max_memory_allocated() - base
    assert np.isfinite(lml) and np.all(np.isfinite(grad))
    assert peak < N * N * 8 // 20, peak
