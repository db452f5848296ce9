"""The device path of KernelIsomap on an MI355X: every kernel of
model/manifold/geodesic.h alone against the definition of the model in numpy
(test_isomap.py: its definition, its data and its bounds), fed the
definition's inputs so that each is tested by itself; then the model on a CUDA
matrix against the definition and against itself on the CPU, and on a graph
kernel of the HIP backend.

The shapes are those of test_isomap.py: below a wave, one tile (one round, two
of the three phases never launched), a tile plus one, two tiles plus one
(`geo_fw_rest` has four workgroups, one of them 1 x 1) and 200 (an interior
tile).  Storage is float and double, in both layouts; one matrix is not
symmetric."""
import numpy as np
import pytest

import test_isomap as cpu

pytestmark = pytest.mark.gpu

SHAPES = cpu.SHAPES
DTYPES = cpu.DTYPES
LAYOUTS = ['row-major', 'column-major']
#: query rows of geo_extend: one; two strips and one row; four and one
ROWS = [1, 33, 65]


def _torch():
    import torch
    import graphdot_amd.model.manifold  # noqa: F401 (torch first)
    return torch


def _t(a):
    return cpu._t(a)


def _matrix(K, layout):
    """K on the device, contiguous along the index `layout` names."""
    A = _t(K).cuda()
    return A.t().contiguous().t() if layout == 'column-major' else A


def _bits(t):
    return t.clone().view(_torch().int64).cpu()


# -- 1. the graph ----------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_graph_against_the_definition(n, k, dtype):
    torch = _torch()
    from graphdot_amd.model.manifold import _geodesic
    c = cpu.case(n, k, dtype)
    for layout in LAYOUTS:
        K = _matrix(c.K, layout)
        assert K.stride() == ((n, 1) if layout == 'row-major' else (1, n))
        W = _geodesic.graph(K, _t(c.d).cuda(), _t(c.idx).cuda())
        assert W.dtype == torch.float64 and W.is_contiguous()
        assert np.array_equal(W.cpu().numpy(), c.W)


@pytest.mark.parametrize('dtype', DTYPES)
def test_graph_of_an_asymmetric_matrix(dtype):
    from graphdot_amd.model.manifold import _geodesic
    n, k = 129, 6
    K = np.array(cpu.case(n, k, dtype).K)
    r = np.random.RandomState(3)
    K += (1e-3 * r.rand(n, n) * ~np.eye(n, dtype=bool)).astype(dtype)
    assert not np.array_equal(K, K.T)
    W, idx = cpu.define_graph(K, k)
    assert np.array_equal(W, W.T)
    d = np.diag(K).astype(np.float64)
    for layout in LAYOUTS:
        got = _geodesic.graph(_matrix(K, layout), _t(d).cuda(),
                              _t(idx).cuda())
        assert np.array_equal(got.cpu().numpy(), W)


# -- 2. the shortest paths -------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_shortest_paths_against_the_definition(n, k, dtype):
    torch = _torch()
    from graphdot_amd.model.manifold import _geodesic
    c = cpu.case(n, k, dtype)
    G = _t(c.W).cuda()
    assert _geodesic.shortest_paths(G) is G                 # (in place)
    again = _geodesic.shortest_paths(_t(c.W).cuda())
    assert torch.equal(_bits(G), _bits(again))
    assert torch.equal(_bits(G), _bits(G.t().contiguous()))
    got = G.cpu().numpy()
    assert cpu.close_paths(got, c.G)
    print(f'n = {n}: geodesics within '
          f'{np.abs(got / np.where(c.G > 0, c.G, 1) - (c.G > 0)).max():.1e} '
          'relative of the definition')


def test_shortest_paths_of_two_clusters():
    from graphdot_amd.model.manifold import _geodesic
    K = cpu.clusters()
    W, _ = cpu.define_graph(K, 3)
    G = _geodesic.shortest_paths(_t(W).cuda())
    got = G.cpu().numpy()
    assert not np.isnan(got).any()
    assert cpu.close_paths(got, cpu.define_paths(W))
    B, label, count = _geodesic.finish(G)
    assert label.cpu().tolist() == [0] * 10 + [10] * 7
    assert count.cpu().tolist() == [2, 0] and label.dtype == count.dtype
    assert _geodesic.component_sizes(label.cpu().numpy()) == [10, 7]
    assert np.array_equal(B.cpu().numpy(), -0.5 * (got * got))


# -- 3. B and the components -----------------------------------------------------------
@pytest.mark.parametrize('n, k', SHAPES)
def test_finish_against_the_definition(n, k):
    from graphdot_amd.model.manifold import _geodesic
    c = cpu.case(n, k, np.float64)
    G = _geodesic.shortest_paths(_t(c.W).cuda())
    own = G.cpu().numpy()
    B, label, count = _geodesic.finish(G)
    assert np.array_equal(G.cpu().numpy(), own)             # (G is read only)
    assert np.array_equal(B.cpu().numpy(), -0.5 * (own * own))
    assert not label.cpu().numpy().any()
    count = count.cpu().numpy()
    assert count.shape == (-(-n // 16),) and count[0] == 1 == count.sum()


# -- 4. out of sample ------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_extension_against_the_definition(n, k, dtype):
    from graphdot_amd.model.manifold import _geodesic
    c = cpu.case(n, k, dtype)
    P = cpu.points(n, cpu.SEEDS[n])
    Q = np.random.RandomState(7).rand(max(ROWS), 3)
    Q[3] = P[0]
    Kq = cpu.gaussian(Q, P).astype(dtype)
    d2, idx = cpu.define_lists(Kq, np.ones(len(Q)), c.d, k)
    want = (np.sqrt(d2)[:, :, None] + c.G[idx]).min(1)
    G = _t(c.G).cuda()
    for b in ROWS:
        Bq, Gq = _geodesic.extend(_t(d2[:b]).cuda(), _t(idx[:b]).cuda(), G,
                                  True)
        assert Bq.shape == Gq.shape == (b, n)
        assert np.array_equal(Gq.cpu().numpy(), want[:b])
        assert np.array_equal(Bq.cpu().numpy(), -0.5 * (want[:b] * want[:b]))
        only, none = _geodesic.extend(_t(d2[:b]).cuda(), _t(idx[:b]).cuda(),
                                      G)
        assert none is None and np.array_equal(only.cpu().numpy(),
                                               Bq.cpu().numpy())


# -- 5. the model on a matrix on the device ----------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, k', SHAPES)
def test_model_on_a_cuda_matrix(n, k, dtype):
    from graphdot_amd.model.manifold import KernelIsomap
    c = cpu.case(n, k, dtype)
    K = _matrix(c.K, LAYOUTS[n % 2])
    bits = K.clone()
    model = KernelIsomap('precomputed', k, c.c)
    Y = model.fit_transform(K)
    assert model.last_timing['fused'] is True
    assert model.last_timing['adopted'] is False
    assert (K == bits).all() and K.stride() == bits.stride()
    worst = cpu.check_model(model, c)
    # ... and against the same model on the same matrix on the CPU
    host = KernelIsomap('precomputed', k, c.c, device='cpu').fit(
        np.array(c.K))
    assert host.last_timing['fused'] is False
    assert cpu.close_paths(model.dist_matrix_, host.dist_matrix_)
    sign = np.where((Y * host.embedding_).sum(0) < 0, -1.0, 1.0)
    assert np.abs(Y * sign - host.embedding_).max() \
        <= cpu.band(n, k, 'embedding')
    Kq, dq = _t(c.Kq).cuda(), _t(c.dq).cuda()
    Gq = model.geodesic_distances(Kq, diag=dq)
    assert cpu.close_paths(Gq, c.Gq, n + 1)
    assert cpu.close_paths(Gq, host.geodesic_distances(np.array(c.Kq), diag=c.dq),
                           n + 1)
    Yq = model.transform(Kq, diag=dq)
    worst_q = np.abs(Yq * np.where((Y * c.Y).sum(0) < 0, -1.0, 1.0)
                     - c.Yq).max()
    assert worst_q <= cpu.band(n, k, 'transform'), worst_q
    assert np.abs(Yq * sign - host.transform(np.array(c.Kq), diag=c.dq)).max() \
        <= cpu.band(n, k, 'transform')
    # a repeat: the same bits
    again = KernelIsomap('precomputed', k, c.c).fit(K)
    assert np.array_equal(again.dist_matrix_, model.dist_matrix_)
    assert np.array_equal(again.embedding_, Y)
    print(f'n = {n}: embedding within {worst:.1e}, transform within '
          f'{worst_q:.1e} of the definition')


def test_model_errors_on_the_device():
    from graphdot_amd.model.manifold import KernelIsomap
    K = _t(cpu.clusters()).cuda()
    with pytest.raises(ValueError, match=r'2 components of sizes \[10, 7\]'):
        KernelIsomap('precomputed', 3, 2).fit(K)
    bad = K.clone()
    bad[1, 3] = float('nan')
    with pytest.raises(ValueError, match='not finite'):
        KernelIsomap('precomputed', 10, 2).fit(bad)
    # the ring: the eigenvalues of largest magnitude are not the largest
    ring = cpu.ring()
    w = cpu.define_embedding(cpu.define_paths(cpu.define_graph(ring, 2)[0]),
                             4)[0]
    model = KernelIsomap('precomputed', 2, 4).fit(_t(ring).cuda())
    assert model.last_timing['fused'] is True
    assert (model.eigenvalues_ > 0).all()
    assert np.abs(model.eigenvalues_ - w).max() <= 16 * 96 * cpu.U * w[0]


# -- 6. the model on a graph kernel ----------------------------------------------------
N_GRAPHS = 40


def _kernel(real):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    knode, kedge, q = cases.config3_fit_kernels()
    return Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, q_bounds=(1e-3, 0.5),
        backend=HIPBackend(real=real),
        ftol=1e-13 if real is np.float64 else 1e-8))


@pytest.mark.parametrize('real', [np.float32, np.float64])
def test_model_on_the_device_path(real, monkeypatch):
    """A graph kernel on the HIP backend: the matrix is adopted where the
    solver wrote it, no host kernel evaluation, the result is that of
    'precomputed' on the downloaded matrix, and the solver's buffer holds the
    same bits afterwards."""
    import cases
    from graphdot_amd.model.manifold import KernelIsomap
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G = np.asarray(list(cases.config3_graphs(N_GRAPHS, seed=29)),
                   dtype=object)
    kernel = _kernel(real)
    theta0 = np.array(kernel.theta)
    K = torch.as_tensor(kernel.device_gram(G), device='cuda').cpu().numpy()
    calls = []

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
    seen, gram = [], KernelIsomap._gram

    def spy(self, X):
        out = gram(self, X)
        seen.append(out[0])
        return out
    monkeypatch.setattr(KernelIsomap, '_gram', spy)
    model = KernelIsomap(kernel, 8, 2, device='cuda')
    Y = model.fit_transform(G)
    assert model.last_timing['adopted'] is True
    assert model.last_timing['fused'] is True
    assert np.array_equal(kernel.theta, theta0) and calls == []
    # the solver's buffer, which the fit worked on: the kernel's matrix still
    after = seen[0].cpu().numpy()
    assert len(seen) == 1 and seen[0].is_cuda
    assert after.dtype == K.dtype and np.array_equal(after, K)
    pre = KernelIsomap('precomputed', 8, 2, device='cuda').fit(K)
    assert np.array_equal(model.dist_matrix_, pre.dist_matrix_)
    assert np.array_equal(Y, pre.embedding_)
    assert np.array_equal(model.eigenvalues_, pre.eigenvalues_)
    Yq = model.transform(G[:5])
    assert Yq.shape == (5, 2) and np.isfinite(Yq).all()
    assert np.array_equal(kernel.theta, theta0) and calls == []
