"""The device path of KernelHDBSCAN on an MI355X: the kernels of
model/clustering/mst.h alone against the definition of the model in numpy
(test_hdbscan.py: its definition and its data), fed the definition's inputs so
that each is tested by itself -- the row pass of a first round and of a
labelling in the middle of a run, the hooking behind it and on hand-made
candidates, the edges of a whole run -- then the model on a CUDA matrix against
the definition and against itself on the CPU, and on a graph kernel of the HIP
backend.  Everything is compared exactly.

The shapes: two samples; below a wave; a tile less one, one tile, a tile plus
one (the second part of the columns holds one column); two tiles plus one;
200, where `parts_for` splits the columns in four and 1, 2 and 4 parts are
forced.  Storage is float and double, in both layouts; one matrix is not
symmetric, one is full of ties, one is all equal, two hold duplicates."""
import functools

import numpy as np
import pytest

import test_hdbscan as cpu

pytestmark = pytest.mark.gpu

SIZES = [2, 5, 63, 64, 65, 129, 200]
DTYPES = cpu.DTYPES
LAYOUTS = ['row-major', 'column-major']
MIN_SAMPLES = [1, 2, 5, 65]
#: query rows of the rectangular row pass: one; two strips and one row; three
ROWS = [1, 33, 65]


def _torch():
    import torch
    import graphdot_amd.model.clustering  # noqa: F401 (torch first)
    return torch


def _t(a):
    return cpu._t(a)


def _matrix(K, layout):
    """K on the device, contiguous along the index `layout` names."""
    A = _t(K).cuda()
    return A.t().contiguous().t() if layout == 'column-major' else A


def _int(a):
    return _t(np.asarray(a).astype(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def sized(n, dtype, min_samples):
    """The leading n samples of the case of 200."""
    return cpu.Case(np.array(cpu.data(200, 4, False, dtype)[:n, :n]),
                    min_samples)


def special(name, dtype):
    if name == 'asymmetric':
        return cpu.asymmetric(dtype=dtype)
    if name == 'grid':
        return np.array(cpu.data(200, 4, True, dtype))
    if name == 'all equal':
        return np.full((70, 70), 0.25, dtype=dtype)
    return cpu.duplicates(int(name)).astype(dtype)


SPECIAL = ['asymmetric', 'grid', 'all equal', '3', '5']


def _settings(n):
    return [m for m in MIN_SAMPLES if m <= n]


def _round(c, K, comp, parts=None):
    """One round on the device from the labels `comp` against the
    definition; the labels behind it."""
    torch = _torch()
    from graphdot_amd.model.clustering import _mst
    n = c.n
    w2, cand = cpu.define_rows(c.W2, comp)
    got = _mst.rows(K, _t(c.d).cuda(), _t(c.c2).cuda(), _int(comp),
                    parts=parts)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32
    assert np.array_equal(got[0].cpu().numpy(), w2)
    assert np.array_equal(got[1].cpu().numpy(), cand)
    assert int(got[2]) == 0
    edges = _mst.new_edges(n, K.device)
    after, count = _mst.hook(got[0], got[1], _int(comp), edges,
                             len(set(comp.tolist())))
    cpu.check_hook(after.cpu().numpy(), count.sum(),
                   [e.cpu().numpy() for e in edges], w2, cand, comp)
    return after.cpu().numpy().astype(np.int64)


# -- 1. a round ------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', SIZES)
def test_rounds_against_the_definition(n, dtype):
    """The row pass and the hooking of a first round and of the round behind
    it, whose labels are no longer the samples' own."""
    from graphdot_amd.model.clustering import _mst
    assert _mst.parts_for(200, 200) == 4 and _mst.parts_for(65, 65) == 2
    for min_samples in _settings(n):
        c = sized(n, dtype, min_samples)
        for layout in LAYOUTS:
            K = _matrix(c.K, layout)
            assert K.stride() == ((n, 1) if layout == 'row-major' else (1, n))
            comp = _round(c, K, np.arange(n))
            if len(set(comp.tolist())) > 1:
                _round(c, K, comp)


@pytest.mark.parametrize('parts', [1, 2, 4])
def test_rounds_with_the_columns_split(parts):
    c = sized(200, np.float32, 5)
    K = _matrix(c.K, 'row-major')
    comp = _round(c, K, np.arange(200), parts)
    _round(c, K, comp, parts)
    # more parts than tiles: the last ones are empty
    c = sized(65, np.float64, 2)
    _round(c, _matrix(c.K, 'column-major'), np.arange(65), 4)


@pytest.mark.parametrize('name', SPECIAL)
def test_rounds_on_the_special_matrices(name):
    for dtype in DTYPES:
        K = special(name, dtype)
        for min_samples in (1, 5):
            c = cpu.Case(K, min_samples)
            comp = _round(c, _matrix(K, 'row-major'), np.arange(c.n))
            if len(set(comp.tolist())) > 1:
                _round(c, _matrix(K, 'column-major'), comp)


def test_hook_on_hand_made_candidates():
    from graphdot_amd.model.clustering import _mst
    torch = _torch()
    for w2, cand, comp in cpu.hand_made():
        for components in (None, len(set(comp.tolist()))):
            edges = _mst.new_edges(len(comp), torch.device('cuda'))
            after, count = _mst.hook(_t(w2).cuda(), _int(cand), _int(comp),
                                     edges, components)
            cpu.check_hook(after.cpu().numpy(), count.sum(),
                           [e.cpu().numpy() for e in edges], w2, cand, comp)
            assert int(count.sum()) == 2


# -- 2. a whole run --------------------------------------------------------------------
def _run(c, K, parts=None):
    from graphdot_amd.model.clustering import _mst
    got = _mst.spanning_tree(K, _t(c.d).to(K.device), _t(c.c2).to(K.device),
                             parts=parts)
    assert got[3] is K.is_cuda
    assert np.array_equal(got[0], c.w2)
    assert np.array_equal(got[1], c.a) and np.array_equal(got[2], c.b)
    return got


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', SIZES)
def test_edges_of_a_whole_run(n, dtype):
    for min_samples in _settings(n):
        c = sized(n, dtype, min_samples)
        for layout in LAYOUTS:
            first = _run(c, _matrix(c.K, layout))
        again = _run(c, _matrix(c.K, layout))
        assert first[0].tobytes() == again[0].tobytes()
        # the torch chain on the same tensors: the same edges bit for bit
        _run(c, _t(c.K))
    if n == 200:
        for parts in (1, 2, 4):
            _run(c, _matrix(c.K, 'row-major'), parts)


@pytest.mark.parametrize('name', SPECIAL)
def test_edges_of_a_whole_run_on_the_special_matrices(name):
    for dtype in DTYPES:
        K = special(name, dtype)
        for min_samples in (1, 5):
            c = cpu.Case(K, min_samples)
            for layout in LAYOUTS:
                _run(c, _matrix(K, layout))
    if name == 'all equal':
        assert np.array_equal(c.a, np.zeros(69)) \
            and np.array_equal(c.b, np.arange(1, 70))


# -- 3. the model ----------------------------------------------------------------------
def _fit(K, min_samples, size, method='eom'):
    from graphdot_amd.model.clustering import KernelHDBSCAN
    return KernelHDBSCAN('precomputed', size, min_samples, method).fit(K)


@pytest.mark.parametrize('grid', [False, True])
@pytest.mark.parametrize('min_samples, size', cpu.SETTINGS + [(65, 10),
                                                              (66, 10)])
def test_model_on_a_cuda_matrix_equals_the_cpu_model(min_samples, size, grid):
    for dtype in DTYPES:
        c = cpu.case(200, 4, grid, dtype, min_samples)
        for method in cpu.METHODS:
            model = _fit(_matrix(c.K, 'column-major' if grid
                                 else 'row-major'), min_samples, size, method)
            assert model.last_timing['fused'] is (min_samples <= 65)
            assert model.last_timing['adopted'] is False
            cpu.check_model(model, c, size, method)
            host = cpu.fit(c.K, min_samples, size, method)
            for name in ('labels_', 'probabilities_', 'core_distances_',
                         'minimum_spanning_tree_', 'single_linkage_tree_',
                         'condensed_tree_'):
                assert np.array_equal(getattr(model, name),
                                      getattr(host, name)), name


@pytest.mark.parametrize('name', SPECIAL)
def test_model_on_the_special_matrices(name):
    K = special(name, np.float64)
    for min_samples in (1, 5):
        c = cpu.Case(K, min_samples)
        model = _fit(_t(K).cuda(), min_samples, 5)
        assert model.last_timing['fused'] is True
        cpu.check_model(model, c, 5, 'eom')
        assert np.isfinite(model.probabilities_).all()


@pytest.mark.parametrize('rows', ROWS)
def test_approximate_predict_equals_the_definition(rows):
    torch = _torch()
    from graphdot_amd.model.clustering import _mst
    n, ce = 200, 4
    X = cpu.points(n, ce, n + ce, False)
    Q = np.concatenate((cpu.points(10 * rows, ce, n + ce, False)[::10][:rows - 1],
                        X[100:101]))
    assert len(Q) == rows
    dq = np.ones(rows)
    for dtype in DTYPES:
        K, Ks = cpu.gaussian(X).astype(dtype), cpu.gaussian(Q, X).astype(dtype)
        for min_samples, size in cpu.SETTINGS + [(65, 10)]:
            c = cpu.Case(K, min_samples)
            model = _fit(_t(K).cuda(), min_samples, size)
            want = cpu.define_predict(c, c.model(size, 'eom'), Ks, dq,
                                      min_samples)
            for layout in LAYOUTS:
                got = model.approximate_predict(_matrix(Ks, layout),
                                                diag=_t(dq).cuda())
                assert np.array_equal(got[0], want[0])
                assert np.array_equal(got[1], want[1])
        # the rectangular row pass by itself, with the columns split
        cq = np.sort(cpu.define_d2(Ks, dq, c.d), axis=1)[:, min_samples - 2]
        args = [_t(a).cuda() for a in (Ks, dq, c.d, cq, c.c2)]
        plain = _mst.cross_rows_torch(*[a.cpu() for a in args])
        for parts in (None, 1, 3):
            got = _mst.cross_rows(*args, parts=parts)
            assert torch.equal(got[0].cpu(), plain[0])
            assert torch.equal(got[1].cpu(), plain[1]) and int(got[2]) == 0


def test_model_errors_on_the_device():
    torch = _torch()
    K = _t(np.array(cpu.data(96, 3, False))).cuda()
    for min_samples in (1, 5):
        for at in ((1, 3), (90, 2)):
            bad = K.clone()
            bad[at] = float('nan')
            with pytest.raises(ValueError, match='not finite'):
                _fit(bad, min_samples, 5)
        model = _fit(K, min_samples, 5)
        bad = K[:3].clone()
        bad[2, 95] = float('inf')
        with pytest.raises(ValueError, match='not finite'):
            model.approximate_predict(bad, diag=torch.ones(
                3, dtype=torch.float64, device='cuda'))
    before = K.clone()
    _fit(K, 5, 5)
    assert torch.equal(K, before)


# -- 4. the model on a graph kernel ----------------------------------------------------
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
    from graphdot_amd.model.clustering import KernelHDBSCAN
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
    seen, gram = [], KernelHDBSCAN._gram

    def spy(self, X):
        out = gram(self, X)
        seen.append(out[0])
        return out
    monkeypatch.setattr(KernelHDBSCAN, '_gram', spy)
    model = KernelHDBSCAN(kernel, 4, 3, device='cuda')
    model.fit(G)
    assert model.last_timing['adopted'] is True
    assert model.last_timing['fused'] is True
    assert np.array_equal(kernel.theta, theta0) and calls == []
    # the solver's buffer, which the fit worked on: the kernel's matrix still
    after = seen[0].cpu().numpy()
    assert len(seen) == 1 and seen[0].is_cuda
    assert after.dtype == K.dtype and np.array_equal(after, K)
    pre = KernelHDBSCAN('precomputed', 4, 3, device='cuda').fit(K)
    cpu.check_model(model, cpu.Case(K, 3), 4, 'eom')
    assert np.array_equal(model.labels_, pre.labels_)
    assert np.array_equal(model.probabilities_, pre.probabilities_)
    labels, strengths = model.approximate_predict(G[:5])
    assert labels.shape == (5,) and np.isfinite(strengths).all()
    assert np.array_equal(kernel.theta, theta0) and calls == []
