"""Active-learning selectors (graphdot_amd.model.active_learning) against the
reference's picks (golden/active_learning.json, made by
golden/make_golden_active_learning.py), against plain float64 restatements of
the greedy criteria written here, and -- on the GPU -- the device loops of
select.hip against the host loops."""
import json
import os
import numpy as np
import pytest
from graphdot_amd.model.active_learning import (
    DeterminantMaximizer, VarianceMinimizer, HierarchicalDrafter,
    SelectionError)

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, 'golden', 'active_learning.json')) as f:
    GOLDEN = json.load(f)


def rbf(X, length):
    X = np.asarray(X, dtype=np.float64)
    d2 = ((X[:, None, :] - X[None, :, :])**2).sum(-1)
    return np.exp(-0.5 * d2 / length**2)


def selector(method, kernel='precomputed', device='cpu', alpha=1e-6):
    if method == 'determinant':
        return DeterminantMaximizer(kernel, device=device)
    return VarianceMinimizer(kernel, alpha=alpha, device=device)


def greedy_margins(K, picks, method, alpha=0.0):
    """For each pick: (best criterion - criterion of the pick) / |best| over
    the samples not chosen before it.  Criteria by the plain updates: the
    reference's row projection for the determinant, a rank-one downdate of
    the posterior covariance of K + alpha I for the variance."""
    N = len(K)
    A = np.array(K, dtype=np.float64)
    if method == 'variance':
        A[np.diag_indices(N)] += alpha
    free = np.ones(N, dtype=bool)
    out = []
    for i in picks:
        if method == 'determinant':
            crit = (A**2).sum(axis=1)
        else:
            crit = A[:, free].sum(axis=1)
        best = crit[free].max()
        out.append((best - crit[i]) / abs(best))
        if method == 'determinant':
            v = A[i] / np.linalg.norm(A[i])
            A -= np.outer(A @ v, v)
        else:
            A -= np.outer(A[:, i], A[i]) / A[i, i]
        free[i] = False
    return np.array(out)


GOLDEN_IDS = [f"{p['method']}-{p['dim']}d-N{p['N']}-n{p['n']}"
              for p in GOLDEN['problems']]


# ---------------------------------------------------------------- host (CPU)
@pytest.mark.parametrize('p', GOLDEN['problems'], ids=GOLDEN_IDS)
def test_host_reproduces_reference_picks(p):
    K = rbf(p['X'], p['length'])
    picks = selector(p['method'], alpha=p['alpha'])(K, p['n'])
    assert picks == p['picks']
    assert all(isinstance(i, int) for i in picks)


def test_golden_problems_cover_the_issue_ranges():
    ps = GOLDEN['problems']
    assert {p['dim'] for p in ps} == {1, 3}
    assert {p['method'] for p in ps} == {'determinant', 'variance'}
    assert all(50 <= p['N'] <= 400 and 5 <= p['n'] <= 40 for p in ps)
    assert all(p['gap'] >= GOLDEN['min_gap'][p['method']] for p in ps)


@pytest.mark.parametrize('d', GOLDEN['drafts'],
                         ids=[f"{d['method']}-N{d['N']}" for d in GOLDEN['drafts']])
def test_drafter_reproduces_reference_picks(d):
    X = np.array(d['X'])
    sel = selector(d['method'], kernel=lambda Y: rbf(Y, d['length']))
    picks = HierarchicalDrafter(sel)(X, d['n'], random_state=d['seed'])
    assert isinstance(picks, np.ndarray)
    assert picks.tolist() == d['picks']
    # a Generator works as well as a seed
    again = HierarchicalDrafter(sel)(
        X, d['n'], random_state=np.random.Generator(np.random.PCG64(d['seed'])))
    assert again.tolist() == d['picks']


def geometry(name, N):
    if name == 'line':
        return np.linspace(0, 1, N)[:, None], 0.1
    if name == 'ring':
        t = 2 * np.pi * np.arange(N) / N
        return np.column_stack((np.cos(t), np.sin(t))), 0.3
    rng = np.random.default_rng(N)
    return rng.uniform(-1, 1, size=(N, 2)), 0.25


@pytest.mark.parametrize('method', ['determinant', 'variance'])
@pytest.mark.parametrize('shape', ['line', 'ring', 'random'])
def test_reference_properties(method, shape):
    N, n = 120, 12
    X, length = geometry(shape, N)
    K = rbf(X, length)
    picks = selector(method)(K, n)
    assert len(picks) == n and len(set(picks)) == n
    assert all(0 <= i < N for i in picks)
    # a kernel (not precomputed) gives the same picks
    assert selector(method, kernel=lambda Y: rbf(Y, length))(X, n) == picks
    # better than random subsets in log-determinant
    rng = np.random.default_rng(0)
    ld = np.linalg.slogdet(K[np.ix_(picks, picks)])[1]
    for _ in range(20):
        r = rng.choice(N, n, replace=False)
        assert ld > np.linalg.slogdet(K[np.ix_(r, r)])[1]
    # N = n returns everything
    small = K[:9, :9]
    assert sorted(selector(method)(small, 9)) == list(range(9))


def test_ties_go_to_the_smallest_index():
    K = np.eye(6)
    assert DeterminantMaximizer('precomputed', device='cpu')(K, 4) == \
        [0, 1, 2, 3]
    assert VarianceMinimizer('precomputed', device='cpu')(K, 4) == \
        [0, 1, 2, 3]


@pytest.mark.parametrize('method', ['determinant', 'variance'])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_every_pick_is_greedy_optimal(method, seed):
    rng = np.random.default_rng(seed)
    N, n = 300, 40
    if seed == 0:           # a grid: many exactly equal criteria
        g = np.arange(10) / 10.0
        X = np.array(np.meshgrid(g, g, g[:3])).reshape(3, -1).T
    else:
        X = rng.uniform(-1, 1, size=(N, 2))
    K = rbf(X, 0.2)
    picks = selector(method)(K, n)
    margins = greedy_margins(K, picks, method, alpha=1e-6)
    assert margins.max() <= 1e-9, margins.max()


@pytest.mark.parametrize('method', ['determinant', 'variance'])
def test_rank_deficient_matrix_raises(method):
    X = np.repeat(np.random.default_rng(3).uniform(-1, 1, (5, 1)), 2, axis=0)
    K = rbf(X, 0.5)
    # exact rank: duplicates are never both picked... until nothing is left
    sel = selector(method, alpha=0.0)
    picks = sel(K, 5)
    assert sorted(X[picks, 0]) == sorted(np.unique(X[:, 0]))
    with pytest.raises(SelectionError) as e:
        sel(K, 6)
    assert len(e.value.picks) == 5
    assert isinstance(e.value, np.linalg.LinAlgError)


def test_arguments_follow_the_reference():
    with pytest.raises(AssertionError):
        DeterminantMaximizer('something else')
    with pytest.raises(AssertionError):
        VarianceMinimizer(42)
    with pytest.raises(AssertionError):
        DeterminantMaximizer('precomputed', device='cpu')(np.eye(3), 4)
    with pytest.raises(AssertionError):
        DeterminantMaximizer('precomputed', device='cpu')(np.ones((3, 4)), 2)
    with pytest.raises(AssertionError):
        HierarchicalDrafter(DeterminantMaximizer('precomputed'), k=1)
    with pytest.raises(ValueError):
        DeterminantMaximizer('precomputed', device='tpu')(np.eye(3), 1)
    assert VarianceMinimizer('precomputed').alpha == 1e-6


def test_cpu_torch_tensor_is_accepted():
    torch = pytest.importorskip('torch')
    K = rbf(np.random.default_rng(1).uniform(size=(40, 2)), 0.3)
    want = DeterminantMaximizer('precomputed', device='cpu')(K, 8)
    got = DeterminantMaximizer('precomputed', device='cpu')(
        torch.from_numpy(K), 8)
    assert got == want


# ---------------------------------------------------------------- the GPU
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('p', GOLDEN['problems'], ids=GOLDEN_IDS)
def test_device_picks_equal_host_picks(p, dtype):
    import torch
    K = rbf(p['X'], p['length']).astype(dtype)
    host = selector(p['method'], alpha=p['alpha'])(K, p['n'])
    assert host == p['picks']
    dev = selector(p['method'], device='cuda', alpha=p['alpha'])
    assert dev(K, p['n']) == host                      # numpy, uploaded
    Kt = torch.from_numpy(K).cuda()
    assert dev(Kt, p['n']) == host                     # a device tensor
    assert dev(Kt.T.contiguous(), p['n']) == host     # (its transpose)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,tol', [('float64', 1e-9), ('float32', 1e-6)])
@pytest.mark.parametrize('method', ['determinant', 'variance'])
def test_device_picks_are_greedy_optimal_at_scale(method, dtype, tol):
    import torch
    N, n = 4000, 200
    X = np.random.default_rng(4000).uniform(-1, 1, size=(N, 3))
    K = rbf(X, 0.3).astype(dtype)
    Kt = torch.from_numpy(K).cuda()
    picks = selector(method, device='cuda')(Kt, n)
    assert len(set(picks)) == n
    margins = greedy_margins(K.astype(np.float64), picks, method, alpha=1e-6)
    assert margins.max() <= tol, margins.max()


def _graph_kernel(normalized=False):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    knode, kedge, _ = cases.config3_kernels()
    k = MarginalizedGraphKernel(knode, kedge, q=0.05, backend='hip')
    return Normalization(k) if normalized else k


@pytest.mark.gpu
@pytest.mark.parametrize('normalized', [False, True])
@pytest.mark.parametrize('method', ['determinant', 'variance'])
def test_graph_kernel_selects_on_the_device_gram_matrix(method, normalized):
    import cases
    G = cases.config3_graphs(40, seed=21)
    kernel = _graph_kernel(normalized)
    K = kernel(G)                     # the download, for the comparison
    n = 10
    want_cpu = selector(method)(K, n)
    want_dev = selector(method, device='cuda')(K, n)

    class NoDownload:
        def __init__(self, k):
            self.k = k

        def __getattr__(self, name):
            return getattr(self.k, name)

        def __call__(self, *args, **kwargs):
            raise AssertionError('the full kernel matrix was downloaded')

        def device_gram(self, X, **kwargs):
            return self.k.device_gram(X, **kwargs)

    got = selector(method, kernel=NoDownload(kernel), device='cuda')(G, n)
    assert got == want_dev == want_cpu
    # the drafter hands every chunk's Gram matrix to the device path as well
    d = HierarchicalDrafter(selector(method, kernel=NoDownload(kernel),
                                     device='cuda'))(G, 8, random_state=1)
    h = HierarchicalDrafter(selector(method, kernel=kernel, device='cpu'))(
        G, 8, random_state=1)
    assert d.tolist() == h.tolist()


@pytest.mark.gpu
def test_rank_deficient_graph_kernel_raises_on_the_device():
    import cases
    G = cases.config3_graphs(6, seed=21)
    G2 = [g for g in G for _ in range(2)]          # every graph twice
    kernel = _graph_kernel(normalized=True)
    sel = DeterminantMaximizer(kernel, device='cuda')
    picks = sel(G2, 6)
    assert len(set(picks)) == 6 and len({i // 2 for i in picks}) == 6
    with pytest.raises(SelectionError) as e:
        sel(G2, 7)
    assert len(e.value.picks) == 6
    vsel = VarianceMinimizer(kernel, alpha=0.0, device='cuda')
    with pytest.raises(SelectionError):
        vsel(G2, 7)
