"""Active-learning selectors (graphdot_amd.model.active_learning) against the
reference's picks (golden/active_learning.json, made by
golden/make_golden_active_learning.py), against plain float64 restatements of
the greedy criteria written here, and -- on the GPU -- the device loops of
select.hip against the host loops.  The state of the two loops by its
definition and by the loops' recurrence, with the bounds derived from their
difference, is here as well: test_active_learning_gpu.py holds select.hip's
state against it."""
import functools
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


# ------------------------------------------------- the state of the two loops
# What test_active_learning_gpu.py compares select.hip's state with.  Both
# references take the stored matrix widened to double and the picks P they are
# to follow (teacher-forced: a near-tie cannot turn a rounding difference
# into another trajectory), and both return the state as `_select.select`
# leaves it after len(P) picks -- the last pick gets no criterion update:
#   determinant: crit (rho after n - 1 updates), Q (N, n - 1), C (n - 1, N),
#                w (the last direction, not scaled), scal (1 / |w|)
#   variance:    crit, L (N, n), p (the posterior column of the last pick)
# and the criterion before every pick, hist (n, N).
EPS = np.finfo(np.float64).eps
#: the tolerance of the GPU tests: 8 x max(E_host, 4 eps) x scale, E_host the
#: error of the recurrence (the host loops', restated) against the definition
FACTOR, FLOOR = 8, 4 * EPS
#: `spd` has a condition number of about 9: classical Gram-Schmidt loses
#: orthogonality like cond^2 eps, and the restatement has to stay within
#: 4 x that of the definition to be a yardstick at all
E_HOST_CAP = 4 * 81 * EPS
ALPHA = 1e-2        # of the variance cases: visible where it is forgotten


@functools.lru_cache(maxsize=None)
def spd(N, seed, dtype='float64'):
    """A A^T / N + I / 2, A (N, N) standard normal, as stored in `dtype`
    (exactly symmetric; read-only: shared among the tests)."""
    A = np.random.default_rng(seed).standard_normal((N, N))
    K = A @ A.T / N + 0.5 * np.eye(N)
    K = (0.5 * (K + K.T)).astype(dtype)
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def tie_matrix(name, dtype='float64'):
    """'pairs': 260 blocks [[1, .5], [.5, 1]] (N = 520; all criteria equal
    at the start, equal within the even and the odd samples afterwards);
    'identity': I_600."""
    K = np.kron(np.eye(260), [[1.0, 0.5], [0.5, 1.0]]) if name == 'pairs' \
        else np.eye(600)
    K = K.astype(dtype)
    K.setflags(write=False)
    return K


#: (N, n) of the state tests: the smallest; the 64 rows of an al_colreduce
#: pass on both sides ((64, 64): n == N); the block of 256 on both sides
#: ((257, 257): a second block of one row, a last al_colreduce block with one
#: live wave, n == N); three blocks
SHAPES = [(1, 1), (2, 2), (63, 20), (64, 64), (65, 33), (255, 33), (256, 33),
          (257, 257), (513, 40)]
#: more picks than one pass of the coefficient staging holds (CHUNK of
#: select.hip): steps 1024 and 1025 are the first with a full chunk and with
#: a second chunk of one coefficient; 1040 = 4 x 256 + 16 rows
BEYOND_ONE_CHUNK = (1040, 1028)


def chunk_of_select_hip():
    import re
    import graphdot_amd.model.active_learning as al
    path = os.path.join(os.path.dirname(al.__file__), 'select.hip')
    with open(path) as f:
        return int(re.search(r'^#define CHUNK (\d+)', f.read(), re.M).group(1))


def define_state(K, P, method, alpha=0.0):
    """The state by its definition (Householder QR of the chosen rows; the
    Cholesky factor of the chosen block), not by the loops' recurrences."""
    N, n = len(K), len(P)
    P = np.asarray(P)
    if method == 'determinant':
        Qr, R = np.linalg.qr(K[P[:-1]].T)
        Qr = Qr * np.sign(np.diag(R))
        C = (K @ Qr).T
        rho0 = np.einsum('ab,ab->a', K, K)
        w = K[P[-1]].copy()
        for _ in range(2):
            w -= Qr @ (Qr.T @ w)
        hist = rho0 - np.vstack((np.zeros(N), np.cumsum(C**2, axis=0)))
        return dict(crit=rho0 - (C**2).sum(axis=0), Q=Qr, C=C, w=w,
                    scal=np.array([1.0 / np.linalg.norm(w)])), hist
    A = K + alpha * np.eye(N)
    Lc = np.linalg.cholesky(A[np.ix_(P, P)])
    L = np.linalg.solve(Lc, A[P]).T
    L1 = L[:, :-1]
    U = np.ones(N, dtype=bool)
    U[P[:-1]] = False
    p = A[:, P[-1]] - L1 @ L1[P[-1]]
    crit = A[:, U].sum(axis=1) - L1 @ L1[U].sum(axis=0)
    hist = [A.sum(axis=1)]
    free = np.ones(N, dtype=bool)
    for s in range(n - 1):
        free[P[s]] = False
        l = L[:, s]
        hist.append(hist[-1] - l * (l[P[s]] + l[free].sum()))
    return dict(crit=crit, L=L, p=p), np.array(hist)


def restate_state(K, P, method, alpha=0.0):
    """The recurrences of `_greedy.determinant_host` / `variance_host`, made
    to pick P."""
    N, n = len(K), len(P)
    if method == 'determinant':
        Q = np.zeros((N, n - 1))
        C = np.zeros((n - 1, N))
        rho = np.einsum('ab,ab->a', K, K)
        hist = [rho.copy()]
        for s, i in enumerate(P):
            w = K[i] - Q[:, :s] @ C[:s, i]
            w2 = w @ w
            if s + 1 == n:
                break
            Q[:, s] = w / np.sqrt(w2)
            C[s] = K @ Q[:, s]
            rho = rho - C[s]**2
            hist.append(rho.copy())
        return dict(crit=rho, Q=Q, C=C, w=w,
                    scal=np.array([1.0 / np.sqrt(w2)])), np.array(hist)
    L = np.zeros((N, n))
    crit = K.sum(axis=1) + alpha
    free = np.ones(N, dtype=bool)
    hist = [crit.copy()]
    for s, j in enumerate(P):
        free[j] = False
        p = K[:, j] - L[:, :s] @ L[j, :s]
        p[j] += alpha
        l = p / np.sqrt(p[j])
        L[:, s] = l
        if s + 1 == n:
            break
        crit = crit - (p + l * l[free].sum())
        hist.append(crit.copy())
    return dict(crit=crit, L=L, p=p), np.array(hist)


def scales(K, want, method, alpha=0.0):
    """What an error of each quantity is relative to: the largest |K_a|^2
    for rho, the largest row sum of |K + alpha I| for the variance criterion,
    the quantity's own largest entry otherwise."""
    out = {k: np.abs(v).max() for k, v in want.items() if v.size}
    if method == 'determinant':
        out['crit'] = np.einsum('ab,ab->a', K, K).max()
    else:
        out['crit'] = np.abs(K + alpha * np.eye(len(K))).sum(axis=1).max()
    return out


def host_error(K, P, method, alpha=0.0):
    """(definition, its history, scales, E_host): E_host[q] is the largest
    error of the restated recurrence in quantity q, relative to its scale."""
    want, hist = define_state(K, P, method, alpha)
    got, _ = restate_state(K, P, method, alpha)
    scale = scales(K, want, method, alpha)
    e_host = {k: np.abs(got[k] - want[k]).max() / scale[k] for k in scale}
    return want, hist, scale, e_host


def bounds(scale, e_host):
    return {k: FACTOR * max(e_host[k], FLOOR) * scale[k] for k in scale}


def history_margins(hist, P):
    """Along the definition's criterion history, over the samples not chosen
    before each pick: (the largest best - criterion of the pick, the
    smallest best - second best)."""
    free = np.ones(hist.shape[1], dtype=bool)
    margin, gap = 0.0, np.inf
    for s, i in enumerate(P):
        c = hist[s][free]
        best = c.max()
        margin = max(margin, best - hist[s][i])
        if len(c) > 1:
            gap = min(gap, best - np.partition(c, -2)[-2])
        free[i] = False
    return margin, gap


@functools.lru_cache(maxsize=None)
def host_picks(matrix, method, n, alpha=0.0):
    """The host loop's picks on `matrix` = ('spd', N, seed, dtype) or
    ('pairs' / 'identity', dtype): computed once for all tests."""
    from graphdot_amd.model.active_learning import _greedy
    return tuple(_greedy.run(stored(matrix).astype(np.float64), n, method,
                             alpha=alpha))


def stored(matrix):
    return spd(*matrix[1:]) if matrix[0] == 'spd' else tie_matrix(*matrix)


def alpha_of(matrix, method):
    """ALPHA for the variance on `spd`; none where the criteria are to stay
    exactly equal."""
    return ALPHA if method == 'variance' and matrix[0] == 'spd' else 0.0


STATE_MATRICES = \
    [(('spd', N, 10 + N, dt), n) for N, n in SHAPES + [BEYOND_ONE_CHUNK]
     for dt in ('float64', 'float32')] + \
    [((name, dt), 300) for name in ('pairs', 'identity')
     for dt in ('float64', 'float32')]


def matrix_id(case):
    matrix, n = case
    return '-'.join(str(x) for x in matrix) + f'-n{n}'


@pytest.mark.parametrize('method', ['determinant', 'variance'])
@pytest.mark.parametrize('case', STATE_MATRICES, ids=matrix_id)
def test_restated_recurrence_agrees_with_the_definition(case, method):
    matrix, n = case
    alpha = alpha_of(matrix, method)
    K = stored(matrix).astype(np.float64)
    P = host_picks(matrix, method, n, alpha)
    assert len(set(P)) == n
    want, hist, scale, e_host = host_error(K, P, method, alpha)
    bound = bounds(scale, e_host)['crit']
    margin, gap = history_margins(hist, P)
    print(f'{matrix_id(case)} {method}: E_host ' +
          ' '.join(f'{k} {v:.1e}' for k, v in e_host.items()) +
          f'; margin {margin / bound:.1e} gap {gap / bound:.1e} of the bound')
    assert max(e_host.values()) <= E_HOST_CAP, e_host
    # the picks are the greedy ones of the definition's criteria ...
    assert margin <= 2 * bound
    if matrix[0] == 'spd':
        # ... and on these matrices no rounding within 1000 bounds changes
        # one: the device has to make the very same picks
        assert gap > 1000 * bound
    else:
        assert gap <= bound             # (ties: the index decides)
        want =list(range(0, 520, 2)) + list(range(1, 80, 2)) \
            if matrix[0] == 'pairs' else list(range(300))
        assert list(P) == want


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
