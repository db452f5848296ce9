"""The device path of the tree search on an MI355X: posterior.hip against
numpy float64 with a derived bound, `DevicePosterior.predict` against
`GaussianProcessRegressor.predict` on QM7-like graphs, `seek` on the device
against `seek` on the host, what a prediction uploads, and one end-to-end
search over symbol strings."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps

#: |device - host| of `predict` relative to the largest host value of the
#: same output: ten times the largest figure measured on an MI355X over the
#: cases of `test_device_posterior_equals_predict` (6.6e-11 with the double
#: solver, 5.1e-11 with the float one, both for the standard deviation under
#: the unnormalised kernel).  Both paths convert the
#: same solver output to double, so the float backend is no further off.
PREDICT_RTOL = {np.float64: 10 * 6.6e-11, np.float32: 10 * 5.1e-11}

#: seed of `test_seek_device_equals_host`, chosen on an MI355X so that the
#: gap condition the test asserts holds: smallest score gap 4.1e-5, largest
#: score difference 5.1e-13
SEEK_SEED = 0


def _torch():
    import torch
    import graphdot_amd.model.gaussian_process  # noqa: F401 (torch first)
    return torch


# -- posterior.hip against numpy float64 ------------------------------------------------
def _case(n, b, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, n))
    Kinv = np.linalg.inv(A @ A.T / n + np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    Ks = rng.normal(size=(b, n))
    return Kinv, Ks, rng.normal(size=n), rng.uniform(0.5, 2.0, size=b)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('b', [1, 3, 8, 16, 17, 40])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('with_T', [False, True])
def test_posterior_against_numpy(n, b, dtype, with_T):
    torch = _torch()
    from graphdot_amd.model.gaussian_process import _posterior
    Kinv, Ks, Ky, scale = _case(n, b, 1000 * n + b)
    Ks = Ks.astype(dtype)                      # the stored inputs
    K64 = Ks.astype(np.float64)
    T_ref = Kinv @ K64.T
    q_ref = np.einsum('cr,rc->c', K64, T_ref)
    kss = q_ref + scale                        # variances of order one
    ymean, ystd = 0.7, 1.9
    # column-major (b, n): element (c, j) at c + j b, as the solver leaves it
    Kst = torch.from_numpy(np.ascontiguousarray(Ks.T)).cuda().t()
    assert Kst.shape == (b, n)
    args = (torch.from_numpy(Kinv).cuda(), Kst, torch.from_numpy(Ky).cuda(),
            torch.from_numpy(kss).cuda(), ymean, ystd)
    out, T = _posterior.posterior(*args, return_T=with_T)
    out2, T2 = _posterior.posterior(*args, return_T=with_T)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)              # bit-identical repeats
    out = out.cpu().numpy()
    # only the order of the double sums differs: |fl(sum) - sum| <= (m - 1)
    # eps sum |terms| for any order of m terms, twice (two orders), with a
    # factor for the products and the nested sum of q: 8 n eps sum |terms|.
    # What the epilogue adds on top is one rounding of the scaled mean and,
    # for q recovered from the standard deviation, the roundings of
    # kss - q, the root and its square: a few eps of the value itself.
    bound_T = 8 * n * EPS * (np.abs(Kinv) @ np.abs(K64.T))
    bound_q = 8 * n * EPS * np.einsum('ij,ci,cj->c', np.abs(Kinv),
                                      np.abs(K64), np.abs(K64))
    bound_m = 8 * n * EPS * (np.abs(K64) @ np.abs(Ky))
    if with_T:
        assert torch.equal(T, T2)
        err = np.abs(T.cpu().numpy() - T_ref)
        print('T: error / bound', (err / bound_T).max())
        assert (err <= bound_T).all()
    else:
        assert T is None
    mean_ref = ystd * (K64 @ Ky) + ymean
    err = np.abs(out[:b] - mean_ref)
    bound = ystd * bound_m + 4 * EPS * np.abs(mean_ref)
    print('mean: error / bound', (err / bound).max())
    assert (err <= bound).all()
    # std through q: (std / ystd)^2 = kss - q
    q = kss - (out[b:] / ystd)**2
    err = np.abs(q - q_ref)
    bound = bound_q + 8 * EPS * np.abs(kss)
    print('q: error / bound', (err / bound).max())
    assert (err <= bound).all()
    # against the torch restatement too
    ref, _ = _posterior.posterior_torch(*args)
    np.testing.assert_allclose(out, ref.cpu().numpy(), rtol=1e-9, atol=1e-12)


def test_posterior_clips_and_keeps_nan():
    torch = _torch()
    from graphdot_amd.model.gaussian_process import _posterior
    Kinv, Ks, Ky, _ = _case(65, 3, 5)
    kss = np.array([-1.0, np.nan, 1e3])
    out, _ = _posterior.posterior(
        torch.from_numpy(Kinv).cuda(),
        torch.from_numpy(np.ascontiguousarray(Ks.T)).cuda().t(),
        torch.from_numpy(Ky).cuda(), torch.from_numpy(kss).cuda())
    std = out.cpu().numpy()[3:]
    assert std[0] == 0 and np.isnan(std[1]) and std[2] > 0
    with pytest.raises(TypeError):
        _posterior.posterior(torch.from_numpy(Kinv), torch.from_numpy(Ks),
                             torch.from_numpy(Ky), torch.from_numpy(kss))


# -- DevicePosterior against GaussianProcessRegressor.predict ---------------------------
def _graphs(n, seed=7165):
    import cases
    G = cases.config3_graphs(n, seed=seed)
    return np.asarray(G, dtype=object), cases.synthetic_energies(G)


def _kernel(real, normalized):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    knode, kedge, q = cases.config3_fit_kernels()
    k = MarginalizedGraphKernel(knode, kedge, q=q, backend=HIPBackend(
        real=real), ftol=1e-13 if real is np.float64 else 1e-8)
    return Normalization(k) if normalized else k


def _fit(real, normalized, normalize_y, n=90, masked=True):
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    G, y = _graphs(n + 12)
    y = list(y)
    if masked:
        y[3] = None
        y[40] = float('nan')
    gpr = GaussianProcessRegressor(
        _kernel(real, normalized), alpha=1e-2 if normalized else 1.0,
        normalize_y=normalize_y, device='cuda')
    gpr.fit(G[:n], y[:n])
    return gpr, G[n:]


@pytest.mark.parametrize('real', [np.float64, np.float32])
@pytest.mark.parametrize('normalized', [False, True])
@pytest.mark.parametrize('normalize_y', [False, True])
def test_device_posterior_equals_predict(real, normalized, normalize_y):
    _torch()
    from graphdot_amd.model.gaussian_process import DevicePosterior
    gpr, Z = _fit(real, normalized, normalize_y)
    post = DevicePosterior(gpr)
    assert post.available and len(post.X) == 88
    rtol = PREDICT_RTOL[real]
    for kw in ({}, dict(return_std=True), dict(return_cov=True)):
        got, ref = post.predict(Z, **kw), gpr.predict(Z, **kw)
        for name, a, r in zip(('mean', 'std' if 'return_std' in kw else 'cov'),
                              got if kw else (got,), ref if kw else (ref,)):
            assert a.dtype == np.float64 and a.shape == r.shape
            err = np.abs(a - r).max() / np.abs(r).max()
            print(f'{np.dtype(real).name} normalized={normalized} '
                  f'normalize_y={normalize_y} {name}: {err:.3e}')
            assert err <= rtol, (name, err)


def test_no_host_kernel_evaluation(monkeypatch):
    _torch()
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.model.gaussian_process import DevicePosterior
    posts = []
    for normalized in (False, True):
        gpr, Z = _fit(np.float64, normalized, True)
        posts.append((DevicePosterior(gpr), Z))

    def refuse(*args, **kwargs):
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', refuse)
        monkeypatch.setattr(cls, 'diag', refuse)
    for post, Z in posts:
        mean, std = post.predict(Z, return_std=True)
        assert np.isfinite(mean).all() and (std > 0).all()
        mean, cov = post.predict(Z[:4], return_cov=True)
        assert cov.shape == (4, 4)


def test_refit_rebuilds_the_device_copies():
    _torch()
    from graphdot_amd.model.gaussian_process import DevicePosterior
    gpr, Z = _fit(np.float64, True, False, masked=False)
    post = DevicePosterior(gpr)
    G, y = _graphs(50, seed=11)
    gpr.fit(G, y)
    got, ref = post.predict(Z, return_std=True), gpr.predict(Z, return_std=True)
    assert tuple(post.Kinv.shape) == (50, 50)
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-9)
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-7)


def test_uploaded_bytes_per_prediction(monkeypatch):
    """What ten predictions with fresh candidates upload, counted.  The
    solver's graph arena is cached under the identity of the whole graph list
    of a call, and a cross evaluation runs on candidates + training graphs:
    today every call assembles and uploads an arena of all N + b graphs again
    (printed below; DESIGN.md section 23 says what an upload of O(b) graphs
    needs and that it is left to a follow-up).  Asserted is what must hold
    either way: a prediction uploads no more than that arena and the job
    list -- nothing that grows with N^2, the inverse never again."""
    _torch()
    from graphdot_amd.hip import runtime
    from graphdot_amd.model.gaussian_process import DevicePosterior
    gpr, _ = _fit(np.float64, False, False, masked=False)
    post = DevicePosterior(gpr)
    b, calls = 5, 10
    Zs, _ = _graphs(b * (calls + 1), seed=99)
    post.predict(Zs[:b], return_std=True)              # code objects, pools
    sent = []
    upload = runtime.DeviceBuffer.upload

    def counting(self, array, *args, **kwargs):
        sent.append(np.asarray(array).nbytes)
        return upload(self, array, *args, **kwargs)
    monkeypatch.setattr(runtime.DeviceBuffer, 'upload', counting)
    backend = gpr.kernel.backend
    blobs = sum(len(backend._register_graph(g).blob)
                for g in list(Zs[:b]) + list(post.X))
    for k in range(1, calls + 1):
        post.predict(Zs[b * k:b * k + b], return_std=True)
    per_call = sum(sent) / calls
    print(f'uploaded per predict over {calls} calls: {per_call:.0f} bytes; '
          f'packed graphs of N + b: {blobs} bytes; of b: '
          f'{blobs * b // (b + len(post.X))} bytes; Kinv: '
          f'{post.Kinv.numel() * 8} bytes')
    assert per_call < 1.5 * blobs + 64 * b * len(post.X)


# -- seek on the device against seek on the host -----------------------------------------
class PoolDraws:
    """Children of a graph: `b` distinct graphs of a candidate pool."""

    def __init__(self, pool, b):
        self.pool, self.b = pool, b

    def __call__(self, node, rng):
        rest = [g for g in self.pool if g is not node.g]
        return [rest[i] for i in rng.choice(len(rest), size=self.b,
                                            replace=False)]


def _rows(tree, level=0):
    cols = ('self_mean', 'self_std', 'tree_mean', 'tree_std', 'score')
    for i in range(len(tree)):
        yield (level, id(tree.g[i]), int(tree.visits[i])), \
            [float(tree[c][i]) for c in cols]
        if tree.children[i] is not None:
            yield from _rows(tree.children[i], level + 1)


def seek_both(seed, maxiter=12):
    _torch()
    from graphdot_amd.model.tree_search import MCTSGraphTransformer
    gpr, _ = _fit(np.float64, True, True, n=90, masked=False)
    pool, _ = _graphs(40, seed=4242)
    rw = PoolDraws(list(pool), 4)
    target = float(np.quantile(gpr.y, 0.2))
    trees, gaps = {}, {'cuda': [], 'cpu': []}
    for device in ('cuda', 'cpu'):
        t = MCTSGraphTransformer(rw, gpr, precision=0.5 * float(np.std(gpr.y)),
                                 device=device)

        def recording(children, log=gaps[device]):
            # the best-to-second gap of the scores this selection compares
            s = np.sort(np.asarray(children.score, dtype=float))[::-1]
            if len(s) > 1:
                log.append(s[0] - s[1])
            return MCTSGraphTransformer._best_child(children)
        t._best_child = recording
        trees[device] = t.seek(pool[0], target, maxiter=maxiter,
                               return_tree=True, random_state=seed)
    return trees, gaps['cpu']


def test_seek_device_equals_host():
    trees, gaps = seek_both(SEEK_SEED)
    dev, host = list(_rows(trees['cuda'])), list(_rows(trees['cpu']))
    assert [k for k, _ in dev] == [k for k, _ in host]
    assert len(host) == 1 + 12 * 4
    a = np.array([v for _, v in dev])
    r = np.array([v for _, v in host])
    scale = np.abs(r).max(axis=0)
    err = (np.abs(a - r) / scale).max(axis=0)
    print('seek: relative differences per column', err)
    assert (err <= PREDICT_RTOL[np.float64]).all()
    gap = min(gaps)
    diff = np.abs(a[:, 4] - r[:, 4]).max()
    print(f'seek seed {SEEK_SEED}: smallest score gap {gap:.3e}, largest '
          f'score difference {diff:.3e}')
    assert gap >= 100 * diff


def test_auto_takes_the_device_for_many_candidates():
    _torch()
    from graphdot_amd.model.tree_search import MCTSGraphTransformer
    from graphdot_amd.model.tree_search.graph_transformer import _BySize
    gpr, _ = _fit(np.float64, True, True, n=260, masked=False)
    pool, _ = _graphs(40, seed=4242)
    trees = {}
    for device in ('auto', 'cpu'):
        t = MCTSGraphTransformer(PoolDraws(list(pool), 5), gpr, device=device,
                                 precision=0.5 * float(np.std(gpr.y)))
        trees[device] = t.seek(pool[0], float(np.quantile(gpr.y, 0.2)),
                               maxiter=3, return_tree=True, random_state=0)
        if device == 'auto':
            assert isinstance(t._predict[0], _BySize)
            assert t._predict[0].posterior.available
    a, r = list(_rows(trees['auto'])), list(_rows(trees['cpu']))
    assert [k for k, _ in a] == [k for k, _ in r]
    np.testing.assert_allclose([v for _, v in a], [v for _, v in r],
                               rtol=PREDICT_RTOL[np.float64], atol=1e-12)


# -- end to end: symbol strings ------------------------------------------------------------
class StringKernel:
    """A graph kernel on symbol strings: every string is a chain graph whose
    nodes carry the symbols."""

    def __init__(self, kernel):
        self.kernel, self._graphs = kernel, {}

    def graphs(self, S):
        import networkx as nx
        from graphdot_amd.graph import Graph
        out = []
        for s in S:
            s = str(s)
            if s not in self._graphs:
                g = nx.path_graph(len(s))
                for i, c in enumerate(s):
                    g.nodes[i]['symbol'] = ord(c) - ord('A')
                self._graphs[s] = Graph.from_networkx(g)
            out.append(self._graphs[s])
        return np.asarray(out, dtype=object)

    def __call__(self, X, Y=None, **kw):
        return self.kernel(self.graphs(X),
                           None if Y is None else self.graphs(Y), **kw)

    def diag(self, X, **kw):
        return self.kernel.diag(self.graphs(X), **kw)

    def device_gram(self, X, **kw):
        return self.kernel.device_gram(self.graphs(X), **kw)

    def device_cross_gram(self, X, Y, **kw):
        return self.kernel.device_cross_gram(self.graphs(X), self.graphs(Y),
                                             **kw)

    def device_diag(self, X, **kw):
        return self.kernel.device_diag(self.graphs(X), **kw)


def share_of_a(s):
    return s.count('A') / len(s)


def test_search_over_symbol_strings():
    _torch()
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.microkernel import (Constant, KroneckerDelta,
                                          TensorProduct)
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    from graphdot_amd.model.tree_search import (LookAheadSequenceRewriter,
                                                MCTSGraphTransformer)
    rng = np.random.default_rng(8)
    train = sorted({''.join(rng.choice(list('ABC'), size=rng.integers(4, 9)))
                    for _ in range(80)})
    kernel = StringKernel(Normalization(MarginalizedGraphKernel(
        TensorProduct(symbol=KroneckerDelta(0.3)), Constant(1.0), q=0.05,
        backend=HIPBackend(real=np.float64))))
    gpr = GaussianProcessRegressor(kernel, alpha=1e-3, normalize_y=True,
                                   device='cuda')
    gpr.fit(train, [share_of_a(s) for s in train])
    rw = LookAheadSequenceRewriter(n=1, b=4, min_edits=1, max_edits=3,
                                   random_state=0).fit(train)
    t = MCTSGraphTransformer(rw, gpr, precision=0.05, device='cuda')
    g0, target = 'BCBCBC', 0.75
    df = t.seek(g0, target, maxiter=40, random_state=2)
    assert t._predict[0].available
    best = df.iloc[0]
    print('best candidate', best['g'], 'true value', share_of_a(best['g']),
          'predicted', best['self_mean'], 'nodes', len(df))
    assert abs(share_of_a(best['g']) - target) < abs(share_of_a(g0) - target)
