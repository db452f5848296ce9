"""KernelHDBSCAN without a GPU: the definition of the model in numpy on the
stored matrix widened to double (the module text of model/clustering/
hdbscan.py, step by step, in the plainest way: all n (n - 1) / 2 edges sorted
for Kruskal's algorithm, members kept as lists), the data, the ``*_torch``
restatements of model/clustering/_mst.py on CPU tensors and the model with
``device='cpu'`` against the definition, the definition's consequences
against scikit-learn and SciPy, the model's interface, and the kernels' unit.
tests/test_hdbscan_gpu.py takes the definition and the data from here.

Every comparison with the definition is exact: the tree is unique under the
strict total order on edges, and everything after it is arithmetic on its n -
1 weights in one order.  scikit-learn is a yardstick only where the tree's
weights have no ties (``min_samples = 1``, off the grid): there its labels are
the model's up to renaming and its probabilities agree within 1e-12."""
import functools
import os
import warnings

import numpy as np
import pytest

#: (samples, centres)
SHAPES = [(96, 3), (200, 4)]
#: (min_samples, min_cluster_size)
SETTINGS = [(1, 5), (5, 8), (10, 10)]
METHODS = ['eom', 'leaf']
DTYPES = [np.float32, np.float64]


def _torch():
    import torch
    import graphdot_amd.model.clustering  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.array(a, order='C'))


# -- the data --------------------------------------------------------------------------
def points(n, c, seed, grid):
    r = np.random.default_rng(seed)
    cen = 2 * r.normal(size=(c, 5))
    lab = r.integers(0, c, n)
    X = cen[lab] + 0.25 * r.normal(size=(n, 5))
    X[:n // 10] = r.uniform(-4, 4, size=(n // 10, 5))
    if grid:
        X = np.round(2 * X) / 2
    return X


def gaussian(X, Y=None):
    Y = X if Y is None else Y
    return np.exp(-((X[:, None, :] - Y[None, :, :]) ** 2).sum(2) / 4.5)


@functools.lru_cache(maxsize=None)
def _data(n, c, grid, dtype):
    K = gaussian(points(n, c, n + c, grid)).astype(dtype)
    K.setflags(write=False)
    return K


def data(n, c, grid, dtype=np.float64):
    """The kernel matrix of a case as it is stored (read-only, shared)."""
    return _data(n, c, bool(grid), np.dtype(dtype))


def asymmetric(n=200, c=4, dtype=np.float64):
    """A matrix that is not symmetric in its last bits."""
    K = np.array(data(n, c, False, dtype))
    r = np.random.RandomState(3)
    K *= (1 + np.finfo(dtype).eps * r.randint(-2, 3, size=K.shape)
          * ~np.eye(n, dtype=bool)).astype(dtype)
    assert not np.array_equal(K, K.T)
    return K


# -- the definition --------------------------------------------------------------------
def define_d2(Ks, dq, dt):
    return np.maximum((dq[:, None] + dt[None, :])
                      - 2.0 * np.asarray(Ks, dtype=np.float64), 0.0)


def define_weights(K, min_samples):
    """(c2 (n,), w2 (n, n)): steps 1 to 3."""
    K = np.asarray(K, dtype=np.float64)
    n = len(K)
    d = np.diag(K).copy()
    D2 = define_d2(K, d, d)
    c2 = np.zeros(n)
    if min_samples > 1:
        E = D2.copy()
        np.fill_diagonal(E, np.inf)
        idx = np.argsort(E, axis=1, kind='stable')      # the order (d2, j)
        c2 = E[np.arange(n), idx[:, min_samples - 2]]
    return c2, np.maximum(np.minimum(D2, D2.T),
                          np.maximum(c2[:, None], c2[None, :]))


def define_tree(W2):
    """(w2, a, b) of step 4: Kruskal's algorithm over all edges in the order
    (w2, min, max)."""
    n = len(W2)
    iu, ju = np.triu_indices(n, 1)
    up = list(range(n))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x
    out = []
    for e in np.lexsort((ju, iu, W2[iu, ju])):
        i, j = int(iu[e]), int(ju[e])
        ri, rj = find(i), find(j)
        if ri != rj:
            up[rj] = ri
            out.append((W2[i, j], i, j))
    assert len(out) == n - 1
    return (np.array([e[0] for e in out]),
            np.array([e[1] for e in out], dtype=np.int64),
            np.array([e[2] for e in out], dtype=np.int64))


def inverse_root(w):
    return np.inf if w == 0.0 else 1.0 / np.sqrt(w)


class Definition:
    """Steps 5 to 8 (and what step 10 needs) from the tree's edges."""

    def __init__(self, n, w2, a, b, min_cluster_size, method):
        # 5. the hierarchy: node -> children, height, members
        node_of = np.arange(n)
        children, height = {}, {}
        members = {i: [i] for i in range(n)}
        following = n
        for w in np.unique(w2):
            link = {}

            def top(x):
                while link.get(x, x) != x:
                    x = link[x]
                return x
            met = set()
            for i, j in zip(a[w2 == w], b[w2 == w]):
                p, q = int(node_of[i]), int(node_of[j])
                met |= {p, q}
                p, q = top(p), top(q)
                assert p != q
                link[q] = p
            groups = {}
            for old in sorted(met):
                groups.setdefault(top(old), []).append(old)
            for olds in groups.values():
                assert len(olds) >= 2
                children[following] = olds
                height[following] = inverse_root(w)
                members[following] = sorted(
                    s for old in olds for s in members[old])
                node_of[members[following]] = following
                following += 1
        root = following - 1
        assert len(members[root]) == n
        # 6. condensing
        self.records = records = []
        self.birth, self.parent = {n: 0.0}, {n: None}
        work, born = [(root, n)], n + 1
        while work:
            node, cluster = work.pop(0)
            lam = height[node]
            large = [c for c in children[node]
                     if len(members[c]) >= min_cluster_size]
            for c in children[node]:
                if c not in large:
                    records += [(cluster, s, lam, 1) for s in members[c]]
            if len(large) >= 2:
                for c in large:
                    records.append((cluster, born, lam, len(members[c])))
                    self.birth[born], self.parent[born] = lam, cluster
                    work.append((c, born))
                    born += 1
            elif large:
                work.append((large[0], cluster))
        clusters = sorted(self.birth)
        below = {c: [d for d in clusters if self.parent[d] == c]
                 for c in clusters}
        # 7. stability and selection
        S = {c: sum((lam - self.birth[c]) * size
                    for p, _, lam, size in records if p == c)
             for c in clusters}
        self.top = {c: max([lam for p, _, lam, _ in records if p == c],
                           default=0.0) for c in clusters}
        if method == 'leaf':
            self.selected = {c: c != n and not below[c] for c in clusters}
        else:
            self.selected = {c: c != n for c in clusters}
            for c in reversed(clusters[1:]):
                rest = sum(S[d] for d in below[c])
                if rest > S[c]:
                    S[c] = rest
                    self.selected[c] = False
                else:
                    todo = list(below[c])
                    while todo:
                        d = todo.pop()
                        self.selected[d] = False
                        todo += below[d]
        # 8. labels and probabilities
        self.left = {s: p for p, s, _, _ in records if s < n}
        leave = {s: lam for _, s, lam, _ in records if s < n}
        assert sorted(self.left) == list(range(n))
        raw = [self.selected_above(self.left[s]) for s in range(n)]
        first = {}
        for s, c in enumerate(raw):
            if c is not None:
                first.setdefault(c, s)
        self.names = {c: k for k, c in enumerate(sorted(first,
                                                        key=first.get))}
        self.labels = np.array([-1 if c is None else self.names[c]
                                for c in raw])
        self.probabilities = np.array(
            [0.0 if c is None else self.strength(leave[s], c)
             for s, c in enumerate(raw)])

    def selected_above(self, c):
        while c is not None and not self.selected[c]:
            c = self.parent[c]
        return c

    def strength(self, lam, c):
        L = self.top[c]
        if L == 0.0 or np.isinf(lam):
            return 1.0
        return min(lam, L) / L

    def predict(self, w2, nearest):
        """Step 10 from the weight and the index of the nearest training
        sample in mutual reachability."""
        lam = inverse_root(w2)
        c = self.left[int(nearest)]
        while self.parent[c] is not None and self.birth[c] > lam:
            c = self.parent[c]
        c = self.selected_above(c)
        return (-1, 0.0) if c is None else (self.names[c],
                                            self.strength(lam, c))


class Case:
    def __init__(self, K, min_samples):
        self.K = K
        self.n = len(K)
        self.d = np.diag(K).astype(np.float64)
        self.c2, self.W2 = define_weights(K, min_samples)
        self.w2, self.a, self.b = define_tree(self.W2)

    @functools.lru_cache(maxsize=None)
    def model(self, min_cluster_size, method):
        return Definition(self.n, self.w2, self.a, self.b, min_cluster_size,
                          method)


@functools.lru_cache(maxsize=None)
def _case(n, c, grid, dtype, min_samples):
    return Case(data(n, c, grid, dtype), min_samples)


def case(n, c, grid, dtype, min_samples):
    return _case(n, c, bool(grid), np.dtype(dtype), min_samples)


def define_rows(W2, comp):
    """(w2 (n,), cand (n,)): per row the first minimum in the order (w2, j)
    among the columns of another component; (inf, -1) without one."""
    n = len(W2)
    out_w, out_j = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    for i in range(n):
        best = None
        for j in range(n):
            if comp[j] != comp[i] and (best is None
                                       or W2[i, j] < W2[i, best]):
                best = j
        if best is not None:
            out_w[i], out_j[i] = W2[i, best], best
    return out_w, out_j


def define_hook(w2, cand, comp):
    """(comp', components, edges {root: (w2, a, b)}) of one round behind the
    row pass."""
    n = len(comp)
    best = {}
    for i in range(n):
        if cand[i] >= 0:
            e = (w2[i], min(i, int(cand[i])), max(i, int(cand[i])))
            r = int(comp[i])
            best[r] = min(best.get(r, e), e)
    parent, edges = {r: r for r in set(comp.tolist())}, {}
    for r, e in best.items():
        other = int(comp[e[1]]) if comp[e[1]] != r else int(comp[e[2]])
        if best.get(other) == e and r < other:
            continue
        parent[r], edges[r] = other, e
    out = np.empty(n, dtype=np.int64)
    for i in range(n):
        r = int(comp[i])
        while parent[r] != r:
            r = parent[r]
        out[i] = r
    return out, len(set(out.tolist())), edges


def hand_made():
    """Two sets of hand-made candidates (w2, cand, comp): singletons with two
    mutual pairs and chains three steps deep; and components of several rows,
    rows of one component that tie in w2, a row without a candidate."""
    inf = np.inf
    return [
        (np.array([1.0, 1.0, 2.0, 3.0, 0.5, 0.5, 2.0, 4.0]),
         np.array([1, 0, 1, 2, 5, 4, 5, 6]), np.arange(8)),
        (np.array([1.0, 1.0, 1.0, 1.0, 2.0, 1.2, 1.5, 1.2, inf]),
         np.array([2, 3, 0, 1, 3, 7, 7, 5, -1]),
         np.array([0, 0, 2, 2, 4, 4, 4, 7, 4])),
    ]


def check_hook(got_comp, got_count, edges, w2, cand, comp):
    """Compare one round's outcome (numpy arrays) with `define_hook`."""
    want, count, chosen = define_hook(w2, cand, comp)
    assert np.array_equal(got_comp, want)
    assert int(got_count) == count
    ew, ea, eb = edges
    for r in range(len(comp)):
        if r in chosen:
            assert (ew[r], ea[r], eb[r]) == chosen[r], r
        else:
            assert np.isnan(ew[r]) and ea[r] == -1 and eb[r] == -1, r


def follows(labels, probabilities, got_labels, got_probabilities, perm):
    """Whether a result on the matrix permuted by `perm` (sample t of it is
    sample perm[t]) is the result on the matrix itself."""
    back_l = np.empty_like(got_labels)
    back_p = np.empty_like(got_probabilities)
    back_l[perm], back_p[perm] = got_labels, got_probabilities
    return np.array_equal(renumber(back_l), labels) \
        and np.array_equal(back_p, probabilities)


def renumber(labels):
    """Labels numbered by smallest member."""
    out = np.full(len(labels), -1, dtype=np.int64)
    seen = {}
    for s, c in enumerate(labels.tolist()):
        if c >= 0:
            out[s] = seen.setdefault(c, len(seen))
    return out


def same_partition(x, y):
    """Equal up to renaming, the noise the same: ARI exactly 1."""
    from sklearn.metrics import adjusted_rand_score
    return np.array_equal(x < 0, y < 0) \
        and np.array_equal(renumber(x), renumber(y)) \
        and adjusted_rand_score(x, y) == 1.0


def fit(K, min_samples, min_cluster_size, method='eom'):
    from graphdot_amd.model.clustering import KernelHDBSCAN
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        return KernelHDBSCAN('precomputed', min_cluster_size, min_samples,
                             method, device='cpu').fit(np.array(K))


def check_model(model, c, min_cluster_size, method):
    """The fitted model against the definition of its case, exactly."""
    want = c.model(min_cluster_size, method)
    tree = model.minimum_spanning_tree_
    assert np.array_equal(tree[:, 0], c.a) and np.array_equal(tree[:, 1], c.b)
    assert np.array_equal(tree[:, 2], np.sqrt(c.w2))
    assert np.array_equal(model.core_distances_, np.sqrt(c.c2))
    assert np.array_equal(model.labels_, want.labels)
    assert np.array_equal(model.probabilities_, want.probabilities)
    assert model.n_clusters_ == want.labels.max() + 1
    records = model.condensed_tree_
    assert sorted(zip(records['lambda_val'], records['child_size'])) \
        == sorted((lam, size) for _, _, lam, size in want.records)


# -- 1. against the definition -----------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('grid', [False, True])
@pytest.mark.parametrize('min_samples, min_cluster_size', SETTINGS)
@pytest.mark.parametrize('n, c', SHAPES)
def test_model_equals_the_definition(n, c, min_samples, min_cluster_size,
                                     grid, dtype):
    ca = case(n, c, grid, dtype, min_samples)
    for method in METHODS:
        model = fit(ca.K, min_samples, min_cluster_size, method)
        check_model(model, ca, min_cluster_size, method)
        assert model.last_timing['fused'] is False
        assert model.last_timing['adopted'] is False
    assert model.labels_.max() >= 1        # (the case has clusters to find)


@pytest.mark.parametrize('dtype', DTYPES)
def test_model_on_a_matrix_that_is_not_symmetric(dtype):
    K = asymmetric(dtype=dtype)
    for min_samples, size in SETTINGS:
        ca = Case(K, min_samples)
        assert np.array_equal(ca.W2, ca.W2.T)
        check_model(fit(K, min_samples, size), ca, size, 'eom')
        # (the lists, and with them c2, are those of the rows as stored)
        check_model(fit(K.T, min_samples, size), Case(K.T, min_samples),
                    size, 'eom')


@pytest.mark.parametrize('grid', [False, True])
@pytest.mark.parametrize('min_samples', [1, 5])
def test_torch_restatements_equal_the_definition(min_samples, grid):
    """A first round and a round in the middle of a run; the hand-made
    candidates."""
    torch = _torch()
    from graphdot_amd.model.clustering import _mst
    ca = case(96, 3, grid, np.float32, min_samples)
    n = ca.n
    comp = np.arange(n)
    for _ in range(2):
        w2, cand = define_rows(ca.W2, comp)
        got = _mst.rows_torch(_t(ca.K), _t(ca.d), _t(ca.c2),
                              _t(comp.astype(np.int32)))
        assert np.array_equal(got[0].numpy(), w2)
        assert np.array_equal(got[1].numpy(), cand) and int(got[2]) == 0
        edges = _mst.new_edges(n, torch.device('cpu'))
        after, count = _mst.hook_torch(got[0], got[1],
                                       _t(comp.astype(np.int32)), edges)
        check_hook(after.numpy(), count.sum(), [e.numpy() for e in edges],
                   w2, cand, comp)
        comp = after.numpy().astype(np.int64)
    assert 1 < len(set(comp.tolist())) <= n // 4


def test_hook_torch_on_hand_made_candidates():
    torch = _torch()
    from graphdot_amd.model.clustering import _mst
    for w2, cand, comp in hand_made():
        edges = _mst.new_edges(len(comp), torch.device('cpu'))
        after, count = _mst.hook_torch(
            _t(w2), _t(cand.astype(np.int32)), _t(comp.astype(np.int32)),
            edges)
        check_hook(after.numpy(), count.sum(), [e.numpy() for e in edges],
                   w2, cand, comp)
        assert int(count.sum()) == 2


def test_cross_rows_torch_and_approximate_predict():
    from graphdot_amd.model.clustering import KernelHDBSCAN
    n, c = 200, 4
    X = points(n, c, n + c, False)
    Q = np.concatenate((points(40, c, n + c, False)[::3], X[100:103]))
    K, Ks = gaussian(X), gaussian(Q, X)
    dq = np.ones(len(Q))
    for min_samples, size in SETTINGS:
        ca = Case(K, min_samples)
        for method in METHODS:
            model = KernelHDBSCAN('precomputed', size, min_samples, method,
                                  device='cpu').fit(K)
            labels, strengths = model.approximate_predict(Ks, diag=dq)
            want = define_predict(ca, ca.model(size, method), Ks, dq,
                                  min_samples)
            assert np.array_equal(labels, want[0])
            assert np.array_equal(strengths, want[1])
            if min_samples == 1:
                # its own nearest sample at lambda = inf: where it left
                assert np.array_equal(labels[-3:], model.labels_[100:103])
            assert (labels >= 0).any() and (strengths[labels < 0] == 0).all()


def define_predict(ca, definition, Ks, dq, min_samples):
    """(labels, strengths) of step 10."""
    D2 = define_d2(Ks, dq, ca.d)
    cq = np.zeros(len(D2))
    if min_samples > 1:
        cq = np.sort(D2, axis=1)[:, min_samples - 2]
    W2 = np.maximum(D2, np.maximum(cq[:, None], ca.c2[None, :]))
    nearest = np.argmin(W2, axis=1)          # (the first minimum)
    out = [definition.predict(W2[q, j], j) for q, j in enumerate(nearest)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]))


# -- 2. against scikit-learn ---------------------------------------------------------------
def _distances(ca):
    """The matrix scikit-learn takes: sqrt of the symmetrised d2."""
    D2 = define_d2(ca.K, ca.d, ca.d)
    return np.sqrt(np.minimum(D2, D2.T))


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('n, c', SHAPES)
def test_labels_and_probabilities_equal_scikit_learn_without_ties(n, c,
                                                                  method):
    from sklearn.cluster import HDBSCAN
    ca = case(n, c, False, np.float64, 1)
    assert len(np.unique(ca.w2)) == n - 1          # no ties in the tree
    model = fit(ca.K, 1, 5, method)
    theirs = HDBSCAN(min_cluster_size=5, min_samples=1, metric='precomputed',
                     cluster_selection_method=method).fit(_distances(ca))
    assert same_partition(model.labels_, theirs.labels_)
    assert model.n_clusters_ == theirs.labels_.max() + 1 >= 2
    assert np.abs(model.probabilities_ - theirs.probabilities_).max() <= 1e-12


@pytest.mark.parametrize('grid', [False, True])
@pytest.mark.parametrize('min_samples, min_cluster_size', SETTINGS)
@pytest.mark.parametrize('n, c', SHAPES)
def test_dbscan_clustering_equals_scikit_learn(n, c, min_samples,
                                               min_cluster_size, grid):
    """Ties included, at cuts that are themselves edge weights (and between
    and beyond them)."""
    from sklearn.cluster import HDBSCAN
    ca = case(n, c, grid, np.float64, min_samples)
    model = fit(ca.K, min_samples, min_cluster_size)
    theirs = HDBSCAN(min_cluster_size=min_cluster_size,
                     min_samples=min_samples,
                     metric='precomputed').fit(_distances(ca))
    lengths = np.unique(model.minimum_spanning_tree_[:, 2])
    cuts = [lengths[len(lengths) * q // 8] for q in range(8)] \
        + [lengths[-1], 2 * lengths[-1], 0.5 * (lengths[-2] + lengths[-1])]
    for cut in cuts:
        for size in (min_cluster_size, 2):
            got = model.dbscan_clustering(cut, size)
            want = theirs.dbscan_clustering(cut, size)
            assert same_partition(got, want), (cut, size)
    assert np.array_equal(model.dbscan_clustering(cuts[4]),
                          model.dbscan_clustering(cuts[4], min_cluster_size))


# -- 3. against SciPy ----------------------------------------------------------------------
@pytest.mark.parametrize('grid', [False, True])
@pytest.mark.parametrize('min_samples, min_cluster_size', SETTINGS)
@pytest.mark.parametrize('n, c', SHAPES)
def test_weights_equal_scipy(n, c, min_samples, min_cluster_size, grid):
    from scipy.cluster.hierarchy import linkage
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    from scipy.spatial.distance import squareform
    ca = case(n, c, grid, np.float64, min_samples)
    model = fit(ca.K, min_samples, min_cluster_size)
    W = np.sqrt(ca.W2)
    np.fill_diagonal(W, 0.0)
    # (a sparse matrix with every edge stored: a length of 0 between
    # duplicates is an edge, where a dense 0 would be none; the tree SciPy
    # returns has used those edges and does not list them)
    iu, ju = np.triu_indices(n, 1)
    graph = csr_matrix((W[iu, ju], (iu, ju)), shape=(n, n))
    theirs = minimum_spanning_tree(graph).data
    assert (theirs > 0.0).all()
    assert len(theirs) == n - 1 - (ca.w2 == 0.0).sum()
    assert grid or len(theirs) == n - 1
    assert np.array_equal(
        np.concatenate((np.zeros(n - 1 - len(theirs)), np.sort(theirs))),
        model.minimum_spanning_tree_[:, 2])
    Z = model.single_linkage_tree_
    assert Z.shape == (n - 1, 4) and Z[-1, 3] == n
    assert np.array_equal(Z[:, 2], linkage(squareform(W), 'single')[:, 2])
    assert np.array_equal(Z[:, 2], model.minimum_spanning_tree_[:, 2])
    # a valid scipy linkage: every id is used once, and before it is made
    ids = Z[:, :2].astype(int)
    assert sorted(ids.ravel().tolist()) == list(range(2 * n - 2))
    assert (ids < n + np.arange(n - 1)[:, None]).all()
    assert (ids[:, 0] < ids[:, 1]).all()


# -- 4. invariance -------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [False, True])
@pytest.mark.parametrize('min_samples, min_cluster_size', SETTINGS)
@pytest.mark.parametrize('n, c', SHAPES)
def test_result_follows_a_permutation_of_the_samples(
        n, c, min_samples, min_cluster_size, grid):
    ca = case(n, c, grid, np.float64, min_samples)
    perm = np.random.RandomState(n + min_samples).permutation(n)
    Kp = ca.K[np.ix_(perm, perm)]
    for method in METHODS:
        want = ca.model(min_cluster_size, method)
        got = fit(Kp, min_samples, min_cluster_size, method)
        assert follows(want.labels, want.probabilities, got.labels_,
                       got.probabilities_, perm)
        back = np.empty(n)
        back[perm] = got.core_distances_
        assert np.array_equal(back, np.sqrt(ca.c2))
        assert np.array_equal(got.minimum_spanning_tree_[:, 2],
                              np.sqrt(ca.w2))


# -- 5. edge cases -------------------------------------------------------------------------
def test_two_samples():
    K = np.array([[1.0, 0.5], [0.5, 1.0]])
    for min_samples in (1, 2):
        model = fit(K, min_samples, 2)
        assert model.minimum_spanning_tree_.tolist() == [[0.0, 1.0, 1.0]]
        assert model.labels_.tolist() == [-1, -1]
        assert model.probabilities_.tolist() == [0.0, 0.0]
        assert model.n_clusters_ == 0
        assert model.single_linkage_tree_.tolist() == [[0.0, 1.0, 1.0, 2.0]]
        assert model.dbscan_clustering(1.0, 2).tolist() == [-1, -1]
        assert model.dbscan_clustering(1.5, 2).tolist() == [0, 0]


def test_all_equal_matrix_gives_the_star():
    n = 37
    for min_samples in (1, 4):
        model = fit(np.full((n, n), 0.25), min_samples, 5)
        tree = model.minimum_spanning_tree_
        assert np.array_equal(tree[:, 0], np.zeros(n - 1))
        assert np.array_equal(tree[:, 1], np.arange(1, n))
        assert np.array_equal(tree[:, 2], np.zeros(n - 1))
        # one node holds everything: the root, which is never a cluster
        assert np.array_equal(model.labels_, np.full(n, -1))
        assert np.array_equal(model.probabilities_, np.zeros(n))
        assert np.isinf(model.condensed_tree_['lambda_val']).all()


def duplicates(group):
    """Two clusters of 20 and `group` copies of one point between them."""
    r = np.random.RandomState(group)
    X = np.concatenate((r.normal(size=(20, 3)) * 0.2,
                        r.normal(size=(20, 3)) * 0.2 + 4.0,
                        np.full((group, 3), 2.0)))
    return gaussian(X)


def test_duplicates_below_min_cluster_size():
    K = duplicates(3)
    for min_samples in (1, 3, 5):
        ca = Case(K, min_samples)
        for method in METHODS:
            model = fit(K, min_samples, 5, method)
            check_model(model, ca, 5, method)
            assert np.all(model.labels_[-3:] == model.labels_[-1])
            assert np.all(model.probabilities_[-3:]
                          == model.probabilities_[-1])
            assert np.isfinite(model.probabilities_).all()
    assert model.core_distances_[-1] > 0.0           # (min_samples = 5)


def test_duplicates_that_are_a_cluster():
    """`min_cluster_size` copies of a point: they meet at lambda = inf."""
    K = duplicates(5)
    for min_samples in (1, 5):
        ca = Case(K, min_samples)
        for method in METHODS:
            model = fit(K, min_samples, 5, method)      # (no warning)
            check_model(model, ca, 5, method)
            assert model.n_clusters_ == 3
            assert np.all(model.labels_[-5:] == 2)
            assert np.all(model.probabilities_[-5:] == 1.0)
            assert np.all(model.core_distances_[-5:] == 0.0)
            assert np.isfinite(model.probabilities_).all()
            assert np.isinf(model.condensed_tree_['lambda_val']).sum() == 5
            labels, strengths = model.approximate_predict(
                K[-1:], diag=np.ones(1))
            assert labels.tolist() == [2] and strengths.tolist() == [1.0]


def test_value_errors():
    from graphdot_amd.model.clustering import KernelHDBSCAN
    K = np.array(data(96, 3, False))
    for kwargs in ({'min_cluster_size': 1}, {'min_cluster_size': 2.5},
                   {'min_cluster_size': True}, {'min_samples': 0},
                   {'min_samples': 1.5},
                   {'cluster_selection_method': 'both'}):
        with pytest.raises(ValueError, match=next(iter(kwargs))):
            KernelHDBSCAN('precomputed', **kwargs)
    for kwargs in ({'min_cluster_size': 97},
                   {'min_cluster_size': 5, 'min_samples': 97}):
        with pytest.raises(ValueError, match='96 samples'):
            KernelHDBSCAN('precomputed', device='cpu', **kwargs).fit(K)
    with pytest.raises(ValueError, match='square'):
        KernelHDBSCAN('precomputed', device='cpu').fit(K[:5])
    model = KernelHDBSCAN('precomputed', device='cpu')
    for call in (lambda: model.single_linkage_tree_,
                 lambda: model.dbscan_clustering(1.0),
                 lambda: model.approximate_predict(K[:2], diag=np.ones(2))):
        with pytest.raises(RuntimeError, match='before fit'):
            call()
    model.fit(K)
    with pytest.raises(ValueError, match='diag'):
        model.approximate_predict(K[:2])
    with pytest.raises(ValueError, match=r'diag: \(2,\)'):
        model.approximate_predict(K[:2], diag=np.ones(3))
    with pytest.raises(ValueError, match='shape'):
        model.approximate_predict(K[:2, :4], diag=np.ones(2))
    for min_samples in (1, 5):
        for at in ((1, 3), (3, 1), (7, 7)):
            bad = np.array(K)
            bad[at] = np.nan if at[0] < 7 else np.inf
            with pytest.raises(ValueError, match='not finite'):
                KernelHDBSCAN('precomputed', 5, min_samples,
                              device='cpu').fit(bad)
        model = KernelHDBSCAN('precomputed', 5, min_samples,
                              device='cpu').fit(K)
        bad = np.array(K[:2])
        bad[1, 3] = np.inf
        with pytest.raises(ValueError, match='not finite'):
            model.approximate_predict(bad, diag=np.ones(2))
    before = np.array(K)
    KernelHDBSCAN('precomputed', device='cpu').fit(K)
    assert np.array_equal(K, before)


def test_defaults_and_fit_predict():
    from graphdot_amd.model.clustering import KernelHDBSCAN
    K = np.array(data(96, 3, False))
    model = KernelHDBSCAN('precomputed', device='cpu')
    assert model.min_cluster_size == 5 and model.min_samples is None
    assert model.cluster_selection_method == 'eom'
    labels = model.fit_predict(K)
    # min_samples=None means min_cluster_size
    assert np.array_equal(labels, fit(K, 5, 5).labels_)
    assert np.array_equal(model.core_distances_, fit(K, 5, 5).core_distances_)
    assert sorted(model.last_timing) == ['adopted', 'fused', 'host', 'kernel',
                                         'tree']
    assert model.condensed_tree_.dtype.names == (
        'parent', 'child', 'lambda_val', 'child_size')
    for name in ('alpha', 'cluster_selection_epsilon', 'max_cluster_size',
                 'allow_single_cluster', 'store_centers'):
        assert name in KernelHDBSCAN.__doc__


def test_sixty_six_neighbours_take_the_torch_chain():
    from graphdot_amd.model.clustering import _mst
    from graphdot_amd.model.neighbors import _knn
    assert _knn.K_MOST == 64
    ca = case(200, 4, False, np.float64, 66)
    model = fit(ca.K, 66, 10)
    check_model(model, ca, 10, 'eom')
    assert model.last_timing['fused'] is False
    # (what declines on a GPU: the search of more than 64 neighbours)
    assert _knn._declines(_t(ca.K), 65) is not None
    assert _mst.rounds_most(2) == 1 and _mst.rounds_most(200) == 8
    assert _mst.rounds_most(256) == 8 and _mst.rounds_most(257) == 9
    assert [_mst.jumps_for(m) for m in (1, 2, 8, 9, 64, 65, 4000)] \
        == [0, 1, 1, 2, 2, 3, 4]


def test_model_on_graphs_leaves_the_kernel_alone():
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.model.clustering import KernelHDBSCAN
    graphs = np.asarray(cases.config3_graphs(12, seed=3), dtype=object)
    knode, kedge, q = cases.config3_kernels()
    kernel = MarginalizedGraphKernel(knode, kedge, q=q,
                                     backend=OracleBackend())
    # (the oracle backend solves pairs only: the self-similarities of Z as
    # the diagonal of its Gram matrix, as in test_neighbors.py)
    kernel.diag = lambda Z: kernel(Z).diagonal()
    theta0 = np.array(kernel.theta)
    K = np.asarray(kernel(graphs), dtype=np.float64)
    model = KernelHDBSCAN(kernel, 3, 2, device='cpu')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        model.fit(graphs)
    assert np.array_equal(kernel.theta, theta0)
    assert model.last_timing['adopted'] is False
    assert model.last_timing['fused'] is False
    pre = KernelHDBSCAN('precomputed', 3, 2, device='cpu').fit(K)
    assert np.array_equal(model.labels_, pre.labels_)
    assert np.array_equal(model.probabilities_, pre.probabilities_)
    assert np.array_equal(model.minimum_spanning_tree_,
                          pre.minimum_spanning_tree_)
    check_model(model, Case(K, 2), 3, 'eom')
    new = graphs[:3]
    Ks = np.asarray(kernel(new, graphs), dtype=np.float64)
    dq = np.asarray(kernel.diag(new), dtype=np.float64)
    got, want = model.approximate_predict(new), \
        pre.approximate_predict(Ks, diag=dq)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(kernel.theta, theta0)


# -- 6. the kernels' unit ------------------------------------------------------------------
def test_model_unit_compiles_for_gfx950():
    from graphdot_amd.hip import jit, source_module
    from graphdot_amd.model.clustering import _mst
    assert 'mst' in source_module.MODEL_UNITS
    for older in (source_module.STATIC, source_module.TEXT_UNITS,
                  source_module.FILE_UNITS):
        assert 'mst' not in older
    assert not any('mst' in p for p in source_module.STATIC_SOURCES)
    module = source_module.MODEL_UNITS['mst']
    path = os.path.join(os.path.dirname(source_module.__file__), '..',
                        'model', 'clustering', 'mst.h')
    with open(path) as f:
        assert module.path is None and module.source == f.read()
    assert module.flags == source_module.DENSE_FLAGS
    assert '#include "dense_reduce.h"' in module.source
    # the only atomics are integer minima
    assert module.source.count('atomicMin(') == 2
    assert 'atomicAdd' not in module.source and 'sqrt(' not in module.source
    assert _mst._module is module
    image = jit.load_image(module.precompile())
    names = jit.entry_points(module.source)
    assert sorted(names) == sorted(_mst.ENTRY_POINTS) and len(names) == 8
    for kernel in names:
        assert kernel.encode() in image, kernel


def test_the_file_keys_its_own_unit_alone(tmp_path, monkeypatch):
    """An edit of model/clustering/mst.h gives its unit a new cache key and
    no other source: the file is no header of csrc/device."""
    import shutil
    from graphdot_amd.hip import jit, source_module
    from graphdot_amd.hip.source_module import (FILE_UNITS, MODEL_UNITS,
                                                STATIC, TEXT_UNITS)
    relative = source_module.MODEL_UNIT_SOURCES['mst']
    assert relative == 'model/clustering/mst.h'
    assert not os.path.exists(os.path.join(jit.DEVICE_INCLUDE, 'mst.h'))
    others = [MODEL_UNITS['geodesic'], FILE_UNITS['tsne'], TEXT_UNITS['knn'],
              STATIC['lloyd.hip'], STATIC['mmd.hip']]

    def keys():
        monkeypatch.setattr(jit, '_hdr_digest', None)
        unit = source_module.SourceModule(source=source_module._text(relative))
        return (unit.key,) + tuple(jit.cache_key(o.source, o.flags)
                                   for o in others)
    before = keys()
    assert before == (MODEL_UNITS['mst'].key,) + tuple(o.key for o in others)
    copy = tmp_path / 'package'
    os.makedirs(copy / 'model')
    shutil.copytree(os.path.join(source_module._PACKAGE, 'model',
                                 'clustering'), copy / 'model' / 'clustering')
    monkeypatch.setattr(source_module, '_PACKAGE', str(copy))
    assert keys() == before
    with open(copy / relative, 'a') as f:
        f.write('// edited\n')
    edited = keys()
    assert edited[0] != before[0] and edited[1:] == before[1:]
