"""HDBSCAN on top of the kernel protocol: find the groups of a library of
graphs, say how many there are, and leave the odd ones out.

The reference has no such model.  scikit-learn's ``HDBSCAN(metric=
'precomputed')`` sorts the edges of its tree with an unstable sort and merges
two components at a time, so its labels depend on the order of the samples as
soon as two mutual-reachability distances are equal -- and kernel matrices of
molecules are full of exact ties.  This model is therefore defined on the
hierarchy of Campello et al. (2013), in which all components that meet at one
height merge at once; where the tree's weights have no
ties it equals scikit-learn's:

1.  ``d2(i, j) = max(0, (diag_i + diag_j) - 2 K[i, j])`` in double and ``s(i,
    j) = min(d2(i, j), d2(j, i))``.
2.  ``c2_i = 0`` if ``min_samples == 1``; otherwise the entry of rank
    ``min_samples - 1`` in row i's list of the `exclude_self` search of the
    neighbour models, which is in the order ``(d2, j)``.  `core_distances_`
    is ``sqrt(c2)``.
3.  ``w2(i, j) = max(c2_i, c2_j, s(i, j))``.  Everything on the device works
    on w2; roots are taken on the host.
4.  The tree is the one spanning tree that is minimal under the strict total
    order ``(w2, min(i, j), max(i, j))`` on edges: Kruskal's algorithm run in
    that order.  `minimum_spanning_tree_` lists its edges in that order.
5.  For each distinct w2 among the tree's edges, ascending, all edges of that
    weight are contracted at once: every component formed from m >= 2 older
    ones is one node with m children, at ``lambda = 1 / sqrt(w2)`` (inf at 0).
6.  Condensing, from the root (cluster n, born at lambda 0): at a node, the
    samples of every child smaller than `min_cluster_size` leave the current
    cluster at the node's lambda.  If two or more children are large enough,
    each becomes a new cluster born at that lambda; if one is, it continues
    the current cluster; if none is, the cluster ends.
7.  ``S(C)`` is the sum over the records that leave C of ``(lambda -
    birth(C)) * size``.  'eom' works bottom-up: if the children's stabilities
    sum to more than S(C), C takes that sum and is not selected; else C is
    selected and all its descendants are deselected; the root is never
    selected.  'leaf' selects the clusters without child clusters.
8.  Selected clusters are numbered by their smallest member.  A sample's
    label is the selected cluster among the cluster it left and that
    cluster's ancestors, else -1.  ``probabilities_ = min(lambda_leave, L) /
    L`` with L the largest lambda of C's own records; 1 where L = 0 or
    lambda_leave is infinite, 0 for noise.  (scikit-learn's rules, restated on
    the multi-way tree.)
9.  ``dbscan_clustering(cut, m)``: the components of the tree's edges with
    ``sqrt(w2) < cut`` (strict, as scikit-learn); those of at least m members
    are numbered by smallest member, the rest are -1.
10. `approximate_predict` of a query q: ``c2_q`` is the entry of rank
    ``min_samples - 1`` of its list against the training set, nothing left
    out, or 0; ``j*`` minimises ``(max(c2_q, c2_j, d2(q, j)), j)`` and
    ``lambda_q`` is 1 / sqrt of that weight.  Start at the cluster j* left and
    climb while the cluster's birth is above lambda_q; the label is the
    selected cluster at or above that point, else -1, and the strength is
    ``min(lambda_q, L) / L`` under the rules of 8.
11. `single_linkage_tree_` is the binary scipy Z of Kruskal's order, for
    plotting only: nothing above is derived from it.

Out of scope: scikit-learn's `alpha`, `cluster_selection_epsilon`,
`max_cluster_size`, `allow_single_cluster` (the root is never a cluster) and
`store_centers`.

On the GPU, for a kernel with `device_gram` or a CUDA tensor, the matrix is
used where it lies (float or double, either layout); the lists come from the
kernels of csrc/device/knn.h and the tree from Boruvka rounds of the kernels
of mst.h on the implicit graph: neither d2 nor w2 is written as a matrix, one
word pair is downloaded per round and the n - 1 edges once.  Steps 5 to 9 are
host work on n - 1 edges.  Anywhere else, and for more than 64 neighbours
(``min_samples > 65``), the same chain runs through torch (`_mst.*_torch`)
and gives the same edges bit for bit."""
import time
import numpy as np
from .._matrices import KernelMatrices
from ..neighbors import device_lists
from . import _mst

METHODS = ('eom', 'leaf')
CONDENSED = np.dtype([('parent', np.int64), ('child', np.int64),
                      ('lambda_val', np.float64), ('child_size', np.int64)])


def _torch():
    import torch
    return torch


def _count(name, k, least=1):
    if isinstance(k, bool) or int(k) != k or k < least:
        raise ValueError(f'{name}: an integer of at least {least} expected, '
                         f'got {k}')
    return int(k)


def _inverse_root(w2):
    """``1 / sqrt(w2)``, inf at 0."""
    w2 = np.asarray(w2, dtype=np.float64)
    lam = np.full(w2.shape, np.inf)
    pos = w2 > 0.0
    lam[pos] = 1.0 / np.sqrt(w2[pos])
    return lam


class _Forest:
    """Union-find over n samples with path halving."""

    def __init__(self, n):
        self.up = list(range(n))

    def find(self, x):
        up = self.up
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x


# -- steps 5 to 8 and 11 on the host ---------------------------------------------------
def _hierarchy(n, w2, a, b):
    """(kids, lam, size, least) of the multi-way tree of step 5: node ids
    below n are samples; node n + t has the children ``kids[t]`` (ordered by
    their smallest member) and the height ``lam[t]``; size and least (the
    smallest member) are per node id.  The last node is the root."""
    forest = _Forest(n)
    node = list(range(n))          # union-find root -> node id
    size, least = [1] * n, list(range(n))
    kids, lam = [], []
    heights = _inverse_root(w2)
    m, t = len(w2), 0
    while t < m:
        u = t + 1
        while u < m and w2[u] == w2[t]:
            u += 1
        ends = [(forest.find(int(a[e])), forest.find(int(b[e])))
                for e in range(t, u)]
        for ra, rb in ends:
            ra, rb = forest.find(ra), forest.find(rb)
            if ra != rb:
                forest.up[max(ra, rb)] = min(ra, rb)
        met = {}
        for pair in ends:
            for r in pair:
                met.setdefault(forest.find(r), set()).add(r)
        for new in sorted(met):
            children = sorted((node[r] for r in met[new]),
                              key=least.__getitem__)
            node[new] = n + len(kids)
            kids.append(children)
            lam.append(heights[t])
            size.append(sum(size[c] for c in children))
            least.append(min(least[c] for c in children))
        t = u
    return kids, lam, size, least


def _leaf_order(n, kids):
    """(order, lo, hi): the samples below node id x are ``order[lo[x]:
    hi[x]]``."""
    total = n + len(kids)
    lo, hi = [0] * total, [0] * total
    order = []
    stack = [(total - 1, False)]
    while stack:
        x, closing = stack.pop()
        if closing:
            hi[x] = len(order)
        elif x < n:
            lo[x] = len(order)
            order.append(x)
            hi[x] = len(order)
        else:
            lo[x] = len(order)
            stack.append((x, True))
            for c in reversed(kids[x - n]):
                stack.append((c, False))
    return order, lo, hi


def _condense(n, kids, lam, size, min_cluster_size):
    """The records of step 6 as a `CONDENSED` array: clusters are numbered
    from n (the root) in the order they are born."""
    order, lo, hi = _leaf_order(n, kids)
    records = []
    born = n + 1
    stack = [(n + len(kids) - 1, n)]
    while stack:
        x, cluster = stack.pop()
        height = lam[x - n]
        large = []
        for c in kids[x - n]:
            if size[c] >= min_cluster_size:
                large.append(c)
            else:
                records.extend((cluster, s, height, 1)
                               for s in order[lo[c]:hi[c]])
        if len(large) == 1:
            stack.append((large[0], cluster))
        elif large:
            for c in large:
                records.append((cluster, born, height, size[c]))
                stack.append((c, born))
                born += 1
    return np.array(records, dtype=CONDENSED)


def _select(n, tree, method):
    """(selected (clusters,) bool, up (clusters,) the parent cluster's
    offset, -1 for the root, birth, top): step 7, clusters by offset ``id -
    n``; top is L of step 8."""
    count = int(max(tree['parent'].max(), tree['child'].max())) - n + 1
    is_cluster = tree['child'] >= n
    up = np.full(count, -1, dtype=np.int64)
    birth = np.zeros(count)
    up[tree['child'][is_cluster] - n] = tree['parent'][is_cluster] - n
    birth[tree['child'][is_cluster] - n] = tree['lambda_val'][is_cluster]
    at = tree['parent'] - n
    stability = np.zeros(count)
    np.add.at(stability, at,
              (tree['lambda_val'] - birth[at]) * tree['child_size'])
    top = np.zeros(count)
    np.maximum.at(top, at, tree['lambda_val'])
    below = [[] for _ in range(count)]
    for c in range(1, count):
        below[up[c]].append(c)
    selected = np.ones(count, dtype=bool)
    selected[0] = False
    if method == 'leaf':
        for c in range(count):
            selected[c] = c > 0 and not below[c]
        return selected, up, birth, top
    for c in range(count - 1, 0, -1):
        if not below[c]:
            continue
        rest = sum(stability[d] for d in below[c])
        if rest > stability[c]:
            stability[c] = rest
            selected[c] = False
        else:
            stack = list(below[c])
            while stack:
                d = stack.pop()
                selected[d] = False
                stack.extend(below[d])
    return selected, up, birth, top


def _strength(lam, top):
    """``min(lam, top) / top``; 1 where top is 0 or lam infinite."""
    lam, top = np.broadcast_arrays(np.asarray(lam, dtype=np.float64),
                                   np.asarray(top, dtype=np.float64))
    out = np.ones(lam.shape)
    plain = (top != 0.0) & np.isfinite(lam)
    out[plain] = np.minimum(lam[plain], top[plain]) / top[plain]
    return out


def _number_by_least(raw, least_size=1):
    """Labels 0, 1, ... for the values of `raw` that are not negative and
    have at least `least_size` members, in the order of their smallest
    member; -1 for the rest."""
    out = np.full(raw.shape, -1, dtype=np.int64)
    values, first, counts = np.unique(raw, return_index=True,
                                      return_counts=True)
    keep = (values >= 0) & (counts >= least_size)
    rank = np.empty(int(keep.sum()), dtype=np.int64)
    rank[np.argsort(first[keep], kind='stable')] = np.arange(len(rank))
    table = dict(zip(values[keep].tolist(), rank.tolist()))
    for at, v in enumerate(raw.tolist()):
        out[at] = table.get(v, -1)
    return out


def _linkage(n, w2, a, b):
    """scipy's Z of the edges in Kruskal's order."""
    forest = _Forest(n)
    ident, size = list(range(n)), [1] * n
    Z = np.empty((n - 1, 4))
    for t in range(n - 1):
        ra, rb = forest.find(int(a[t])), forest.find(int(b[t]))
        lo, hi = sorted((ident[ra], ident[rb]))
        forest.up[rb] = ra
        size[ra] += size[rb]
        ident[ra] = n + t
        Z[t] = lo, hi, np.sqrt(w2[t]), size[ra]
    return Z


class KernelHDBSCAN(KernelMatrices):
    """Density clustering of graphs in the feature space of a kernel: the
    clusters, their number, and the noise.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, Y=None)``, ``kernel.diag(X)``; the
        device path asks for ``device_gram`` / ``device_cross_gram`` /
        ``device_diag``), or ``'precomputed'``: then `fit` takes the (n, n)
        kernel matrix and `approximate_predict` a (b, n) cross matrix and the
        (b,) self-similarities `diag` of the new samples, as numpy arrays or
        torch tensors (CPU or CUDA, float32 or float64, in either layout; a
        tensor is worked on where it lies).  The kernel is never modified.
    min_cluster_size: int, ``2 <= min_cluster_size <= n``.
    min_samples: int, ``1 <= min_samples <= n``; None: `min_cluster_size`.
        The sample itself counts, as in scikit-learn.
    cluster_selection_method: 'eom' or 'leaf'.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the matrix lies and the chain runs.

    Not offered: scikit-learn's `alpha`, `cluster_selection_epsilon`,
    `max_cluster_size`, `allow_single_cluster` (the root is never a cluster)
    and `store_centers`.

    After `fit`: `labels_` (-1: noise), `probabilities_`, `n_clusters_`,
    `core_distances_` (n,), `minimum_spanning_tree_` (n - 1, 3): i < j and
    the distance, `single_linkage_tree_` (scipy's Z, for dendrograms),
    `condensed_tree_` (records parent, child, lambda_val, child_size),
    `last_timing`."""

    def __init__(self, kernel, min_cluster_size=5, min_samples=None,
                 cluster_selection_method='eom', kernel_options=None,
                 device='auto'):
        self.kernel = kernel
        self.min_cluster_size = _count('min_cluster_size', min_cluster_size, 2)
        self.min_samples = None if min_samples is None \
            else _count('min_samples', min_samples)
        if cluster_selection_method not in METHODS:
            raise ValueError(f'cluster_selection_method: one of {METHODS} '
                             f'expected, got {cluster_selection_method!r}')
        self.cluster_selection_method = cluster_selection_method
        self.kernel_options = dict(kernel_options or {})
        self.device = device

    # -- the training set ------------------------------------------------------------
    def fit(self, X):
        """Cluster the graphs (or the samples of the precomputed kernel
        matrix) `X`."""
        torch = _torch()
        t = time.perf_counter()
        K, adopted = self._gram(X)
        n = K.shape[0]
        size = self.min_cluster_size
        samples = size if self.min_samples is None else self.min_samples
        if not 2 <= size <= n:
            raise ValueError(f'KernelHDBSCAN: min_cluster_size = {size} with '
                             f'{n} samples; 2 <= min_cluster_size <= n '
                             'expected')
        if not 1 <= samples <= n:
            raise ValueError(f'KernelHDBSCAN: min_samples = {samples} with '
                             f'{n} samples; 1 <= min_samples <= n expected')
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        diag = K.diagonal().to(torch.float64).clone()
        fused = _mst._declines(K) is None
        if samples > 1:
            (d2, _, flag), listed = device_lists(K, diag, diag, samples - 1,
                                                 exclude_self=True)
            c2 = d2[:, samples - 2].contiguous()
            fused = fused and listed
        else:
            c2, flag = torch.zeros_like(diag), None
        w2, a, b, fused = _mst.spanning_tree(K, diag, c2, flag=flag,
                                             fused=fused, name='KernelHDBSCAN')
        core2 = c2.cpu().numpy()
        t_tree = time.perf_counter() - t
        t = time.perf_counter()
        self._n, self._samples = n, samples
        self._dt, self._c2 = diag, c2
        self._w2, self._a, self._b = w2, a, b
        self.core_distances_ = np.sqrt(core2)
        self.minimum_spanning_tree_ = np.column_stack(
            (a.astype(np.float64), b.astype(np.float64), np.sqrt(w2)))
        kids, lam, sizes, _ = _hierarchy(n, w2, a, b)
        tree = _condense(n, kids, lam, sizes, size)
        self.condensed_tree_ = tree
        self._label(tree)
        self._Z = None
        self.X = None if self._precomputed else np.asarray(X)
        self.last_timing = {'kernel': t_kernel, 'tree': t_tree,
                            'host': time.perf_counter() - t,
                            'adopted': adopted, 'fused': fused}
        return self

    def fit_predict(self, X):
        """`labels_` of the graphs `X`."""
        return self.fit(X).labels_

    def _label(self, tree):
        """Steps 7 and 8."""
        n = self._n
        selected, up, birth, top = _select(n, tree,
                                           self.cluster_selection_method)
        # the selected cluster at or above every cluster: parents are born
        # before their children
        above = np.full(len(up), -1, dtype=np.int64)
        for c in range(1, len(up)):
            above[c] = c if selected[c] else above[up[c]]
        point = tree[tree['child'] < n]
        left = np.empty(n, dtype=np.int64)
        leave = np.empty(n)
        left[point['child']] = point['parent'] - n
        leave[point['child']] = point['lambda_val']
        raw = above[left]
        self.labels_ = _number_by_least(raw)
        self.n_clusters_ = int(self.labels_.max()) + 1
        prob = np.zeros(n)
        member = raw >= 0
        prob[member] = _strength(leave[member], top[raw[member]])
        self.probabilities_ = prob
        self._left, self._above, self._up = left, above, up
        self._birth, self._top = birth, top
        # raw cluster -> label
        self._names = np.full(len(up), -1, dtype=np.int64)
        self._names[raw[member]] = self.labels_[member]

    def _fitted(self, what):
        if not hasattr(self, '_w2'):
            raise RuntimeError(f'KernelHDBSCAN: {what} before fit')

    @property
    def single_linkage_tree_(self):
        """scipy's (n - 1, 4) linkage matrix of Kruskal's order (built on
        first access)."""
        self._fitted('single_linkage_tree_')
        if self._Z is None:
            self._Z = _linkage(self._n, self._w2, self._a, self._b)
        return self._Z

    def dbscan_clustering(self, cut_distance, min_cluster_size=None):
        """(n,) labels of DBSCAN* at `cut_distance`: the components of the
        tree's edges shorter than it, those of at least `min_cluster_size`
        members (the model's, if None) numbered by smallest member, -1 for
        the rest."""
        self._fitted('dbscan_clustering')
        size = self.min_cluster_size if min_cluster_size is None \
            else _count('min_cluster_size', min_cluster_size)
        forest = _Forest(self._n)
        for t in np.flatnonzero(np.sqrt(self._w2) < cut_distance).tolist():
            ra = forest.find(int(self._a[t]))
            rb = forest.find(int(self._b[t]))
            forest.up[max(ra, rb)] = min(ra, rb)
        raw = np.array([forest.find(i) for i in range(self._n)],
                       dtype=np.int64)
        return _number_by_least(raw, size)

    # -- new samples -----------------------------------------------------------------
    def _query(self, Z, diag):
        """(cross matrix (b, n), self-similarities (b,)) of new samples."""
        torch = _torch()
        dev = self._dt.device
        if self._precomputed:
            if diag is None:
                raise ValueError("KernelHDBSCAN: kernel='precomputed' needs "
                                 'the self-similarities `diag` of the new '
                                 'samples')
            Ks = self._cross(Z, dev)
            dq = torch.as_tensor(np.array(diag, dtype=np.float64)
                                 if not torch.is_tensor(diag) else diag)
            dq = dq.detach().to(dev, torch.float64)
            if dq.shape != Ks.shape[:1]:
                raise ValueError(f'diag: ({Ks.shape[0]},) expected')
            return Ks, dq
        # (the diagonal first, and kept: the cross matrix is the last thing
        # the kernel's backend is asked for)
        dq = self._self_similarity(Z, dev).clone()
        return self._cross_from(Z, dev)[0], dq

    def approximate_predict(self, Z, diag=None):
        """``(labels (b,), strengths (b,))`` of the graphs `Z`: where each
        would have joined the hierarchy of the training set, which is left as
        it is.  With a precomputed kernel `Z` is the (b, n) cross matrix and
        `diag` the (b,) self-similarities of the new samples."""
        torch = _torch()
        self._fitted('approximate_predict')
        Ks, dq = self._query(Z, diag)
        k = self._samples - 1
        fused = _mst._declines(Ks) is None
        if k:
            (d2, _, flag), listed = device_lists(Ks, dq, self._dt, k)
            cq = d2[:, k - 1].contiguous()
            fused = fused and listed
        else:
            cq, flag = torch.zeros_like(dq), None
        if fused:
            w2, cand, flag = _mst.cross_rows(Ks, dq, self._dt, cq, self._c2,
                                             flag=flag)
        else:
            w2, cand, flag = _mst.cross_rows_torch(Ks, dq, self._dt, cq,
                                                   self._c2, flag=flag)
        down = torch.cat((w2, cand.to(torch.float64),
                          flag.to(torch.float64))).cpu().numpy()
        if down[-1] != 0.0:
            raise ValueError('KernelHDBSCAN: the cross matrix or a '
                             'self-similarity has entries that are not '
                             'finite')
        b = Ks.shape[0]
        lam = _inverse_root(down[:b])
        at = self._left[down[b:2 * b].astype(np.int64)]
        for q in range(b):
            while at[q] > 0 and self._birth[at[q]] > lam[q]:
                at[q] = self._up[at[q]]
        raw = self._above[at]
        labels = np.where(raw >= 0, self._names[np.maximum(raw, 0)], -1)
        strengths = np.zeros(b)
        member = raw >= 0
        strengths[member] = _strength(lam[member], self._top[raw[member]])
        return labels, strengths
