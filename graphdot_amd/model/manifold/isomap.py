"""Isomap maps of graphs on top of the kernel protocol.

The reference has no such model; the meaning of every attribute is that of
scikit-learn's ``Isomap(metric='precomputed', eigen_solver='dense')`` on the
matrix of feature-space distances ``sqrt(D2)``:

1. ``D2[i, j] = max((K[i, i] + K[j, j]) - 2 K[i, j], 0)``;
2. the neighbours N(i) of a sample are the `n_neighbors` first ``j != i`` in
   the total order ``(D2[i, j], j)``: the lists of the neighbour models;
3. the graph has the undirected edge {i, j} where j is in N(i) or i in N(j),
   of length ``W[i, j] = sqrt(min(D2[i, j], D2[j, i]))``; ``W[i, i] = 0``
   and ``W = inf`` elsewhere (the min makes W symmetric to the bit even where
   the stored K is not);
4. `dist_matrix_` G holds the lengths of the shortest paths in W;
5. a graph that is not connected is an error: `fit` raises ValueError with
   the number of components and their sizes.  *This departs from
   scikit-learn on purpose*, which joins the components by their closest
   pairs with a warning: an edge made up for the occasion decides where whole
   components lie on the map, and a larger `n_neighbors` is the honest fix;
6. with ``B = -0.5 G * G`` and ``H = I - 1 1^T / n``, `eigenvalues_` and the
   embedding are the `n_components` algebraically largest eigenpairs of ``H B
   H``, scaled and signed as `KernelPCA.fit_transform` does it; components
   at or below ``rcond * eigenvalues_[0]`` are dropped with its warning;
7. a new sample with the list ``(d2_r, j_r)`` against the training set
   (nothing left out) is at ``Gq[j] = min_r (sqrt(d2_r) + G[j_r, j])`` from
   training sample j; `transform` is `KernelPCA.transform` of ``Bq = -0.5 Gq
   * Gq`` and `geodesic_distances` returns Gq;
8. ``reconstruction_error() = sqrt(|H B H|_F^2 - sum eigenvalues_^2) / n``.

``H B H`` is indefinite -- geodesics are not Euclidean distances -- so its
eigenvalues of largest magnitude need not be its largest: the eigenpairs come
from the dense solver of `KernelPCA`, never from its subspace iteration.

On the GPU, for a kernel with `device_gram`, the matrix is adopted where the
solver wrote it (float or double, its own layout); the lists come from the
kernels of csrc/device/knn.h, and the graph, the shortest paths (a blocked
Floyd-Warshall algorithm), B and the out-of-sample geodesics from those of
geodesic.h: two (n, n) double buffers are written, G and B, and one word is
downloaded before the eigenpairs, the number of components.  Anywhere else,
and for more than 64 neighbours, the same chain runs through torch
(`_geodesic.*_torch`)."""
import time
import numpy as np
from .._matrices import KernelMatrices
from ..decomposition import KernelPCA
from ..neighbors import device_lists
from . import _geodesic

#: most components: `KernelPCA`'s
N_COMPONENTS_MOST = 16


def _torch():
    import torch
    return torch


def _count(name, k):
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f'{name}: a positive integer expected, got {k}')
    return int(k)


class KernelIsomap(KernelMatrices):
    """A low-dimensional map of graphs that keeps their geodesic distances
    on the neighbourhood graph of a kernel's feature space.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, Y=None)``, ``kernel.diag(X)``; the
        device path asks for ``device_gram`` / ``device_cross_gram`` /
        ``device_diag``), or ``'precomputed'``: then `fit` takes the (n, n)
        kernel matrix and `transform` a (b, n) cross matrix and the (b,)
        self-similarities `diag` of the new samples, as numpy arrays or torch
        tensors (CPU or CUDA, float32 or float64, in either layout; a tensor
        is worked on where it lies).  The kernel is never modified.
    n_neighbors: int, ``1 <= n_neighbors <= n - 1``.
    n_components: int, ``1 <= n_components <= min(16, n - 1)``.
    rcond: relative eigenvalue below which a component is dropped.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the matrix lies and the chain runs.

    A neighbourhood graph that is not connected raises ValueError in `fit`
    (scikit-learn joins the components with a warning; see the module's
    text).

    After `fit`: `embedding_` (n, n_components_), `eigenvalues_`,
    `n_components_`, `dist_matrix_` (downloaded on first access),
    `last_timing`."""

    def __init__(self, kernel, n_neighbors=5, n_components=2, rcond=1e-10,
                 kernel_options=None, device='auto'):
        self.kernel = kernel
        self.n_neighbors = _count('n_neighbors', n_neighbors)
        self.n_components = _count('n_components', n_components)
        if self.n_components > N_COMPONENTS_MOST:
            raise ValueError('n_components: an integer from 1 to '
                             f'{N_COMPONENTS_MOST} expected, got '
                             f'{n_components}')
        self.rcond = rcond
        self.kernel_options = dict(kernel_options or {})
        self.device = device

    # -- the training set ------------------------------------------------------------
    def fit(self, X):
        """Map the graphs (or the samples of the precomputed kernel matrix)
        `X`."""
        torch = _torch()
        t = time.perf_counter()
        K, adopted = self._gram(X)
        n, k, c = K.shape[0], self.n_neighbors, self.n_components
        if not 1 <= k <= n - 1:
            raise ValueError(f'KernelIsomap: n_neighbors = {k} with {n} '
                             'samples; 1 <= n_neighbors <= n - 1 expected')
        if not 1 <= c <= min(N_COMPONENTS_MOST, n - 1):
            raise ValueError(
                f'KernelIsomap: n_components = {c} with {n} samples; 1 <= '
                f'n_components <= min({N_COMPONENTS_MOST}, n - 1) expected')
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        dev = K.device
        diag = K.diagonal().to(torch.float64).clone()
        (_, idx, flag), fused = device_lists(K, diag, diag, k,
                                             exclude_self=True)
        fused = fused and _geodesic._declines(K, k) is None
        if fused:
            G = _geodesic.shortest_paths(_geodesic.graph(K, diag, idx))
            B, label, count = _geodesic.finish(G)
        else:
            G = _geodesic.shortest_paths_torch(
                _geodesic.graph_torch(K, diag, idx))
            B, label, count = _geodesic.finish_torch(G)
        # one download before the eigenpairs: the components and the flag word
        n_graphs, bad = torch.stack((count.sum(), flag.sum())).cpu().tolist()
        if bad:
            raise ValueError('KernelIsomap: the kernel matrix has entries '
                             'that are not finite')
        if n_graphs != 1:
            sizes = _geodesic.component_sizes(label.cpu().numpy())
            raise ValueError(
                f'KernelIsomap: the neighbourhood graph of n_neighbors = {k} '
                f'is not connected: {n_graphs} components of sizes {sizes}; '
                'use a larger n_neighbors')
        if K.is_cuda:
            torch.cuda.synchronize(dev)
        t_paths = time.perf_counter() - t
        t = time.perf_counter()
        pca = KernelPCA('precomputed', c, eigen_solver='dense',
                        rcond=self.rcond, device=self.device)
        self.embedding_ = pca.fit_transform(B)
        # |H B H|_F^2 = |B|_F^2 - 2 |B 1|^2 / n + (1^T B 1)^2 / n^2, from
        # reductions of B: the centred matrix is not written for it
        colsum = B.sum(0)
        total = colsum.sum()
        norm2 = torch.linalg.vector_norm(B) ** 2 \
            - 2.0 * (colsum @ colsum) / n + total * total / (n * n)
        self._centred_norm2 = float(norm2)
        self._pca = pca
        self.eigenvalues_ = pca.eigenvalues_
        self.n_components_ = pca.n_components_
        self._G, self._dist = G, None
        self._dt = diag
        self._n = n
        self._fused = fused
        self.X = None if self._precomputed else np.asarray(X)
        self.last_timing = {'kernel': t_kernel, 'paths': t_paths,
                            'linalg': time.perf_counter() - t,
                            'adopted': adopted, 'fused': fused}
        return self

    def fit_transform(self, X):
        """`embedding_` of the graphs `X`."""
        return self.fit(X).embedding_

    def _fitted(self, what):
        if not hasattr(self, '_G'):
            raise RuntimeError(f'KernelIsomap: {what} before fit')

    @property
    def dist_matrix_(self):
        """(n, n) geodesic distances of the training samples, as a numpy
        array: downloaded on first access."""
        self._fitted('dist_matrix_')
        if self._dist is None:
            self._dist = self._G.cpu().numpy()
        return self._dist

    def reconstruction_error(self):
        """``sqrt(|H B H|_F^2 - sum eigenvalues_^2) / n``: scikit-learn's."""
        self._fitted('reconstruction_error')
        rest = self._centred_norm2 - float(np.sum(self.eigenvalues_ ** 2))
        return float(np.sqrt(max(rest, 0.0))) / self._n

    # -- new samples -----------------------------------------------------------------
    def _query(self, Z, diag):
        """(cross matrix (b, n), self-similarities (b,), adopted?) of new
        samples."""
        torch = _torch()
        dev = self._G.device
        if self._precomputed:
            if diag is None:
                raise ValueError("KernelIsomap: kernel='precomputed' needs "
                                 'the self-similarities `diag` of the new '
                                 'samples')
            Ks = self._cross(Z, dev)
            dq = torch.as_tensor(np.array(diag, dtype=np.float64)
                                 if not torch.is_tensor(diag) else diag)
            dq = dq.detach().to(dev, torch.float64)
            if dq.shape != Ks.shape[:1]:
                raise ValueError(f'diag: ({Ks.shape[0]},) expected')
            return Ks, dq, False
        # (the diagonal first, and kept: the cross matrix is the last thing
        # the kernel's backend is asked for)
        dq = self._self_similarity(Z, dev).clone()
        Ks, adopted = self._cross_from(Z, dev)
        return Ks, dq, adopted

    def _extend(self, Z, diag, distances):
        """(Bq, Gq) of new samples on the device of G."""
        self._fitted('a query')
        Ks, dq, _ = self._query(Z, diag)
        k = self.n_neighbors
        (d2, idx, flag), fused = device_lists(Ks, dq, self._dt, k)
        if fused and self._G.is_cuda and k <= _geodesic.K_MOST:
            Bq, Gq = _geodesic.extend(d2, idx, self._G, distances)
        else:
            Bq, Gq = _geodesic.extend_torch(d2, idx, self._G, distances)
        if int(flag):
            raise ValueError('KernelIsomap: the cross matrix or a '
                             'self-similarity has entries that are not '
                             'finite')
        return Bq, Gq

    def transform(self, Z, diag=None):
        """(b, n_components_) coordinates of the graphs `Z`.  With a
        precomputed kernel `Z` is the (b, n) cross matrix and `diag` the (b,)
        self-similarities of the new samples."""
        Bq, _ = self._extend(Z, diag, False)
        return self._pca.transform(Bq)

    def geodesic_distances(self, Z, diag=None):
        """(b, n) geodesic distances of the graphs `Z` to the training
        samples: to the nearest training samples directly, on through the
        graph."""
        return self._extend(Z, diag, True)[1].cpu().numpy()
