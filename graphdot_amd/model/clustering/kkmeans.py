"""Kernel k-means clustering on top of the kernel protocol.

The reference has no such model; the meaning of every attribute is that of
Lloyd's k-means run in the feature space of the kernel, on the Gram matrix
alone.  With ``lab`` in {0..k-1}^n and n_c the size of
cluster c,

* ``S[i, c] = sum_{j: lab[j] = c} K[i, j]``, ``T[c] = sum_{i: lab[i] = c} S[i,
  c]`` and ``d2(i, c) = K[i, i] - 2 S[i, c] / n_c + T[c] / n_c^2``, the squared
  distance of sample i to the mean of cluster c;
* one round sets ``lab'[i] = argmin_c d2(i, c)`` (the lowest cluster on a
  tie; an empty cluster never attracts a sample); a restart has converged in
  the first round with ``lab' == lab``, whose number is its `n_iter_`;
* ``inertia_ = sum_i K[i, i] - sum_{c: n_c > 0} T[c] / n_c``.

On the GPU, for a kernel with `device_gram`, the matrix is adopted where the
solver wrote it (float or double, its own layout) and all restarts advance in
the same launches of lloyd.hip -- three per round, nothing of size n x n
written or downloaded; `predict` is one launch on the `device_cross_gram`
matrix.  Anywhere else the same chain runs through torch
(`_lloyd.*_torch`)."""
import time
import warnings
import numpy as np
from .._matrices import KernelMatrices
from . import _lloyd


def _torch():
    import torch
    return torch


class KernelKMeans(KernelMatrices):
    """A partition of graphs into k clusters under a kernel.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, Y=None)``; the device path asks for
        ``device_gram`` / ``device_cross_gram`` / ``device_diag``), or
        ``'precomputed'``: then `fit` takes the (n, n) kernel matrix and
        `predict` a (b, n) cross matrix, as numpy arrays or torch tensors (CPU
        or CUDA, float32 or float64; a tensor is worked on where it lies).
    n_clusters: int, ``1 <= k <= min(64, n)``.
    init: 'k-means++' (seed t is drawn with probability proportional to the
        squared distance to the nearest seed so far), 'farthest' (seed t is
        the sample farthest from the seeds so far), or integer seed sample
        indices of shape (k,) or (R, k); the start labels are those of the
        nearest seed.
    n_init: restarts of the two named seedings; the one of lowest inertia is
        reported (the lowest index on a tie).
    max_iter: most rounds; a restart that has not converged by then reports
        the labels its last round used, and `fit` warns.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the dense algebra runs.
    random_state: seed of the ``n_init x k`` uniform numbers of the seeding
        (drawn on the host, once).

    After `fit`: `labels_` (n,), `inertia_`, `cluster_sizes_` (k,),
    `medoid_indices_` (k,; the member nearest to its cluster's mean, -1 for an
    empty cluster), `n_iter_`, `best_restart_`, `restart_inertia_`,
    `restart_n_iter_`, `seed_indices_` (R, k; None with `labels0`),
    `last_timing`."""

    def __init__(self, kernel, n_clusters, init='k-means++', n_init=10,
                 max_iter=300, kernel_options=None, device='auto',
                 random_state=0):
        if int(n_clusters) != n_clusters \
                or not 1 <= n_clusters <= _lloyd.KMAX:
            raise ValueError('n_clusters: an integer from 1 to '
                             f'{_lloyd.KMAX} expected, got {n_clusters}')
        if isinstance(init, str) and init not in _lloyd.INITS:
            raise ValueError(f'init: one of {_lloyd.INITS} or an array of '
                             f'seed indices expected, got {init!r}')
        self.kernel = kernel
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.kernel_options = dict(kernel_options or {})
        self.device = device
        self.random_state = random_state

    def fit(self, X, labels0=None):
        """Cluster the graphs (or the samples of the precomputed kernel
        matrix) `X`.  `labels0`: (n,) or (R, n) start labels in the place of
        the seeding."""
        torch = _torch()
        t = time.perf_counter()
        K, adopted = self._gram(X)
        n, k = K.shape[0], self.n_clusters
        _lloyd._check_k(k, n)
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        # (the matrix as it lies: symmetric, so either contiguous index)
        if K.is_cuda and (n > 1 and K.stride() not in ((n, 1), (1, n))
                          or K.data_ptr() % 16):
            K = K.contiguous()
        r = _lloyd.iterate(K, k, labels0, self.init, self.n_init,
                           self.max_iter, self.random_state)
        if r.status.any():
            raise ValueError('KernelKMeans: the kernel matrix has entries '
                             'that are not finite')
        b = r.best
        # everything below is n x k or smaller; K is not needed any more
        lab, S, T, counts = r.labels[b], r.S[b], r.T[b], r.counts[b]
        diag = K.diagonal().to(torch.float64)
        pick = lab.long()
        d2own = diag - 2.0 * S.gather(1, pick[:, None])[:, 0] / counts[pick] \
            + (T / (counts * counts))[pick]
        D = torch.full((n, k), float('inf'), dtype=torch.float64,
                       device=K.device)
        D.scatter_(1, pick[:, None], d2own[:, None])
        medoid = torch.where(counts > 0, torch.argmin(D, dim=0),
                             torch.full_like(pick[:k], -1))
        self.labels_ = lab.cpu().numpy().astype(np.int64)
        self.cluster_sizes_ = counts.cpu().numpy().astype(np.int64)
        self.medoid_indices_ = medoid.cpu().numpy()
        self.inertia_ = float(r.inertia[b])
        self.n_iter_ = int(r.n_iter[b])
        self.best_restart_ = b
        self.restart_inertia_, self.restart_n_iter_ = r.inertia, r.n_iter
        self.seed_indices_ = None if r.seeds is None \
            else r.seeds.cpu().numpy().astype(np.int64)
        if not r.converged[b]:
            warnings.warn(
                f'KernelKMeans: the best of {len(r.inertia)} restarts had '
                f'not converged after {self.max_iter} rounds; its attributes '
                'describe the labels the last round used', UserWarning)
        if (self.cluster_sizes_ == 0).any():
            warnings.warn(
                f'KernelKMeans: {int((self.cluster_sizes_ == 0).sum())} of '
                f'{k} clusters are empty', UserWarning)
        self._n = n
        self.X = None if self._precomputed else np.asarray(X)
        # what `predict` needs, where the matrix was
        self._state = (lab.contiguous(), T.contiguous(), counts.contiguous())
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'n_iter': self.n_iter_, 'rounds': r.rounds,
                            'looks': r.looks, 'adopted': adopted}
        return self

    def fit_predict(self, X, labels0=None):
        """`labels_` of the graphs `X`."""
        return self.fit(X, labels0).labels_

    def _nearest(self, Z):
        """(D (b, k) = d2 without the samples' own K_zz, argmin (b,))"""
        if not hasattr(self, '_state'):
            raise ValueError('KernelKMeans: predict before fit')
        lab, T, counts = self._state
        Ks = self._cross(Z, lab.device)
        fused = _lloyd.predict if lab.is_cuda else _lloyd.predict_torch
        return fused(Ks, lab, T, counts)

    def predict(self, Z):
        """(b,) the nearest cluster of each of the graphs `Z` (or of the rows
        of a precomputed (b, n) cross matrix)."""
        return self._nearest(Z)[1].cpu().numpy().astype(np.int64)

    def transform(self, Z, diag=None):
        """(b, k) feature-space distances of the graphs `Z` to the cluster
        means (+inf for an empty cluster).  With a precomputed kernel `Z` is
        the (b, n) cross matrix and `diag` the (b,) self-similarities."""
        torch = _torch()
        D = self._nearest(Z)[0]
        if self._precomputed:
            if diag is None:
                raise ValueError("transform: kernel='precomputed' needs the "
                                 'self-similarities `diag` of the new samples')
            d = torch.as_tensor(np.asarray(diag, dtype=np.float64)
                                if not torch.is_tensor(diag) else diag)
            d = d.to(D.device, torch.float64)
            if d.shape != D.shape[:1]:
                raise ValueError(f'diag: ({D.shape[0]},) expected')
        else:
            d = self._self_similarity(Z, D.device)
        return torch.sqrt(torch.clamp_min(d[:, None] + D, 0.0)).cpu().numpy()
