"""Nearest-neighbour search in the feature space of a kernel.

The squared distance of two samples is ``d2(x, y) = max(0, (k(x, x) + k(y,
y)) - 2 k(x, y))`` and ``d = sqrt(d2)``: the reference's
`KernelInducedDistance` -- ``sqrt(max(0, k(x, x) / 2 + k(y, y) / 2 - k(x,
y)))``, with an exact one half -- times sqrt 2.  The neighbours of a sample
are the k candidates that come first in the total order (d2, index): ties go
to the smaller index, which makes the lists independent of how the matrix
lies and of how the search is split.  Every method
means what its scikit-learn counterpart means with ``metric='precomputed'``
on the matrix of d.

On the GPU, for a kernel with `device_gram` / `device_cross_gram`, the matrix
is adopted where the solver wrote it (float or double, its own layout) and
the lists are selected there by the kernels of csrc/device/knn.h; one
download per call: the lists and a flag word.  Anywhere else, and for more
than `_knn.K_MOST` neighbours, the same chain runs through torch
(`_knn.topk_torch`)."""
import time
import numpy as np
from .._matrices import KernelMatrices
from . import _knn


def _torch():
    import torch
    return torch


def _count(name, k):
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f'{name}: a positive integer expected, got {k}')
    return int(k)


def device_lists(Ks, dq, dt, k, exclude_self=False):
    """(``(d2 (b, k) float64, idx (b, k) int64, flag (1,) int32)``, fused?)
    on the device of the (b, n) matrix `Ks`, nothing downloaded: per row the k
    nearest columns in the order (d2, column), nearest first, with the
    self-similarities `dq` (b,) and `dt` (n,) float64; `flag` is not zero if
    some d2 is not finite.  exclude_self: column i is no candidate of row i.
    The search of the neighbour models, for the models of other packages that
    build on the lists: the kernels of csrc/device/knn.h where they apply,
    torch anywhere else."""
    return _knn.search(Ks, dq, dt, k, exclude_self=exclude_self)


class KernelNeighborsBase(KernelMatrices):
    """What the neighbour models share: the training matrix and its diagonal,
    the two searches and the one download of a call."""

    def _init(self, kernel, n_neighbors, kernel_options, device):
        self.kernel = kernel
        self.n_neighbors = _count('n_neighbors', n_neighbors)
        self.kernel_options = dict(kernel_options or {})
        self.device = device

    @property
    def _name(self):
        return type(self).__name__

    # -- the training set ------------------------------------------------------------
    def _fit_matrix(self, X):
        """(K, adopted?, seconds of the kernel): the training matrix; keeps
        its diagonal, its size and what `_cross` needs.  An adopted matrix is
        the solver's own buffer: it is used before `fit` returns and not
        kept (`_training_matrix` asks again)."""
        torch = _torch()
        t = time.perf_counter()
        K, adopted = self._gram(X)
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        if K.shape[0] < 1:
            raise ValueError(f'{self._name}: an empty training set')
        self._n = K.shape[0]
        self.X = None if self._precomputed else np.asarray(X)
        self._K = K if self._precomputed else None
        self._dt = K.diagonal().to(torch.float64).clone()
        return K, adopted, t_kernel

    def _fitted(self, what):
        if not hasattr(self, '_dt'):
            raise ValueError(f'{self._name}: {what} before fit')

    def _training_matrix(self):
        """(K, adopted?) of the training set again."""
        if self._K is not None:
            return self._K, False
        return self._gram(self.X)

    # -- the searches ----------------------------------------------------------------
    def _k(self, n_neighbors, candidates):
        k = self.n_neighbors if n_neighbors is None \
            else _count('n_neighbors', n_neighbors)
        if k > candidates:
            raise ValueError(f'{self._name}: n_neighbors = {k} exceeds the '
                             f'{candidates} candidates')
        return k

    def _own_lists(self, K, k):
        """(``(d2, idx, flag)``, fused?) of the training samples, each left
        out of its own list."""
        return _knn.search(K, self._dt, self._dt, self._k(k, self._n - 1),
                           exclude_self=True)

    def _query(self, Z, diag):
        """(cross matrix (b, n), self-similarities (b,), adopted?) of new
        samples."""
        torch = _torch()
        dev = self._dt.device
        if self._precomputed:
            if diag is None:
                raise ValueError(f"{self._name}: kernel='precomputed' needs "
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

    def _lists(self, Z, diag, n_neighbors=None):
        """(``(d2, idx, flag)``, timing) of the samples `Z` -- of the
        training samples, each left out, for ``Z=None``."""
        torch = _torch()
        self._fitted('a query')
        t = time.perf_counter()
        if Z is None:
            K, adopted = self._training_matrix()
            k = self._k(n_neighbors, self._n - 1)
        else:
            K, dq, adopted = self._query(Z, diag)
            k = self._k(n_neighbors, self._n)
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        timing = {'kernel': time.perf_counter() - t, 'adopted': adopted}
        timing['start'] = time.perf_counter()
        if Z is None:
            lists, timing['fused'] = self._own_lists(K, k)
        else:
            lists, timing['fused'] = _knn.search(K, dq, self._dt, k)
        return lists, timing

    def _download(self, flag, *tensors, timing=None):
        """The tensors as numpy arrays, from one download with the flag word;
        ValueError if the flag is up."""
        torch = _torch()
        flat = [t.reshape(-1).to(torch.float64) for t in tensors]
        down = torch.cat(flat + [flag.to(torch.float64)]).cpu().numpy()
        if down[-1] != 0.0:
            raise ValueError(f'{self._name}: the kernel matrix or a '
                             'self-similarity has entries that are not '
                             'finite')
        out, at = [], 0
        for t in tensors:
            out.append(down[at:at + t.numel()].reshape(tuple(t.shape)))
            at += t.numel()
        if timing is not None:
            timing['linalg'] = time.perf_counter() - timing.pop('start')
            self.last_timing = timing
        return out


class KernelNearestNeighbors(KernelNeighborsBase):
    """The k nearest training graphs of a graph under a kernel.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, Y=None)``, ``kernel.diag(X)``; the
        device path asks for ``device_gram`` / ``device_cross_gram`` /
        ``device_diag``), or ``'precomputed'``: then `fit` takes the (n, n)
        kernel matrix and `kneighbors` a (b, n) cross matrix and the (b,)
        self-similarities `diag` of the new samples, as numpy arrays or torch
        tensors (CPU or CUDA, float32 or float64; a tensor is worked on where
        it lies).  The kernel is never modified.
    n_neighbors: int, the default k of `kneighbors`.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the matrix lies and the search runs.

    After `fit`: `n_samples_fit_`, `last_timing`."""

    def __init__(self, kernel, n_neighbors=5, kernel_options=None,
                 device='auto'):
        self._init(kernel, n_neighbors, kernel_options, device)

    def fit(self, X):
        """Take the graphs (or the samples of the precomputed kernel matrix)
        `X` as the candidates."""
        K, adopted, t_kernel = self._fit_matrix(X)
        self.n_samples_fit_ = self._n
        self.last_timing = {
            'kernel': t_kernel, 'linalg': 0.0, 'adopted': adopted,
            'fused': _knn._declines(K, self.n_neighbors) is None}
        return self

    def kneighbors(self, Z=None, n_neighbors=None, return_distance=True,
                   diag=None):
        """``(dist (b, k) float64, idx (b, k) int64)`` -- or the indices
        alone -- of the k nearest candidates of the graphs `Z`, nearest
        first.  ``Z=None``: of the training samples, each left out of its own
        list.  With a precomputed kernel `Z` is the (b, n) cross matrix and
        `diag` the (b,) self-similarities.  ValueError if k exceeds the
        number of candidates: n, or n - 1 with ``Z=None``."""
        (d2, idx, flag), timing = self._lists(Z, diag, n_neighbors)
        d2, idx = self._download(flag, d2, idx, timing=timing)
        idx = idx.astype(np.int64)
        return (np.sqrt(d2), idx) if return_distance else idx
