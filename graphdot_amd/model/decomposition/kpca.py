"""Kernel principal component analysis on top of the kernel protocol.

The reference has no such model; the meaning of every attribute is that of
scikit-learn's ``KernelPCA`` with a precomputed kernel.  With ``H = I - 1 1^T
/ n`` and ``Kc = H K H``:

* `eigenvalues_` are the k largest eigenvalues of Kc in descending order,
  `eigenvectors_` (n, k) the orthonormal vectors that belong to them, each
  with its entry of largest magnitude positive (the lowest index on a tie);
* ``fit_transform(X) = eigenvectors_ * sqrt(eigenvalues_)`` and
  ``transform(Z) = Kc_s (eigenvectors_ / sqrt(eigenvalues_))`` with
  ``Kc_s[c, i] = Ks[c, i] - mean_i' Ks[c, i'] - mean_i' K[i', i] + mean K``;
* ``explained_variance_ratio_ = eigenvalues_ / trace(Kc)``, ``trace(Kc) =
  sum_i K_ii - sum_ij K_ij / n``;
* components with an eigenvalue ``<= rcond * eigenvalues_[0]`` are dropped
  with a warning; `n_components_` says how many were kept.

On the GPU, for a kernel with `device_gram`, the matrix is adopted where the
solver wrote it (float or double, its own layout), the k eigenpairs come from
the blocked subspace iteration of subspace.hip -- three launches per
iteration, the centred matrix never written -- and `transform` is one launch on
the `device_cross_gram` matrix.  Anywhere else the same chain runs through
torch (`_subspace.*_torch`)."""
import time
import warnings
import numpy as np
from .._matrices import KernelMatrices
from . import _subspace

SOLVERS = ('auto', 'dense', 'subspace')


def _torch():
    import torch
    return torch


class KernelPCA(KernelMatrices):
    """The k leading principal components of graphs under a kernel.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, Y=None)``; the device path asks for
        ``device_gram`` / ``device_cross_gram``), or ``'precomputed'``: then
        `fit` takes the (n, n) kernel matrix and `transform` a (b, n) cross
        matrix, as numpy arrays or torch tensors (CPU or CUDA, float32 or
        float64; a tensor is worked on where it lies).
    n_components: int, ``1 <= k <= min(16, n - 1)`` (Kc has rank n - 1 at most).
    eigen_solver: 'dense' centres explicitly and calls ``torch.linalg.eigh``;
        'subspace' runs the blocked subspace iteration (`_subspace.iterate`:
        HIP on a CUDA matrix, its torch restatement on a CPU one) and
        finishes with 'dense', with a warning, if that has not met `tol`
        after `max_iter` iterations or its block lost its rank; 'auto' is
        'subspace' for a matrix on a GPU and 'dense' otherwise.
    tol: the first k residual norms ``|Kc v - w v|`` must be ``<= tol |w_0|``.
    max_iter: most iterations of 'subspace'.
    rcond: relative eigenvalue below which a component is dropped.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the dense algebra runs.
    random_state: seed of the start block of 'subspace' (drawn on the host).

    After `fit`: `eigenvalues_`, `eigenvectors_`, `n_components_`,
    `explained_variance_ratio_`, `eigen_solver_` (what ran last), `n_iter_`
    and `residuals_` (of 'subspace'), `last_timing`."""

    def __init__(self, kernel, n_components, eigen_solver='auto', tol=1e-10,
                 max_iter=100, rcond=1e-10, kernel_options=None,
                 device='auto', random_state=0):
        if eigen_solver not in SOLVERS:
            raise ValueError(f'eigen_solver: one of {SOLVERS} expected, got '
                             f'{eigen_solver!r}')
        if int(n_components) != n_components or not \
                1 <= n_components <= _subspace.KMAX:
            raise ValueError('n_components: an integer from 1 to '
                             f'{_subspace.KMAX} expected, got {n_components}')
        self.kernel = kernel
        self.n_components = int(n_components)
        self.eigen_solver = eigen_solver
        self.tol = tol
        self.max_iter = max_iter
        self.rcond = rcond
        self.kernel_options = dict(kernel_options or {})
        self.device = device
        self.random_state = random_state

    # -- the eigenpairs --------------------------------------------------------------
    @staticmethod
    def _eigh_dense(K, colsum, total, k):
        """The k largest eigenpairs of the explicitly centred matrix."""
        torch = _torch()
        n = K.shape[0]
        K = K.to(torch.float64)
        K = 0.5 * (K + K.T)
        cm = colsum / n
        Kc = K - cm[:, None] - cm[None, :] + total / (n * n)
        w, V = torch.linalg.eigh(Kc)
        return (torch.flip(w[n - k:], (0,)).cpu().numpy(),
                torch.flip(V[:, n - k:], (1,)).cpu().numpy())

    def _eigenpairs(self, K, colsum, total, k, v0):
        solver = self.eigen_solver
        if solver == 'auto':
            solver = 'subspace' if K.is_cuda else 'dense'
        self.n_iter_, self.residuals_ = 0, None
        if solver == 'subspace':
            r = _subspace.iterate(K, k, self.tol, self.max_iter,
                                  self.random_state, v0)
            self.n_iter_, self.residuals_ = r.n_iter, r.residuals[:k]
            if r.converged:
                self.eigen_solver_ = 'subspace'
                return r.w[:k].copy(), r.V[:, :k].cpu().numpy()
            _subspace.warn_not_converged(r, k, self.tol, self.max_iter)
        self.eigen_solver_ = 'dense'
        return self._eigh_dense(K, colsum, total, k)

    def fit(self, X, v0=None):
        """Find the components of the graphs (or of the precomputed kernel
        matrix) `X`.  `v0`: an (n, m) start block for 'subspace' in the
        place of the random one."""
        torch = _torch()
        t = time.perf_counter()
        K, adopted = self._gram(X)
        n, k = K.shape[0], self.n_components
        if not 1 <= k <= min(_subspace.KMAX, n - 1):
            raise ValueError(
                f'n_components = {k}: the centred matrix of {n} samples has '
                f'rank {max(n - 1, 0)} at most; 1 <= n_components <= '
                f'min({_subspace.KMAX}, n - 1) expected')
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        if K.is_cuda:
            # (the matrix as it lies: symmetric, so either contiguous index)
            if n > 1 and K.stride() not in ((n, 1), (1, n)) \
                    or K.data_ptr() % 16:
                K = K.contiguous()
            colsum, tot = _subspace.sums(K)
        else:
            colsum, tot = _subspace.sums_torch(K)
        w, V = self._eigenpairs(K, colsum, tot[0], k, v0)
        # everything below is n x k or smaller; K is not needed any more
        tot = tot.cpu().numpy()
        trace = float(tot[1] - tot[0] / n)
        lead = np.argmax(np.abs(V), axis=0)          # (the first on a tie)
        V = V * np.where(V[lead, np.arange(V.shape[1])] < 0, -1.0, 1.0)
        keep = w > self.rcond * w[0] if w[0] > 0 else np.zeros(k, dtype=bool)
        if not keep.all():
            warnings.warn(
                f'KernelPCA: {k - int(keep.sum())} of {k} components have an '
                f'eigenvalue <= rcond * {w[0]:.3g} and are dropped',
                UserWarning)
            w, V = w[keep], V[:, keep]
        self.eigenvalues_ = w
        self.eigenvectors_ = V
        self.n_components_ = len(w)
        self.explained_variance_ratio_ = w / trace
        self._n = n
        self.X = None if self._precomputed else np.asarray(X)
        # what `transform` needs, where the matrix was
        A = np.ascontiguousarray(V / np.sqrt(w))
        self._state = (torch.from_numpy(A).to(K.device),
                       (colsum / n).contiguous(), float(tot[0]) / (n * n))
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'n_iter': self.n_iter_, 'adopted': adopted,
                            'solver': self.eigen_solver_}
        return self

    def fit_transform(self, X, v0=None):
        """(n, n_components_) coordinates of the training samples."""
        self.fit(X, v0)
        return self.eigenvectors_ * np.sqrt(self.eigenvalues_)

    def transform(self, Z):
        """(b, n_components_) coordinates of the graphs `Z` (or of the rows
        of a precomputed (b, n) cross matrix)."""
        if not hasattr(self, '_state'):
            raise RuntimeError('Model not trained.')
        A, colmean, gmean = self._state
        Ks = self._cross(Z, A.device)
        if A.shape[1] == 0:
            return np.zeros((Ks.shape[0], 0))
        fused = _subspace.project if A.is_cuda else _subspace.project_torch
        return fused(Ks, A, colmean, gmean).cpu().numpy()
