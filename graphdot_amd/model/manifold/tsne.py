"""t-SNE maps of graphs on top of the kernel protocol.

The reference has no such model; the meaning of every attribute is that of
scikit-learn's ``TSNE(method='exact', metric='precomputed')`` on the matrix of
feature-space distances ``sqrt(d2)``, ``d2[i, j] = max(0, (K[i, i] + K[j, j])
- 2 K[i, j])``.  With ``eps = np.finfo(float).eps``:

* per row, ``beta_i`` from scikit-learn's bisection (from 1, at most 100
  steps, to within 1e-5) for the entropy ``log(perplexity)`` of ``e_ij =
  exp(-beta_i (d2[i, j] - m_i))``, ``m_i = min_{j != i} d2[i, j]``, ``Z_i =
  sum_{j != i} e_ij`` -- in double and with the shift, where scikit-learn
  searches in float32 without it;
* ``p_ij = max((e_ij / Z_i + e_ji / Z_j) / (2 n), eps)``, ``w_ij = 1 / (1 +
  |y_i - y_j|^2)``, ``q_ij = max(w_ij / sum_{k != l} w_kl, eps)``, and with the
  exaggeration a the objective ``KL = sum_{i != j} a p_ij log(max(a p_ij,
  eps) / q_ij)`` with the gradient ``4 sum_j (a p_ij - q_ij) w_ij (y_i -
  y_j)``;
* scikit-learn's descent: gains (+0.2 where update and gradient differ in
  sign, x 0.8 elsewhere, 0.01 at the least), ``update = momentum update -
  learning_rate gains grad``; ``min(250, max_iter)`` steps at ``a =
  early_exaggeration`` with momentum 0.5, the rest at 1 with 0.8, update and
  gains starting anew; a look at the KL and at the norm of the gains-scaled
  gradient every 50th step, which ends the descent if the KL has not improved
  for more than 250 (then `n_iter_without_progress`) steps or the norm is
  ``<= min_grad_norm``.

On the GPU, for a kernel with `device_gram`, the matrix is adopted where the
solver wrote it (float or double, its own layout) and every step is two
launches of tsne.h: P is recomputed per pair from three numbers per row,
nothing of size n x n is written, and three numbers are downloaded per look.
Anywhere else, and for ``n_components`` other than 2 and 3, the same chain
runs through torch (`_tsne.*_torch`) with P stored."""
import time
import warnings
import numpy as np
from .._matrices import KernelMatrices
from . import _tsne

INITS = ('kpca', 'random')
#: the standard deviation of the first column of a named start
INIT_SCALE = 1e-4


def _torch():
    import torch
    return torch


class KernelTSNE(KernelMatrices):
    """A low-dimensional map of graphs that keeps their neighbourhoods under
    a kernel.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, Y=None)``; the device path asks for
        ``device_gram``), or ``'precomputed'``: then `fit` takes the (n, n)
        kernel matrix, as a numpy array or a torch tensor (CPU or CUDA,
        float32 or float64; a tensor is worked on where it lies).  The
        kernel is never modified.
    n_components: int >= 1; the fused chain has 2 and 3.
    perplexity: the effective number of neighbours, ``0 < perplexity < n``.
    early_exaggeration: the factor on P in the first phase.
    learning_rate: a number, or 'auto': ``max(n / early_exaggeration / 4,
        50)``.
    max_iter: steps of the descent, both phases together.
    n_iter_without_progress, min_grad_norm: what ends the descent early.
    init: 'kpca' (the first coordinates of `KernelPCA` on the same matrix,
        scaled to a standard deviation of 1e-4 in the first), 'random' (1e-4
        times standard normal numbers of `random_state`), or an (n,
        n_components) array.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the matrix lies and the descent
        runs.
    random_state: seed of the 'random' start (drawn on the host) and of
        `KernelPCA`'s.

    After `fit`: `embedding_` (n, n_components), `kl_divergence_`, `n_iter_`
    (steps taken), `beta_` (n,), `n_uncalibrated_` (rows whose bisection used
    all its steps), `learning_rate_`, `last_timing`."""

    def __init__(self, kernel, n_components=2, perplexity=30.0,
                 early_exaggeration=12.0, learning_rate='auto', max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7,
                 init='kpca', kernel_options=None, device='auto',
                 random_state=0):
        if isinstance(n_components, bool) or int(n_components) != n_components \
                or n_components < 1:
            raise ValueError('n_components: a positive integer expected, got '
                             f'{n_components}')
        if not perplexity > 0:
            raise ValueError(f'perplexity: a positive number expected, got '
                             f'{perplexity}')
        if isinstance(init, str) and init not in INITS:
            raise ValueError(f'init: one of {INITS} or an (n, n_components) '
                             f'array expected, got {init!r}')
        if isinstance(learning_rate, str) and learning_rate != 'auto':
            raise ValueError("learning_rate: a number or 'auto' expected, got "
                             f'{learning_rate!r}')
        if int(max_iter) != max_iter or max_iter < 0:
            raise ValueError('max_iter: a non-negative integer expected, got '
                             f'{max_iter}')
        self.kernel = kernel
        self.n_components = int(n_components)
        self.perplexity = float(perplexity)
        self.early_exaggeration = float(early_exaggeration)
        self.learning_rate = learning_rate
        self.max_iter = int(max_iter)
        self.n_iter_without_progress = n_iter_without_progress
        self.min_grad_norm = min_grad_norm
        self.init = init
        self.kernel_options = dict(kernel_options or {})
        self.device = device
        self.random_state = random_state

    def _start(self, K, n):
        """The (n, d) start on the host."""
        d = self.n_components
        if isinstance(self.init, str) and self.init == 'random':
            rng = np.random.RandomState(self.random_state)
            return INIT_SCALE * rng.standard_normal((n, d))
        if isinstance(self.init, str):
            from ..decomposition import KernelPCA
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', UserWarning)
                Y = KernelPCA('precomputed', d, device=self.device,
                              random_state=self.random_state).fit_transform(K)
            if Y.shape[1] < d or not Y[:, 0].std() > 0:
                raise ValueError(
                    f"KernelTSNE: init='kpca' found {Y.shape[1]} of {d} "
                    "components in this matrix; use init='random'")
            return Y * (INIT_SCALE / Y[:, 0].std())
        Y = np.array(self.init.detach().cpu() if _torch().is_tensor(self.init)
                     else self.init, dtype=np.float64)
        if Y.shape != (n, d):
            raise ValueError(f'init: an array of shape {(n, d)} expected, '
                             f'got {Y.shape}')
        if not np.isfinite(Y).all():
            raise ValueError('init: entries that are not finite')
        return Y

    def fit(self, X):
        """Map the graphs (or the samples of the precomputed kernel matrix)
        `X`."""
        torch = _torch()
        t = time.perf_counter()
        K, adopted = self._gram(X)
        n, d = K.shape[0], self.n_components
        if not self.perplexity < n:
            raise ValueError(f'KernelTSNE: perplexity = {self.perplexity} '
                             f'must be less than the {n} samples')
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        # (the matrix as it lies: symmetric, so either contiguous index)
        if K.is_cuda and K.stride() not in ((n, 1), (1, n)):
            K = K.contiguous()
        fused = _tsne._declines(K, d) is None
        diag = K.diagonal().to(torch.float64).contiguous()
        calibrate = _tsne.calibrate if fused else _tsne.calibrate_torch
        beta, m, rZ, steps, flag = calibrate(K, diag, self.perplexity)
        if isinstance(self.init, str) and self.init == 'kpca' and int(flag):
            # (KernelPCA downloads its eigenvectors: the flag word is read
            # here, before it, and not with the first look)
            raise ValueError('KernelTSNE: the kernel matrix has entries that '
                             'are not finite')
        Y0 = self._start(K, n)
        Y0 = torch.from_numpy(np.ascontiguousarray(Y0))
        lr = self.learning_rate
        if isinstance(lr, str):
            lr = max(n / self.early_exaggeration / 4.0, 50.0)
        try:
            r = _tsne.descend(K, diag, beta, m, rZ, flag, Y0.to(K.device),
                              self.max_iter, self.early_exaggeration,
                              float(lr), self.n_iter_without_progress,
                              self.min_grad_norm, fused=fused)
        except ValueError as e:
            raise ValueError(f'KernelTSNE: {e}') from None
        # one download: everything below is n x d or smaller
        down = torch.cat((r.Y.reshape(-1), beta,
                          steps.to(torch.float64))).cpu().numpy()
        self.embedding_ = down[:n * d].reshape(n, d).copy()
        self.beta_ = down[n * d:n * d + n].copy()
        self.n_uncalibrated_ = int((down[n * d + n:] >= _tsne.N_STEPS).sum())
        if self.n_uncalibrated_:
            warnings.warn(
                f'KernelTSNE: the bisection of {self.n_uncalibrated_} of {n} '
                f'rows used all its {_tsne.N_STEPS} steps without reaching '
                f'the perplexity {self.perplexity}', UserWarning)
        self.kl_divergence_ = r.kl
        self.n_iter_ = r.n_iter
        self.learning_rate_ = float(lr)
        self._n = n
        self.X = None if self._precomputed else np.asarray(X)
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'n_iter': r.n_iter, 'looks': r.looks,
                            'stopped': r.stopped, 'adopted': adopted,
                            'fused': r.fused}
        return self

    def fit_transform(self, X):
        """`embedding_` of the graphs `X`."""
        return self.fit(X).embedding_
