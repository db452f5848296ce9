"""The kernel two-sample test on top of the kernel protocol: do two sets of
graphs come from the same distribution?

The reference has no such model; the quantity is the maximum mean discrepancy
of Gretton, Borgwardt, Rasch, Schoelkopf and Smola, "A kernel two-sample
test" (JMLR 13, 2012).  With the Gram matrix K of the
pooled sample of N = n + m graphs and the 0/1 vector z of the members of the
first sample, ``S_xx = z^T K z``, ``S_xy = z^T K (1 - z)`` and ``S_yy = (1 -
z)^T K (1 - z)`` give the squared discrepancy

    biased:    S_xx / n^2 + S_yy / m^2 - 2 S_xy / (n m)
    unbiased:  the same with the diagonal left out of S_xx and S_yy, over
               n (n - 1) and m (m - 1)

and the same sums for `n_permutations` random splits of the pool into n and m
graphs give its null distribution: ``pvalue_ = (1 + #{null_ >= statistic_})
/ (1 + n_permutations)``.  The witness ``w_i = sum_j K_ij s_j``, ``s = z / n -
(1 - z) / m``, is positive where the first sample is the denser one.

On the GPU, for a kernel with `device_gram`, the pooled matrix is adopted where
the solver wrote it (float or double, its own layout) and all the sums are
three launches of mmd.hip with one download of ``3 (n_permutations + 1) + 2``
doubles and the N witness values; nothing of size N x N is written.  Anywhere
else the same chain runs through torch (`_mmd.forms_torch`)."""
import time
import numpy as np
from .._matrices import KernelMatrices
from . import _mmd


def _torch():
    import torch
    return torch


class KernelTwoSampleTest(KernelMatrices):
    """The MMD permutation test of two samples of graphs.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X)``, ``kernel(X, Y)``; the device path
        asks for ``device_gram``), or ``'precomputed'``: then `fit` and
        `statistic` take the (N, N) symmetric kernel matrix of the pooled
        sample as a numpy array or a torch tensor (CPU or CUDA, float32 or
        float64; a tensor is worked on where it lies), and for `Y` the size n
        of the first sample (its first n rows) or a boolean membership vector
        of length N.  The kernel is never modified.
    n_permutations: int
        Random splits for the null distribution; 0: the statistic alone.
    estimator: 'unbiased' (needs two points per sample) or 'biased'.
    random_state: seed of the permutations (None: drawn once per `fit` from
        numpy's global generator, and kept as `seed_`).
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the matrix lies and the sums run.

    After `fit`: `statistic_`, `pvalue_` (None without permutations), `null_`
    (n_permutations,), `witness_` (N,), `n_`, `m_`, `seed_`, `last_timing`."""

    def __init__(self, kernel, n_permutations=999, estimator='unbiased',
                 random_state=None, kernel_options=None, device='auto'):
        if estimator not in _mmd.ESTIMATORS:
            raise ValueError(f'estimator: one of {_mmd.ESTIMATORS} expected, '
                             f'got {estimator!r}')
        if isinstance(n_permutations, bool) \
                or int(n_permutations) != n_permutations \
                or n_permutations < 0:
            raise ValueError('n_permutations: a non-negative integer '
                             f'expected, got {n_permutations}')
        self.kernel = kernel
        self.n_permutations = int(n_permutations)
        self.estimator = estimator
        self.random_state = random_state
        self.kernel_options = dict(kernel_options or {})
        self.device = device

    # -- the pooled sample -----------------------------------------------------------
    def _pool(self, X, Y):
        """(what `_gram` takes, the observed split z0 or None until the size
        of a precomputed matrix is known)"""
        if not self._precomputed:
            X, Y = np.asarray(X), np.asarray(Y)
            if len(X) == 0 or len(Y) == 0:
                raise ValueError('KernelTwoSampleTest: an empty sample')
            return np.concatenate((X, Y)), np.arange(len(X) + len(Y)) < len(X)
        return X, None

    @staticmethod
    def _membership(Y, N):
        """The observed split of a precomputed (N, N) matrix."""
        if _torch().is_tensor(Y):
            Y = Y.detach().cpu().numpy()
        Y = np.asarray(Y)
        if Y.ndim == 0:
            if Y.dtype.kind not in 'iu' or not 0 <= int(Y) <= N:
                raise ValueError('Y: the size of the first sample, an integer '
                                 f'from 0 to {N}, or a boolean membership '
                                 f'vector expected, got {Y}')
            return np.arange(N) < int(Y)
        if Y.ndim != 1 or len(Y) != N or Y.dtype.kind != 'b':
            raise ValueError(f'Y: a boolean membership vector of length {N} '
                             f'expected, got {Y.dtype} of shape {Y.shape}')
        return Y

    def _evaluate(self, X, Y, B, seed):
        """(statistics of the B + 1 splits, witness, z0, timing)"""
        torch = _torch()
        t = time.perf_counter()
        pooled, z0 = self._pool(X, Y)
        K, adopted = self._gram(pooled)
        if z0 is None:
            z0 = self._membership(Y, K.shape[0])
        n = int(z0.sum())
        m = len(z0) - n
        if n == 0 or m == 0:
            raise ValueError('KernelTwoSampleTest: an empty sample')
        if self.estimator == 'unbiased' and (n < 2 or m < 2):
            raise ValueError("estimator='unbiased' needs at least two points "
                             f'in each sample, got {n} and {m}')
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        Z = _mmd.splits(z0, B, seed)
        s = np.where(z0, 1.0 / n, -1.0 / m)
        (sums, r, d, w), fused = _mmd.solve(K, torch.from_numpy(Z),
                                            torch.from_numpy(s))
        # the one download: 3 (B + 1) + 2 doubles and the witness
        down = torch.cat((sums.reshape(-1), r.sum()[None], d.sum()[None],
                          w)).cpu().numpy()
        k = 3 * (B + 1)
        stats = _mmd.statistics(down[:k], down[k], down[k + 1], n, m,
                                self.estimator)
        witness = down[k + 2:]
        if not np.all(np.isfinite(witness)):
            raise ValueError('two-sample test: the kernel matrix has entries '
                             'that are not finite')
        timing = {'kernel': t_kernel, 'linalg': time.perf_counter() - t,
                  'adopted': adopted, 'fused': fused}
        return stats, witness, z0, pooled, K.device, timing

    # -- the test --------------------------------------------------------------------
    def fit(self, X, Y):
        """Test the graphs `X` against the graphs `Y` (with a precomputed
        kernel: `X` is the pooled matrix, `Y` the size of the first sample or
        a boolean membership vector)."""
        B = self.n_permutations
        seed = self.random_state
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        stats, witness, z0, pooled, device, timing = self._evaluate(
            X, Y, B, seed)
        self.seed_ = seed
        self.statistic_ = float(stats[0])
        self.null_ = stats[1:].copy()
        # (a permutation that reproduces the split ties with it bit for bit)
        self.pvalue_ = (1 + int(np.sum(self.null_ >= stats[0]))) / (1 + B) \
            if B else None
        self.witness_ = witness
        self.n_ = int(z0.sum())
        self.m_ = len(z0) - self.n_
        self._n = len(z0)
        self.X = None if self._precomputed else pooled
        s = np.where(z0, 1.0 / self.n_, -1.0 / self.m_)
        self._s = _torch().from_numpy(s).to(device)
        self.last_timing = timing
        return self

    def statistic(self, X, Y):
        """The squared MMD of the two samples alone: no permutations, nothing
        kept."""
        return float(self._evaluate(X, Y, 0, 0)[0][0])

    def reject(self, alpha=0.05):
        """Whether the hypothesis of one common distribution is rejected at
        the level `alpha`."""
        if getattr(self, 'pvalue_', None) is None:
            raise ValueError('KernelTwoSampleTest: reject needs a fit with '
                             'n_permutations > 0')
        return bool(self.pvalue_ <= alpha)

    def witness(self, G):
        """The witness function at the graphs `G` (with a precomputed kernel:
        at the rows of a (b, N) cross matrix against the pooled sample)."""
        if not hasattr(self, '_s'):
            raise ValueError('KernelTwoSampleTest: witness before fit')
        torch = _torch()
        Ks = self._cross(G, self._s.device)
        return (Ks.to(torch.float64) @ self._s).cpu().numpy()
