"""``VarianceMinimizer`` of the reference
(graphdot/model/active_learning/variance_minimizer.py), greedy on a kernel
matrix that stays on the GPU (select.hip) or on the host (numpy)."""
from ._greedy import gram, resolve_device, run


class VarianceMinimizer:
    '''Select a subset of a dataset such that the Gaussian process posterior
    variance, i.e. the Nystrom residual norm, of the kernel matrix of the
    UNSELECTED samples is as small as possible: the chosen samples span the
    space the whole dataset occupies in a reproducing kernel Hilbert space.

    Each pick is the unselected sample with the largest row sum of the
    posterior covariance over the unselected samples (a partial pivoted
    Cholesky factorisation of ``K + alpha I``).  Ties go to the smallest
    index (the reference's loop breaks them in its own swapped order).

    Parameters
    ----------
    kernel: callable or 'precomputed'
        A symmetric positive semidefinite function implemented via the
        ``__call__`` semantics.  'precomputed': a square kernel matrix (numpy
        array or torch tensor) is expected as the argument to ``__call__``.
        A kernel with ``device_gram`` computes the matrix on the GPU and the
        selection reads it there.
    alpha: float, default=1e-6
        A small value added to the diagonal elements of the kernel matrix in
        order to regularize the variance calculations.
    kernel_options: dict
        Additional arguments to be passed into the kernel.
    device: 'auto', 'cuda' or 'cpu'
        Where the selection runs ('auto': the GPU if torch sees one).

    Raises ``SelectionError`` from ``__call__`` when a pick's posterior
    variance is not positive (rank below ``n``; only possible with a tiny or
    zero ``alpha``).
    '''

    def __init__(self, kernel, alpha=1e-6, kernel_options=None,
                 device='auto'):
        assert kernel == 'precomputed' or callable(kernel)
        self.kernel = kernel
        self.alpha = alpha
        self.kernel_options = kernel_options or {}
        self.device = device

    def __call__(self, X, n):
        '''Find a n-sample subset of X that attempts to maximize the diversity
        and return the indices of the samples.

        Parameters
        ----------
        X: feature matrix or list of objects
            Input dataset.
        n: int
            Number of samples to be chosen.

        Returns
        -------
        chosen: list
            Indices of the samples that are chosen.
        '''
        assert len(X) >= n
        if n == 0:
            return []
        device = resolve_device(self.device)
        return run(gram(self, X, device), n, 'variance', alpha=self.alpha)
