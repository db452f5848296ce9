"""``DeterminantMaximizer`` of the reference
(graphdot/model/active_learning/determinant_maximizer.py), greedy on a
kernel matrix that stays on the GPU (select.hip) or on the host (numpy)."""
from ._greedy import gram, resolve_device, run


class DeterminantMaximizer:
    '''Select a subset of a dataset such that the determinant of the kernel
    matrix of the selected samples is as large as possible: the samples are
    as linearly independent as possible in a reproducing kernel Hilbert
    space.

    Each pick is the sample whose row of the kernel matrix, projected off
    the rows chosen before, is longest.  Ties go to the smallest index.  The
    arithmetic is float64 (the reference's loop works in float32), so picks
    whose criteria differ by less than float32 rounding may differ from the
    reference's.

    Parameters
    ----------
    kernel: callable or 'precomputed'
        A symmetric positive semidefinite function implemented via the
        ``__call__`` semantics.  'precomputed': a square kernel matrix (numpy
        array or torch tensor) is expected as the argument to ``__call__``.
        A kernel with ``device_gram`` (the marginalized graph kernel on the
        HIP backend, the wrappers of kernel/fix.py around it) computes the
        matrix on the GPU and the selection reads it there.
    kernel_options: dict
        Additional arguments to be passed into the kernel.
    device: 'auto', 'cuda' or 'cpu'
        Where the selection runs ('auto': the GPU if torch sees one).

    Raises ``SelectionError`` from ``__call__`` when the kernel matrix has
    rank below ``n``.
    '''

    def __init__(self, kernel, kernel_options=None, device='auto'):
        assert kernel == 'precomputed' or callable(kernel)
        self.kernel = kernel
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
        return run(gram(self, X, device), n, 'determinant')
