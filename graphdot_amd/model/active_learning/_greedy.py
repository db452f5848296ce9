"""What the selectors share: where the kernel matrix comes from and lives,
the host (numpy, float64) restatement of the two greedy loops of select.hip,
and the error raised when a pick has no residual left.

Both loops keep the largest criterion and, among exactly equal values, the
smallest index (`np.argmax`; the same rule as select.hip)."""
import numpy as np

#: a pivot whose squared residual is not above this fraction of its own
#: squared size ends the selection with `SelectionError`:
#: DeterminantMaximizer |w|^2 <= DM_TOL |K_i|^2 (w: row i of K off the rows
#: chosen before), VarianceMinimizer p_j <= VM_TOL (K_jj + alpha) (p_j: the
#: posterior variance of j)
DM_TOL = 1e-20
VM_TOL = 1e-13


class SelectionError(np.linalg.LinAlgError):
    """The greedy selection ran out of rank: the next pick's residual is not
    positive (a kernel matrix of rank below `n`, e.g. duplicated samples).
    `picks` holds the indices chosen before it."""

    def __init__(self, message, picks=()):
        super().__init__(message)
        self.picks = list(picks)


def _torch():
    import torch
    return torch


def resolve_device(device):
    """'auto' -> 'cuda' when torch sees a GPU, else 'cpu' (like the dense
    algebra of model.gaussian_process)."""
    if device not in ('auto', 'cuda', 'cpu'):
        raise ValueError(f"device must be 'auto', 'cuda' or 'cpu', "
                         f"not {device!r}")
    if device == 'auto':
        try:
            return 'cuda' if _torch().cuda.is_available() else 'cpu'
        except ImportError:          # pragma: no cover
            return 'cpu'
    return device


def gram(selector, X, device):
    """The square kernel matrix of `X` for `selector` (its `kernel` and
    `kernel_options`): a numpy array on the host for device 'cpu', a CUDA
    tensor otherwise.  A precomputed CUDA tensor and the Gram matrix of a
    kernel with a device path are not downloaded."""
    import sys
    torch = _torch() if device == 'cuda' or 'torch' in sys.modules else None
    if selector.kernel == 'precomputed':
        is_tensor = torch is not None and isinstance(X, torch.Tensor)
        assert (
            (isinstance(X, np.ndarray) or is_tensor) and
            X.ndim == 2 and
            X.shape[0] == X.shape[1]
        ), 'A precomputed kernel matrix must be square.'
        K = X
    else:
        from .._device_kernel import device_call
        K = None
        if device == 'cuda' and not selector.kernel_options:
            # (None: the kernel has no device path)
            K = device_call(selector.kernel, 'device_gram', X)
        if K is None:
            K = selector.kernel(X, **selector.kernel_options)
        elif not isinstance(K, torch.Tensor):
            K = torch.as_tensor(K, device='cuda')
    if device == 'cpu':
        if torch is not None and isinstance(K, torch.Tensor):
            K = K.detach().cpu().numpy()
        return np.asarray(K, dtype=np.float64)
    if not isinstance(K, torch.Tensor):
        K = np.asarray(K)
        if K.dtype not in (np.float32, np.float64):
            K = K.astype(np.float64)
        K = torch.from_numpy(np.ascontiguousarray(K))
    if not K.is_cuda:
        K = K.to('cuda')
    return K


def _argmax(crit, chosen):
    c = np.where(chosen | np.isnan(crit), -np.inf, crit)
    i = int(np.argmax(c))
    if chosen[i] or np.isnan(crit[i]):
        raise SelectionError('no candidate left to choose from')
    return i


def determinant_host(K, n, tol=DM_TOL):
    """Greedy determinant maximisation on the host: the same implicit row
    Gram-Schmidt as select.hip.  `K`: symmetric float64 (N, N)."""
    N = len(K)
    Q = np.zeros((N, n))
    C = np.zeros((n, N))
    rho = np.einsum('ab,ab->a', K, K)
    chosen = np.zeros(N, dtype=bool)
    picks = []
    for s in range(n):
        i = _argmax(rho, chosen)
        w = K[i] - Q[:, :s] @ C[:s, i]
        w2 = w @ w
        if not (w2 > tol * (K[i] @ K[i]) and np.isfinite(w2)):
            raise SelectionError(
                f'DeterminantMaximizer: no residual left at pick {s} (index '
                f'{i}): the kernel matrix has rank {s} or less', picks)
        chosen[i] = True
        picks.append(i)
        q = w / np.sqrt(w2)
        Q[:, s] = q
        C[s] = K @ q
        rho -= C[s]**2
    return picks


def variance_host(K, n, alpha, tol=VM_TOL):
    """Greedy posterior-variance minimisation on the host: the same partial
    pivoted Cholesky of K + alpha I as select.hip.  `K`: symmetric float64
    (N, N), not modified."""
    N = len(K)
    L = np.zeros((N, n))
    crit = K.sum(axis=1) + alpha
    chosen = np.zeros(N, dtype=bool)
    picks = []
    for s in range(n):
        j = _argmax(crit, chosen)
        chosen[j] = True
        p = K[:, j] - L[:, :s] @ L[j, :s]
        p[j] += alpha
        kjj = K[j, j] + alpha
        if not (p[j] > tol * kjj and np.isfinite(p[j])):
            raise SelectionError(
                f'VarianceMinimizer: posterior variance of the pick {s} '
                f'(index {j}) is not positive: the kernel matrix has rank '
                f'{s} or less', picks)
        picks.append(j)
        l = p / np.sqrt(p[j])
        L[:, s] = l
        crit -= p + l * l[~chosen].sum()
    return picks


def run(K, n, method, alpha=0.0):
    """Select `n` indices on the matrix `gram` returned: numpy -> host loop,
    CUDA tensor -> select.hip."""
    tol = DM_TOL if method == 'determinant' else VM_TOL
    if isinstance(K, np.ndarray):
        if method == 'determinant':
            return determinant_host(K, n, tol)
        return variance_host(K, n, alpha, tol)
    from ._select import select, ST_OK, ST_NO_CANDIDATE
    picks, status = select(K, n, method, alpha=alpha, tol=tol)
    if status == ST_OK:
        return [int(i) for i in picks]
    # the picks before the failing one are valid: find how many there are
    done = int(np.argmax(picks < 0)) if (picks < 0).any() else len(picks)
    name = 'DeterminantMaximizer' if method == 'determinant' \
        else 'VarianceMinimizer'
    if status == ST_NO_CANDIDATE:
        raise SelectionError(f'{name}: no candidate left to choose from')
    raise SelectionError(
        f'{name}: no residual left at pick {done - 1}: the kernel matrix has '
        f'rank {done - 1} or less', picks[:done - 1])
