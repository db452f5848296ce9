"""Host side of subspace.hip, the blocked subspace iteration behind
`KernelPCA`: compiles the kernels once (JIT cache of graphdot_amd.hip.jit,
IEEE arithmetic: no fast-math) and runs them on torch's *current* stream of
the matrix's device, in stream order with the torch operations around them.
No launch here synchronises with the host.  Every launch has a ``*_torch``
restatement on any device: the yardstick of the kernels and the host path of
the model.

The block V (n, m) is stored as the rotate before left it, unnormalised; its
column statistics travel beside it as ``vpart = [sum of squares (m, nvb) | sum
(m, nvb)]``, per-block partial sums which every consumer adds up in the same
fixed order (`col_stats_torch`) and applies on load."""
import warnings
import numpy as np
from ...hip.source_module import STATIC, chunk, current_stream, suffix
from .._dense_host import _check_K, _f64

_module = STATIC['subspace.hip']
precompile = _module.precompile
_BLOCK = 256
_WAVE = 64
_WAVES = 4          # rows per workgroup of kpca_colsum (one per wave)
_ROWS = 16          # rows of K per workgroup of kpca_apply
_RB = 64            # rows per workgroup of kpca_rotate
MMAX = 32           # widest block
KMAX = 16           # most components
PD_TOL = 1e-13      # a pivot of S = V^T V below PD_TOL S_jj: not positive definite
#: the host looks at the residuals and the status word after every CHECK_EVERY
#: iterations (one download of 2 m + 1 numbers)
CHECK_EVERY = 4


def block_width(n, k):
    """``m = min(n - 1, max(2 k, k + 8))``: at most MMAX."""
    return min(n - 1, max(2 * k, k + 8))


def grid(n, m):
    """(chunk size KC, row blocks, chunks): kpca_apply runs row blocks x
    chunks workgroups.  A function of the shapes alone, so that the order of
    every sum is the same on every call."""
    kc = chunk(m)
    return kc, -(-n // _ROWS), max(1, -(-m // kc))


def _check_block(V, vpart, n, dev):
    if V.dim() != 2 or not 1 <= V.shape[1] <= MMAX:
        raise ValueError(f'V: (n, m) with 1 <= m <= {MMAX} expected')
    m = V.shape[1]
    V = _f64('V', V, (n, m), dev)
    if vpart.dim() != 2 or vpart.shape[0] != 2 * m or vpart.shape[1] < 1:
        raise ValueError(f'vpart: ({2 * m}, nvb) expected')
    return V, _f64('vpart', vpart, vpart.shape, dev), m


def start_block(n, m, random_state=0, v0=None):
    """(V, vpart) on the host: the start block drawn from `random_state` (or
    `v0`), and its column statistics as one block of partial sums."""
    import torch
    if v0 is None:
        v0 = np.random.default_rng(random_state).normal(size=(n, m))
    v0 = np.ascontiguousarray(v0, dtype=np.float64)
    if v0.shape != (n, m):
        raise ValueError(f'v0: ({n}, {m}) expected, got {v0.shape}')
    vpart = np.concatenate(((v0 * v0).sum(0), v0.sum(0)))[:, None]
    return torch.from_numpy(v0), torch.from_numpy(np.ascontiguousarray(vpart))


def col_stats_torch(vpart, m):
    """(scale, scaled column sums) of the block whose statistics are
    `vpart`; a zero (or NaN) column gets the scale 0."""
    import torch
    a, b = vpart[:m].sum(1), vpart[m:].sum(1)
    scale = torch.where(a > 0, 1.0 / torch.sqrt(a), torch.zeros_like(a))
    return scale, scale * b


# -- the sums of K -------------------------------------------------------------------
def sums(K):
    """``(colsum (n), [sum of K, trace of K])`` as float64 tensors
    (`kpca_colsum_*`, then `kpca_reduce`)."""
    import torch
    n = _check_K(K)
    dev = K.device
    with torch.cuda.device(dev):
        stat = torch.zeros(2 * n, dtype=torch.float64, device=dev)
        tot = torch.zeros(2, dtype=torch.float64, device=dev)
        if n:
            stream = current_stream(dev)
            _module.launch(f'kpca_colsum_{suffix(K.dtype)}', -(-n // _WAVES),
                           _BLOCK, 'QqQ', K.data_ptr(), n, stat.data_ptr(),
                           stream=stream)
            _module.launch('kpca_reduce', 2, _BLOCK, 'QqQ', stat.data_ptr(),
                           n, tot.data_ptr(), stream=stream)
    return stat[:n], tot


def sums_torch(K):
    import torch
    K = K.to(torch.float64)
    colsum = K.sum(0)
    return colsum, torch.stack((colsum.sum(), K.diagonal().sum()))


# -- one iteration: apply, ritz, rotate ----------------------------------------------
def apply(K, V, vpart, out=None):
    """``(Z, part)`` of `kpca_apply_*`: ``Z = K (V s - 1 vmean^T)`` (n, m)
    for the scaled block ``V s`` and ``part`` (row blocks, 2 m^2 + m): per
    row block the shares of ``(V s)^T (V s)``, ``(V s)^T Z`` and ``1^T Z``.

    K: (n, n) float32 or float64 CUDA tensor, symmetric, contiguous along
    either index, 16-byte aligned (read as it lies).  `out`: the pair of
    tensors to write into (new ones otherwise)."""
    import torch
    n = _check_K(K)
    dev = K.device
    V, vpart, m = _check_block(V, vpart, n, dev)
    kc, nrb, gz = grid(n, m)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty((n, m), dtype=torch.float64, device=dev),
                   torch.empty((nrb, 2 * m * m + m), dtype=torch.float64,
                               device=dev))
        Z = _f64('Z', out[0], (n, m), dev)
        part = _f64('part', out[1], (nrb, 2 * m * m + m), dev)
        if n:
            _module.launch(
                f'kpca_apply_{suffix(K.dtype)}_k{kc}', nrb * gz, _BLOCK,
                'QqQiQqQQ', K.data_ptr(), n, V.data_ptr(), m,
                vpart.data_ptr(), vpart.shape[1], Z.data_ptr(),
                part.data_ptr(), stream=current_stream(dev))
    return Z, part


def apply_torch(K, V, vpart, out=None):
    import torch
    m = V.shape[1]
    n = K.shape[0]
    scale, vsum = col_stats_torch(vpart, m)
    Vs = V * scale
    Z = K.to(torch.float64) @ (Vs - vsum / n)
    part = torch.cat(((Vs.T @ Vs).reshape(-1), (Vs.T @ Z).reshape(-1),
                      Z.sum(0)))
    return Z, part[None, :]


def ritz(part, vpart, n, m, out=None):
    """``(R, info, cols)`` of `kpca_ritz`: ``R`` (m, m) with ``R^T S R = I``
    and ``R^T G R = diag(w)``, w descending, for ``S = V^T V`` and ``G = V^T
    H Z``; ``info = [w (m) | (m, for the residuals) | status]``; ``cols =
    [scale | V^T 1 | 1^T Z / n]``.  Status bit 0: S is not positive
    definite; bit 1: the Jacobi sweeps reached their cap; the bits of an
    `info` handed in through `out` stay set."""
    import torch
    dev = part.device
    if not part.is_cuda:
        raise TypeError('part: a CUDA tensor expected; see ritz_torch')
    if not 1 <= m <= MMAX:
        raise ValueError(f'1 <= m <= {MMAX} expected')
    rec = 2 * m * m + m
    if part.dim() != 2 or part.shape[1] != rec or part.shape[0] < 1:
        raise ValueError(f'part: (row blocks, {rec}) expected')
    part = _f64('part', part, part.shape, dev)
    if vpart.dim() != 2 or vpart.shape[0] != 2 * m or vpart.shape[1] < 1:
        raise ValueError(f'vpart: ({2 * m}, nvb) expected')
    vpart = _f64('vpart', vpart, vpart.shape, dev)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty((m, m), dtype=torch.float64, device=dev),
                   torch.zeros(2 * m + 1, dtype=torch.float64, device=dev),
                   torch.empty(3 * m, dtype=torch.float64, device=dev))
        R = _f64('R', out[0], (m, m), dev)
        info = _f64('info', out[1], (2 * m + 1,), dev)
        cols = _f64('cols', out[2], (3 * m,), dev)
        _module.launch('kpca_ritz', 1, _BLOCK, 'QqiqQqQQQ', part.data_ptr(),
                       part.shape[0], m, n, vpart.data_ptr(), vpart.shape[1],
                       R.data_ptr(), info.data_ptr(), cols.data_ptr(),
                       stream=current_stream(dev))
    return R, info, cols


def ritz_torch(part, vpart, n, m, out=None):
    """The same with `torch.linalg.eigh` in the place of the Jacobi sweeps
    (the columns of R agree up to their signs where the Ritz values are
    distinct)."""
    import torch
    mm = m * m
    scale, vsum = col_stats_torch(vpart, m)
    tot = part.sum(0)
    S = tot[:mm].reshape(m, m)
    zmean = tot[2 * mm:] / n
    G = tot[mm:2 * mm].reshape(m, m) - torch.outer(vsum, zmean)
    G = 0.5 * (G + G.T)
    info = torch.zeros(2 * m + 1, dtype=torch.float64, device=part.device)
    if out is not None:
        info[2 * m] = out[1][2 * m]
    cols = torch.cat((scale, vsum, zmean))
    L, fail = torch.linalg.cholesky_ex(0.5 * (S + S.T))
    d = torch.diagonal(L)
    if int(fail) != 0 or not bool((d * d > PD_TOL * torch.diagonal(S)).all()):
        info[:m] = float('nan')
        info[2 * m] = float(int(info[2 * m]) | 1)
        return torch.full_like(S, float('nan')), info, cols
    X = torch.linalg.solve_triangular(L, G, upper=False)
    T = torch.linalg.solve_triangular(L, X.T, upper=False)
    w, C = torch.linalg.eigh(0.5 * (T + T.T))
    order = torch.argsort(w, descending=True, stable=True)
    info[:m] = w[order]
    R = torch.linalg.solve_triangular(L.T, C[:, order], upper=True)
    return R, info, cols


def rotate(V, Z, R, info, cols, out=None):
    """``(Vr, Vnext, rpart)`` of `kpca_rotate`: ``Vr = (V s) R``, the next
    block ``Vnext = (Z - 1 zmean^T) R`` and ``rpart`` (3 m, row blocks): per
    row block the shares of the columns' ``sum Vnext^2``, ``sum Vnext`` (the
    first 2 m rows are the next block's `vpart`) and ``sum (Vnext - w
    Vr)^2``."""
    import torch
    if not V.is_cuda:
        raise TypeError('V: a CUDA tensor expected; see rotate_torch')
    dev = V.device
    if V.dim() != 2 or not 1 <= V.shape[1] <= MMAX:
        raise ValueError(f'V: (n, m) with 1 <= m <= {MMAX} expected')
    n, m = V.shape
    V, Z = _f64('V', V, (n, m), dev), _f64('Z', Z, (n, m), dev)
    R = _f64('R', R, (m, m), dev)
    info = _f64('info', info, (2 * m + 1,), dev)
    cols = _f64('cols', cols, (3 * m,), dev)
    nb = -(-n // _RB)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty((n, m), dtype=torch.float64, device=dev),
                   torch.empty((n, m), dtype=torch.float64, device=dev),
                   torch.empty((3 * m, max(nb, 1)), dtype=torch.float64,
                               device=dev))
        Vr, Vnext = (_f64(name, t, (n, m), dev)
                     for name, t in (('Vr', out[0]), ('Vnext', out[1])))
        rpart = _f64('rpart', out[2], (3 * m, max(nb, 1)), dev)
        if n and Vnext.data_ptr() in (V.data_ptr(), Z.data_ptr()):
            raise ValueError('the next block cannot overwrite V or Z')
        if n:
            _module.launch('kpca_rotate', nb, _BLOCK, 'QQqiQQQQQQ',
                           V.data_ptr(), Z.data_ptr(), n, m, R.data_ptr(),
                           info.data_ptr(), cols.data_ptr(), Vr.data_ptr(),
                           Vnext.data_ptr(), rpart.data_ptr(),
                           stream=current_stream(dev))
        else:
            rpart.zero_()
    return Vr, Vnext, rpart


def rotate_torch(V, Z, R, info, cols, out=None):
    import torch
    m = V.shape[1]
    Vr = (V * cols[:m]) @ R
    Yr = (Z - cols[2 * m:]) @ R
    D = Yr - info[:m] * Vr
    rpart = torch.cat(((Yr * Yr).sum(0), Yr.sum(0), (D * D).sum(0)))
    return Vr, Yr, rpart[:, None]


def residuals(rpart, info):
    """Adds the residual shares of `rpart` up into ``info[m:2 m]`` (squared
    norms; `kpca_reduce`), in place."""
    import torch
    m = rpart.shape[0] // 3
    dev = rpart.device
    rpart = _f64('rpart', rpart, (3 * m, rpart.shape[1]), dev)
    info = _f64('info', info, (2 * m + 1,), dev)
    with torch.cuda.device(dev):
        _module.launch('kpca_reduce', m, _BLOCK, 'QqQ',
                       rpart[2 * m:].data_ptr(), rpart.shape[1],
                       info[m:].data_ptr(), stream=current_stream(dev))
    return info


def residuals_torch(rpart, info):
    m = rpart.shape[0] // 3
    info[m:2 * m] = rpart[2 * m:].sum(1)
    return info


class Result:
    """What `iterate` found: `w` (m) Ritz values, `V` (n, m) Ritz vectors
    (device tensor), `residuals` (m), `n_iter`, `status` of kpca_ritz and
    `converged`."""

    def __init__(self, w, V, res, n_iter, status, converged):
        self.w, self.V, self.residuals = w, V, res
        self.n_iter, self.status, self.converged = n_iter, status, converged


def iterate(K, k, tol=1e-10, max_iter=100, random_state=0, v0=None):
    """Blocked subspace iteration on ``H K H`` for its `k` largest
    eigenpairs, with the block width `block_width`: the HIP launches for a
    CUDA matrix, their restatements for a CPU one.  Three launches per
    iteration on the current stream and no download, except after every
    `CHECK_EVERY`-th iteration (4, 8, 12, ...: a function of nothing but that
    constant) and after the last one: then one more launch adds the residual
    shares up and the host reads ``info = [w | |r|^2 | status]`` (2 m + 1
    numbers).  Converged when the first k residual norms are ``<= tol
    |w_0|``; a set status word ends the run at the next look."""
    import torch
    n = K.shape[0]
    m = block_width(n, k)
    V, vpart = start_block(n, m, random_state, v0)
    if K.is_cuda:
        fns = (apply, ritz, rotate, residuals)
        V, vpart = V.to(K.device), vpart.to(K.device)
    else:
        fns = (apply_torch, ritz_torch, rotate_torch, residuals_torch)
        K = K.to(torch.float64)
    f_apply, f_ritz, f_rotate, f_res = fns
    out = None
    # (each launch writes into the tensors of the iteration before; the
    # block and its statistics are read while the next ones are written, so
    # two sets of them alternate)
    o_apply = o_ritz = None
    o_rotate = [None, None]
    for it in range(1, max_iter + 1):
        o_apply = Z, part = f_apply(K, V, vpart, o_apply)
        o_ritz = R, info, cols = f_ritz(part, vpart, n, m, o_ritz)
        o_rotate[it % 2] = Vr, V, rpart = f_rotate(V, Z, R, info, cols,
                                                   o_rotate[it % 2])
        vpart = rpart[:2 * m]
        if it % CHECK_EVERY and it != max_iter:
            continue
        h = f_res(rpart, info).cpu().numpy()
        w, res, status = h[:m], np.sqrt(h[m:2 * m]), int(h[2 * m])
        done = status == 0 and bool(np.all(res[:k] <= tol * abs(w[0])))
        out = Result(w, Vr, res, it, status, done)
        if done or status:
            break
    return out


# -- the projection of new rows ------------------------------------------------------
def project(Ks, A, colmean, gmean):
    """``(Ks - rowmean 1^T - 1 colmean^T + gmean) A`` (b, k) as a float64
    tensor on A's device, in one launch of `kpca_project_*`.

    Ks: (b, n) float32 or float64 CUDA tensor, any positive strides (read
    as it lies; column-major, as the solver leaves it, is the coalesced
    one).  A: (n, k) float64, k <= 16.  colmean: (n,) float64."""
    import torch
    if not A.is_cuda:
        raise TypeError('A: a CUDA tensor expected; see project_torch')
    dev = A.device
    if A.dim() != 2 or not 1 <= A.shape[1] <= KMAX:
        raise ValueError(f'A: (n, k) with 1 <= k <= {KMAX} expected')
    n, k = A.shape
    A = _f64('A', A, (n, k), dev)
    colmean = _f64('colmean', colmean, (n,), dev)
    if Ks.dim() != 2 or Ks.shape[1] != n \
            or Ks.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'Ks: (b, {n}) float32 or float64 expected')
    if Ks.device != dev:
        raise ValueError('Ks and A must be on the same device')
    if min(Ks.stride()) < 0:
        raise ValueError('Ks: negative strides')
    b = Ks.shape[0]
    with torch.cuda.device(dev):
        out = torch.zeros((b, k), dtype=torch.float64, device=dev)
        if b and n:
            _module.launch(
                f'kpca_project_{suffix(Ks.dtype)}_k{chunk(k)}',
                -(-b // _WAVE), _BLOCK, 'QqqqqQiQdQ', Ks.data_ptr(), b, n,
                Ks.stride(0), Ks.stride(1), A.data_ptr(), k,
                colmean.data_ptr(), float(gmean), out.data_ptr(),
                stream=current_stream(dev))
    return out


def project_torch(Ks, A, colmean, gmean):
    import torch
    Ks = Ks.to(torch.float64)
    if Ks.shape[1] == 0:
        return torch.zeros((Ks.shape[0], A.shape[1]), dtype=torch.float64,
                           device=A.device)
    return (Ks - Ks.mean(1, keepdim=True) - colmean + float(gmean)) @ A


def warn_not_converged(result, k, tol, max_iter):
    if result.status & 1:
        why = ('the block lost its rank (V^T V is not positive definite)')
    elif result.status:
        why = 'the Jacobi sweeps of the Ritz problem reached their cap'
    else:
        why = (f'the worst residual after {max_iter} iterations is '
               f'{np.max(result.residuals[:k]):.3g} (tol {tol:g} x '
               f'{abs(result.w[0]):.3g})')
    warnings.warn(f"KernelPCA: eigen_solver='subspace' did not converge: "
                  f"{why}; finishing with 'dense'", UserWarning)
