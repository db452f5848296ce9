"""Host side of mmd.hip, the fused sums of the kernel two-sample test (mmd.py;
DESIGN.md section 32): compiles the kernels once (JIT cache of
graphdot_amd.hip.jit, IEEE arithmetic: no fast-math) and runs them on torch's
*current* stream of the matrix's device, in stream order with the torch
operations around them.  Three launches per call (the row sums and the
witness, the pass over the matrix, the fixed-order reduction), no host
synchronisation, a workspace of ``ceil(n / 64) rows`` doubles and nothing of
size n x n or, in a floating type, n x rows written.  `forms_torch` is the same
chain through torch on any device: the restatement the kernels are compared
with, and the path of CPU tensors.  `splits` draws the permutations on the
host and `statistics` turns the downloaded sums into the two estimators."""
import numpy as np
from ...hip.source_module import (
    CHUNKS, STATIC, chunk, current_stream, suffix)
from .._dense_host import matrix_strides

_module = STATIC['mmd.hip']
precompile = _module.precompile
_BLOCK = 256
_WAVES = 4          # rows / splits per workgroup of mmd_rows and mmd_reduce
_TILE = 64          # rows per strip, and splits per chunk, of mmd_forms
#: splits per block of `forms_torch`
TORCH_BLOCK = 1024
ESTIMATORS = ('unbiased', 'biased')


def splits(z0, B, seed):
    """The (B + 1, N) uint8 splits of a test: row 0 is the observed split
    `z0` (ones for the members of the first sample), rows 1 .. B are
    ``default_rng(seed).permuted(tile(z0, (B, 1)), axis=1)``.  Made on the
    host: the same on every device."""
    z0 = np.ascontiguousarray(z0, dtype=np.uint8).ravel()
    Z = np.empty((B + 1, len(z0)), dtype=np.uint8)
    Z[0] = z0
    if B:
        Z[1:] = np.random.default_rng(seed).permuted(
            np.tile(z0, (B, 1)), axis=1)
    return Z


#: most chunks of 64 splits per workgroup of mmd_forms (the kernels exist for
#: the chunk sizes up to it; larger ones measured slower)
KC_MOST = 4
KCS = tuple(k for k in CHUNKS if k <= KC_MOST)


def grid(n, rows, kc=None):
    """(chunk size KC, strips of 64 rows, groups of 64 KC splits): mmd_forms
    runs strips x groups workgroups.  KC is the chunk size that holds the
    chunks of 64 splits, `KC_MOST` at the most, or `kc` where one is given.
    A function of the shapes alone -- and no sum depends on KC."""
    chunks = -(-rows // _TILE)
    if kc is None:
        kc = chunk(min(chunks, KC_MOST))
    elif kc not in KCS:
        raise ValueError(f'kc: one of {KCS} expected, got {kc}')
    return kc, -(-n // _TILE), -(-chunks // kc)


def _check(K, Z, s):
    """(n, rows) of checked arguments, any device."""
    import torch
    if not torch.is_tensor(K) or K.dim() != 2 or K.shape[0] != K.shape[1] \
            or K.dtype not in (torch.float32, torch.float64):
        raise TypeError('K: a square float32 or float64 tensor expected')
    n = K.shape[0]
    if not torch.is_tensor(Z) or Z.dtype != torch.uint8 or Z.dim() != 2 \
            or Z.shape[1] != n or Z.shape[0] < 1:
        raise TypeError(f'Z: (rows, {n}) uint8 splits, rows >= 1, expected')
    if not torch.is_tensor(s) or s.dtype != torch.float64 \
            or tuple(s.shape) != (n,):
        raise TypeError(f's: ({n},) float64 witness weights expected')
    if min(K.stride()) < 0:
        raise ValueError('K: negative strides')
    return n, Z.shape[0]


def forms(K, Z, s, kc=None):
    """``(sums, r, d, w)`` as float64 tensors on K's device, enqueued on
    torch's current stream (`mmd_rows_*`, `mmd_forms_*`, `mmd_reduce`):
    ``sums[b] = (z^T K z, z^T r, z^T d)`` for the split ``z = Z[b]``, ``r =
    K 1``, ``d = diag K`` and ``w = K s``.  The sums of a split depend on that
    split and K alone, not on its row or on the number of rows.

    K: (n, n) symmetric float32 or float64 CUDA tensor, any strides with
    positive values (read as it lies).  Z: (rows, n) uint8 zeros and ones
    (nothing else: the kernels read bit 0), s: (n,) float64, both on any
    device.  kc: the chunk size of `grid` in the place of its own choice
    (the same bits with every one)."""
    import torch
    n, rows = _check(K, Z, s)
    if not K.is_cuda:
        raise TypeError('K: a CUDA tensor expected; see forms_torch')
    dev = K.device
    Z = Z.to(dev).contiguous()
    s = s.to(dev).contiguous()
    with torch.cuda.device(dev):
        sums = torch.zeros((rows, 3), dtype=torch.float64, device=dev)
        r, d, w = torch.zeros((3, n), dtype=torch.float64, device=dev)
        if n == 0:
            return sums, r, d, w
        stream = current_stream(dev)
        sfx = suffix(K.dtype)
        k_lane, k_col = matrix_strides(K)
        _module.launch(f'mmd_rows_{sfx}', -(-n // _WAVES), _BLOCK, 'QqqqQQQQ',
                       K.data_ptr(), n, k_lane, k_col, s.data_ptr(),
                       r.data_ptr(), d.data_ptr(), w.data_ptr(),
                       stream=stream)
        kc, nb, groups = grid(n, rows, kc)
        partial = torch.empty(nb * rows, dtype=torch.float64, device=dev)
        _module.launch(f'mmd_forms_{sfx}_k{kc}', nb * groups, _BLOCK,
                       'QqqqQqqQ', K.data_ptr(), n, k_lane, k_col,
                       Z.data_ptr(), rows, nb, partial.data_ptr(),
                       stream=stream)
        _module.launch('mmd_reduce', -(-rows // _WAVES), _BLOCK, 'QqQqqQQQ',
                       partial.data_ptr(), nb, Z.data_ptr(), rows, n,
                       r.data_ptr(), d.data_ptr(), sums.data_ptr(),
                       stream=stream)
    return sums, r, d, w


def forms_torch(K, Z, s):
    """The same four tensors by torch on any device, in blocks of at most
    `TORCH_BLOCK` splits (the restatement stores K in double and, per block,
    the splits in double and their products with K)."""
    import torch
    n, rows = _check(K, Z, s)
    dev = K.device
    Kd = K.to(torch.float64)
    Z, s = Z.to(dev), s.to(dev)
    r, d, w = Kd.sum(1), Kd.diagonal().clone(), Kd @ s
    sums = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    for b in range(0, rows, TORCH_BLOCK):
        Zb = Z[b:b + TORCH_BLOCK].to(torch.float64)
        sums[b:b + TORCH_BLOCK, 0] = ((Zb @ Kd) * Zb).sum(1)
        sums[b:b + TORCH_BLOCK, 1] = Zb @ r
        sums[b:b + TORCH_BLOCK, 2] = Zb @ d
    return sums, r, d, w


def solve(K, Z, s):
    """(``(sums, r, d, w)``, fused?): `forms` for a CUDA matrix,
    `forms_torch` anywhere else."""
    if K.is_cuda:
        return forms(K, Z, s), True
    return forms_torch(K, Z, s), False


def statistics(sums, t, dt, n, m, estimator):
    """The squared MMD of every split from its downloaded sums ``(q, u, dz)``,
    ``t = sum r`` and ``dt = sum d``, for first samples of `n` and second
    samples of `m` points, in numpy double: with ``S_xx = q``, ``S_xy = u -
    q`` and ``S_yy = t - 2 u + q``,

    biased:    ``S_xx / n^2 + S_yy / m^2 - 2 S_xy / (n m)``
    unbiased:  ``(S_xx - dz) / (n (n - 1)) + (S_yy - (dt - dz)) / (m (m - 1))
               - 2 S_xy / (n m)``

    ValueError where `t` or `dt` is not finite."""
    if estimator not in ESTIMATORS:
        raise ValueError(f'estimator: one of {ESTIMATORS} expected, got '
                         f'{estimator!r}')
    t, dt = float(t), float(dt)
    if not (np.isfinite(t) and np.isfinite(dt)):
        raise ValueError('two-sample test: the kernel matrix has entries '
                         'that are not finite')
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 3)
    q, u, dz = sums[:, 0], sums[:, 1], sums[:, 2]
    n, m = float(n), float(m)
    sxx, sxy, syy = q, u - q, t - 2.0 * u + q
    if estimator == 'biased':
        return sxx / (n * n) + syy / (m * m) - 2.0 * sxy / (n * m)
    if n < 2 or m < 2:
        raise ValueError("estimator='unbiased' needs at least two points in "
                         f'each sample, got {int(n)} and {int(m)}')
    return (sxx - dz) / (n * (n - 1.0)) \
        + (syy - (dt - dz)) / (m * (m - 1.0)) - 2.0 * sxy / (n * m)
