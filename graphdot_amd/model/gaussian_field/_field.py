"""Host side of field.hip, the fused weight-matrix kernels of the Gaussian
field regressor: compiles them once (JIT cache of graphdot_amd.hip.jit, IEEE
arithmetic: no fast-math) and runs them on torch's *current* stream of the
block's device, in stream order with the torch operations around them.  Two
launches per call (the pass over the block, the fixed-order reduction of its
per-workgroup sums) and no host synchronisation."""
import numpy as np
from ...hip.source_module import STATIC, chunk, current_stream, suffix

_module = STATIC['field.hip']
precompile = _module.precompile
_BLOCK = 256
_ROWS = 64           # rows per workgroup (one per lane)
_WAVES = 4           # columns per workgroup and step (one per wave)
_TARGET_BLOCKS = 2048          # workgroups to aim for (256 CUs x 8)
#: the kernel-induced distance's constants (KernelInducedDistance)
HALF = 0.4999997
EPS = 1e-4


def grid(Nr, Nc, n):
    """(chunk size KC, row tiles gx, column sets gy, chunks gz): a function
    of the shapes alone, so that the order of every sum is the same on every
    call.  (`n` = 0: gf_rowsums, one chunk.)"""
    kc = chunk(n)
    gz = max(1, -(-n // kc))
    gx = -(-Nr // _ROWS)
    gy = max(1, min(-(-Nc // _WAVES), -(-_TARGET_BLOCKS // (gx * gz))))
    return kc, gx, gy, gz


def _vec(a, n, dev, what):
    """float64 vector of length n on `dev` (contiguous), or None."""
    import torch
    if a is None:
        return None
    a = torch.as_tensor(a, device=dev, dtype=torch.float64).contiguous()
    if a.shape != (n,):
        raise ValueError(f'{what}: shape {(n,)} expected, got {tuple(a.shape)}')
    return a


def _mat(a, n, m, dev, what):
    """float64 (n, m) column-major on `dev`, or None."""
    import torch
    if a is None:
        return None
    a = torch.as_tensor(a, device=dev, dtype=torch.float64)
    if tuple(a.shape) != (n, m):
        raise ValueError(f'{what}: shape {(n, m)} expected, '
                         f'got {tuple(a.shape)}')
    return a.t().contiguous().t() if n > 0 and m > 0 else a.contiguous()


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _check_block(K, kr, kc):
    import torch
    if K.dim() != 2:
        raise ValueError('K: a 2-D block expected')
    if not K.is_cuda:
        raise TypeError('the field kernels run on CUDA tensors')
    suffix(K.dtype)
    Nr, Nc = K.shape
    return Nr, Nc, _vec(kr, Nr, K.device, 'kr'), _vec(kc, Nc, K.device, 'kc')


def rowsums(K, kr, kc, sigma, smoothing, self_block, y=None, write=False,
            half=HALF):
    """Per row of the weight block of K: ``s = sum_c (w + smoothing)``,
    ``t = sum_c (w + smoothing) y_c`` (zeros if `y` is None) and, with
    `write`, the float64 block ``w + smoothing`` (column-major).  Returns
    (s, t, W or None), float64 tensors on K's device, enqueued on torch's
    current stream."""
    import torch
    Nr, Nc, kr, kc = _check_block(K, kr, kc)
    dev = K.device
    y = _vec(y, Nc, dev, 'y')
    with torch.cuda.device(dev):
        s = torch.zeros(Nr, dtype=torch.float64, device=dev)
        t = torch.zeros(Nr, dtype=torch.float64, device=dev)
        W = (torch.empty((Nc, Nr), dtype=torch.float64, device=dev).t()
             if write else None)
        if Nr == 0 or Nc == 0:
            return s, t, W
        stream = current_stream(dev)
        _, gx, gy, _ = grid(Nr, Nc, 0)
        ps = torch.empty(gy * Nr, dtype=torch.float64, device=dev)
        pt = torch.empty(gy * Nr, dtype=torch.float64, device=dev)
        _module.launch(
            f'gf_rowsums_{suffix(K.dtype)}', gx * gy, _BLOCK,
            'QqqqqQQdddiQQiiQQ', K.data_ptr(), K.stride(0), K.stride(1), Nr,
            Nc, kr.data_ptr(), kc.data_ptr(), half, float(sigma)**-2,
            float(smoothing), int(bool(self_block)), _ptr(y), _ptr(W), gx, gy,
            ps.data_ptr(), pt.data_ptr(), stream=stream)
        _module.launch(
            'gf_rowsums_reduce', -(-Nr // _BLOCK), _BLOCK, 'QQqiQQ',
            ps.data_ptr(), pt.data_ptr(), Nr, gy, s.data_ptr(), t.data_ptr(),
            stream=stream)
    return s, t, W


def contract(K, kr, kc, dkr, dkc, sigma, alpha, beta, gamma, P, planes,
             self_block, row=None, col=None, u=None, v=None, eps=EPS,
             half=HALF):
    """The gradient sums of one block (field.hip, gf_contract): a float64
    tensor of ``n + 1`` numbers, the sigma column first, with ``n =
    len(planes)``.  P: (Nr, Nc, n_planes) float32 or float64 tensor of raw
    planes, any strides; `planes`: the n plane indices (host integers) the
    columns stand for.  dkr (Nr, n), dkc (Nc, n), u (Nr, n), v (Nc, n): float64
    (u, v, row, col: None for zeros / ones).  Enqueued on torch's current
    stream; an empty block gives zeros and launches nothing."""
    import torch
    Nr, Nc, kr, kc = _check_block(K, kr, kc)
    dev = K.device
    planes = np.asarray(planes, dtype=np.int64).ravel()
    n = len(planes)
    if P.dim() != 3 or tuple(P.shape[:2]) != (Nr, Nc):
        raise ValueError(f'P: shape ({Nr}, {Nc}, n_planes) expected, '
                         f'got {tuple(P.shape)}')
    if P.device != dev:
        raise ValueError('P and K on different devices')
    suffix(P.dtype)
    if n and (planes.min() < 0 or planes.max() >= P.shape[2]):
        raise IndexError('plane index out of range')
    alpha = _vec(alpha, Nr, dev, 'alpha')
    beta = _vec(beta, Nr, dev, 'beta')
    gamma = _vec(gamma, Nc, dev, 'gamma')
    row = _vec(row, Nr, dev, 'row')
    col = _vec(col, Nc, dev, 'col')
    dkr = _mat(dkr, Nr, n, dev, 'dkr')
    dkc = _mat(dkc, Nc, n, dev, 'dkc')
    u = _mat(u, Nr, n, dev, 'u')
    v = _mat(v, Nc, n, dev, 'v')
    with torch.cuda.device(dev):
        out = torch.zeros(n + 1, dtype=torch.float64, device=dev)
        if Nr == 0 or Nc == 0:
            return out
        pk = torch.from_numpy(planes.astype(np.int32)).to(dev)
        stream = current_stream(dev)
        kc_, gx, gy, gz = grid(Nr, Nc, n)
        nblk = gx * gy
        partial = torch.empty((n + 1) * nblk, dtype=torch.float64,
                              device=dev)
        sigma = float(sigma)
        _module.launch(
            f'gf_contract_{suffix(K.dtype)}_{suffix(P.dtype)}_k{kc_}',
            gx * gy * gz, _BLOCK, 'QqqqqQQQQddddiQQQQqqqQiQQQQiiQ',
            K.data_ptr(), K.stride(0), K.stride(1), Nr, Nc, kr.data_ptr(),
            kc.data_ptr(), _ptr(dkr), _ptr(dkc), half, sigma**-2, sigma**-3,
            float(eps), int(bool(self_block)), alpha.data_ptr(),
            beta.data_ptr(), gamma.data_ptr(), P.data_ptr(), P.stride(0),
            P.stride(1), P.stride(2), pk.data_ptr(), n, _ptr(row), _ptr(col),
            _ptr(u), _ptr(v), gx, gy, partial.data_ptr(), stream=stream)
        _module.launch('gf_reduce', n + 1, _BLOCK, 'QqQ', partial.data_ptr(),
                       nblk, out.data_ptr(), stream=stream)
    return out
