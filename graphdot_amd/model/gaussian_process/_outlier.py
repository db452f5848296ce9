"""Host side of outlier.hip, the fused epilogue of the outlier detector's
likelihood: compiles the kernels once (JIT cache of graphdot_amd.hip.jit,
IEEE arithmetic: no fast-math) and runs them on torch's *current* stream of
the matrices' device, in stream order with the torch operations around them.
Three launches per call (the rows of the inverse, the pass over the gradient
planes, the fixed-order reduction) and no host synchronisation."""
import numpy as np
from ...hip.source_module import STATIC, current_stream, suffix
from .._dense_host import _contract_planes, plane_strides, triangle_grid

_module = STATIC['outlier.hip']
_BLOCK = 256
_WAVES = 4          # rows per workgroup of od_rows (one per wave)
_SUB = 4            # workgroups per tile (TILE / SUB columns each)
#: od_planes runs tiles x SUB x chunks workgroups
grid = triangle_grid


def _check_square(name, A, n):
    import torch
    if A.dtype != torch.float64 or tuple(A.shape) != (n, n):
        raise TypeError(f'{name}: ({n}, {n}) float64 expected')
    if n > 1 and A.stride() != (n, 1):
        raise ValueError(f'{name} must be row-major contiguous')


def epilogue(Kinv, Ks, y, sigma2, P=None, planes=()):
    """``[y^T a, ||Ks||_inf, ||Kinv||_inf, d_theta, d_alpha]`` as one float64
    tensor on Kinv's device, enqueued on torch's current stream, with
    ``a = Kinv y``, ``d_theta[k] = sum_ij (Kinv_ij - a_i a_j)
    P[i, j, planes[k]]`` and ``d_alpha_i = (Kinv_ii - a_i^2) 2 sigma2_i``.

    Kinv, Ks: (n, n) float64 CUDA tensors, row-major contiguous, symmetric.
    y, sigma2: n float64 values (tensors on the device or host arrays).
    P: None or the (n, n, m) symmetric gradient planes in float32 or float64,
    any strides with positive values (read as they lie; the kernel's
    `device_gram` hands them over column-major).  planes: indices into the
    m planes (`active_theta_mask`)."""
    import torch
    n = Kinv.shape[0]
    if not Kinv.is_cuda:
        raise TypeError('epilogue runs on CUDA tensors; see epilogue_torch')
    _check_square('Kinv', Kinv, n)
    _check_square('Ks', Ks, n)
    dev = Kinv.device
    if Ks.device != dev:
        raise ValueError('Kinv and Ks must be on the same device')
    planes = np.asarray(planes, dtype=np.int64).ravel()
    nt = len(planes)
    if nt:
        if P is None or P.dim() != 3 or P.dtype not in (torch.float32,
                                                        torch.float64):
            raise TypeError('P: (n, n, m) float32 or float64 planes expected')
        if tuple(P.shape[:2]) != (n, n) or P.device != dev:
            raise ValueError(f'P: ({n}, {n}, m) planes on {dev} expected')
        if planes.min() < 0 or planes.max() >= P.shape[2]:
            raise IndexError('plane index out of range')
        if min(P.stride()) < 0:
            raise ValueError('P: negative strides')
    y = torch.as_tensor(y, dtype=torch.float64).to(dev).contiguous()
    sigma2 = torch.as_tensor(sigma2, dtype=torch.float64).to(dev).contiguous()
    if y.shape != (n,) or sigma2.shape != (n,):
        raise ValueError(f'y and sigma2: {n} values expected')
    with torch.cuda.device(dev):
        out = torch.zeros(3 + nt + n, dtype=torch.float64, device=dev)
        if n == 0:
            return out
        stream = current_stream(dev)
        rows = torch.empty(5 * n, dtype=torch.float64, device=dev)
        _module.launch('od_rows', -(-n // _WAVES), _BLOCK, 'QQqQQQ',
                       Kinv.data_ptr(), Ks.data_ptr(), n, y.data_ptr(),
                       sigma2.data_ptr(), rows.data_ptr(), stream=stream)
        kc, ntiles, gz = grid(n, nt)
        nblk = ntiles * _SUB
        partial = torch.empty(max(nt, 1) * nblk, dtype=torch.float64,
                              device=dev)
        if nt:
            pidx = torch.from_numpy(planes).to(dev)
            s_lane, s_col, s_k = plane_strides(P)
            _module.launch(
                f'od_planes_{suffix(P.dtype)}_k{kc}', nblk * gz, _BLOCK,
                'QqqqqQiQQqQ', P.data_ptr(), n, s_lane, s_col, s_k,
                pidx.data_ptr(), nt, Kinv.data_ptr(), rows.data_ptr(), ntiles,
                partial.data_ptr(), stream=stream)
        _module.launch('od_reduce', 3 + nt + -(-n // _BLOCK), _BLOCK,
                       'QqQqiQ', rows.data_ptr(), n, partial.data_ptr(), nblk,
                       nt, out.data_ptr(), stream=stream)
    return out


def epilogue_torch(Kinv, Ks, y, sigma2, P=None, planes=()):
    """The same buffer by torch on any device: the yardstick of the kernels
    and the CPU path of the detector."""
    import torch
    dev = Kinv.device
    y = torch.as_tensor(y, dtype=torch.float64).to(dev)
    sigma2 = torch.as_tensor(sigma2, dtype=torch.float64).to(dev)
    a = Kinv @ y
    head = torch.stack(((y * a).sum(), Ks.abs().sum(1).max(),
                        Kinv.abs().sum(1).max())) if len(y) else \
        torch.zeros(3, dtype=torch.float64, device=dev)
    d_alpha = (torch.diagonal(Kinv) - a * a) * 2.0 * sigma2
    planes = np.asarray(planes, dtype=np.int64).ravel()
    if len(planes):
        dK = P if P.shape[2] == len(planes) and \
            np.array_equal(planes, np.arange(P.shape[2])) else \
            P.index_select(2, torch.as_tensor(planes, device=P.device))
        d_theta = _contract_planes(Kinv - torch.outer(a, a),
                                   dK.to(torch.float64))
    else:
        d_theta = torch.zeros(0, dtype=torch.float64, device=dev)
    return torch.cat((head, d_theta, d_alpha))
