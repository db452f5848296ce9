"""Host side of alignment.hip, the fused sums of the centred kernel-target
alignment and its gradient (kta.py): compiles the
kernels once (JIT cache of graphdot_amd.hip.jit, IEEE arithmetic: no
fast-math) and runs them on torch's *current* stream of the matrix's device, in
stream order with the torch operations around them.  Three launches per call
(the row sums, the pass over the matrix and the planes, the fixed-order
reduction), no host synchronisation and nothing of size n x n written.
`alignment_torch` is the same chain through torch on any device: the
restatement the kernels are compared with, and the path of CPU tensors and of
more than `KMAX` target columns."""
import numpy as np
from ...hip.source_module import STATIC, current_stream, suffix
from .._dense_host import (_contract_planes, matrix_strides, plane_strides,
                           triangle_grid)

_module = STATIC['alignment.hip']
precompile = _module.precompile
_BLOCK = 256
_WAVES = 4          # indices per workgroup of ka_rows (one per wave)
#: most target columns of the fused path (KT of alignment.hip)
KMAX = 16
#: ka_planes runs tiles x chunks workgroups
grid = triangle_grid


def _check(K, Tc, P, planes):
    """(n, kt, plane indices as int64) of checked arguments, any device."""
    import torch
    floats = (torch.float32, torch.float64)
    if not torch.is_tensor(K) or K.dim() != 2 or K.shape[0] != K.shape[1] \
            or K.dtype not in floats:
        raise TypeError('K: a square float32 or float64 tensor expected')
    n = K.shape[0]
    if not torch.is_tensor(Tc) or Tc.dtype != torch.float64 or Tc.dim() != 2 \
            or Tc.shape[0] != n or Tc.shape[1] < 1:
        raise TypeError(f'Tc: ({n}, k) float64 target columns expected')
    if min(K.stride()) < 0:
        raise ValueError('K: negative strides')
    planes = np.asarray(planes, dtype=np.int64).ravel()
    if len(planes):
        if P is None or not torch.is_tensor(P) or P.dim() != 3 \
                or P.dtype not in floats or tuple(P.shape[:2]) != (n, n) \
                or P.device != K.device:
            raise TypeError(f'P: ({n}, {n}, m) float32 or float64 planes on '
                            f'{K.device} expected')
        if min(P.stride()) < 0:
            raise ValueError('P: negative strides')
        if planes.min() < 0 or planes.max() >= P.shape[2]:
            raise ValueError('plane index out of range')
    return n, Tc.shape[1], planes


def alignment(K, Tc, P=None, planes=()):
    """``[a, b, g, h]`` (2 + 2 m) as one float64 tensor on K's device,
    enqueued on torch's current stream (`ka_rows_*`, `ka_planes_*`,
    `ka_reduce`): ``a = <K_c, w>``, ``b = <K_c, K_c>``, ``g[p] = <dK_p, w>``,
    ``h[p] = <dK_p, K_c>`` with ``K_c = H K H``, ``w = Tc Tc^T`` and ``dK_p =
    P[:, :, planes[p]]``; neither K_c nor w is stored.

    K: (n, n) symmetric float32 or float64 CUDA tensor, any strides with
    positive values (read as it lies).  Tc: the (n, k) centred targets,
    float64, k <= KMAX, on any device.  P: None or the (n, n, m) symmetric
    gradient planes in K's type on K's device, any strides with positive
    values (read as they lie).  planes: indices into the m planes."""
    import torch
    n, kt, planes = _check(K, Tc, P, planes)
    if not K.is_cuda:
        raise TypeError('K: a CUDA tensor expected; see alignment_torch')
    if kt > KMAX:
        raise TypeError(f'Tc: at most KMAX = {KMAX} columns on the fused '
                        f'path, got {kt}; see alignment_torch')
    nt = len(planes)
    if nt and P.dtype != K.dtype:
        raise TypeError(f'P: planes of {K.dtype}, the type of K, expected, '
                        f'got {P.dtype}')
    dev = K.device
    Tc = Tc.to(dev).contiguous()
    with torch.cuda.device(dev):
        out = torch.zeros(2 + 2 * nt, dtype=torch.float64, device=dev)
        if n == 0:
            return out
        stream = current_stream(dev)
        sfx = suffix(K.dtype)
        k_lane, k_col = matrix_strides(K)
        r = torch.empty(n, dtype=torch.float64, device=dev)
        _module.launch(f'ka_rows_{sfx}', -(-n // _WAVES), _BLOCK, 'QqqqQ',
                       K.data_ptr(), n, k_lane, k_col, r.data_ptr(),
                       stream=stream)
        kc, ntiles, gz = grid(n, nt)
        partial = torch.empty((2 + 2 * nt) * ntiles, dtype=torch.float64,
                              device=dev)
        if nt:
            pidx = torch.from_numpy(planes).to(dev)
            p_ptr, pidx_ptr = P.data_ptr(), pidx.data_ptr()
            s_lane, s_col, s_k = plane_strides(P)
        else:                   # (no plane is read: nk = 0 in every chunk)
            p_ptr, pidx_ptr = K.data_ptr(), 0
            s_lane = s_col = s_k = 0
        _module.launch(
            f'ka_planes_{sfx}_k{kc}', ntiles * gz, _BLOCK, 'QqqqQQiQqqqQiqQ',
            K.data_ptr(), n, k_lane, k_col, r.data_ptr(), Tc.data_ptr(), kt,
            p_ptr, s_lane, s_col, s_k, pidx_ptr, nt, ntiles,
            partial.data_ptr(), stream=stream)
        _module.launch('ka_reduce', 2 + 2 * nt, _BLOCK, 'QqQ',
                       partial.data_ptr(), ntiles, out.data_ptr(),
                       stream=stream)
    return out


def alignment_torch(K, Tc, P=None, planes=()):
    """The same buffer by torch on any device, for any number of target
    columns (the restatement stores K_c and w, which the kernels form on the
    fly)."""
    import torch
    n, kt, planes = _check(K, Tc, P, planes)
    dev = K.device
    Kd = K.to(torch.float64)
    Tc = Tc.to(dev)
    if n == 0:
        return torch.zeros(2 + 2 * len(planes), dtype=torch.float64,
                           device=dev)
    r = Kd.sum(1)
    Kc = Kd - r[:, None] / n - r[None, :] / n + r.sum() / (n * n)
    W = Tc @ Tc.T
    head = torch.stack(((Kc * W).sum(), (Kc * Kc).sum()))
    if not len(planes):
        return head
    dK = P if P.shape[2] == len(planes) and \
        np.array_equal(planes, np.arange(P.shape[2])) else \
        P.index_select(2, torch.as_tensor(planes, device=dev))
    dK = dK.to(torch.float64)
    return torch.cat((head, _contract_planes(W, dK),
                      _contract_planes(Kc, dK)))


def solve(K, Tc, P=None, planes=()):
    """(``[a, b, g, h]``, fused?): `alignment` for a CUDA matrix, at most
    KMAX target columns and planes of the matrix's type; `alignment_torch`
    anywhere else."""
    if K.is_cuda and Tc.shape[1] <= KMAX and (
            P is None or not len(planes) or P.dtype == K.dtype):
        return alignment(K, Tc, P, planes), True
    return alignment_torch(K, Tc, P, planes), False


def value_and_gradient(a, b, g, h, Lnorm):
    """(A, dA / dtheta) from the downloaded sums and ``Lnorm = ||L_c||_F``:
    ``A = a / (||K_c|| ||L_c||)`` with ``||K_c||^2 = b`` and ``dA_p = g_p /
    (||K_c|| ||L_c||) - A h_p / ||K_c||^2``.  ValueError where a sum is not
    finite or a norm is zero.  A is clipped to [-1, 1], which it can leave
    by rounding alone (Cauchy-Schwarz)."""
    a, b, Lnorm = float(a), float(b), float(Lnorm)
    g, h = np.asarray(g, dtype=np.float64), np.asarray(h, dtype=np.float64)
    if not (np.isfinite(a) and np.isfinite(b) and np.all(np.isfinite(g))
            and np.all(np.isfinite(h))):
        raise ValueError('alignment: the kernel matrix or its gradient has '
                         'entries that are not finite')
    if not np.isfinite(Lnorm):
        raise ValueError('alignment: the targets are not finite')
    if not b > 0:
        raise ValueError('alignment: the centred kernel matrix is zero '
                         '(||K_c|| = 0)')
    if not Lnorm > 0:
        raise ValueError('alignment: the centred targets are zero '
                         '(||L_c|| = 0)')
    norm = np.sqrt(b) * Lnorm
    A = a / norm
    return min(1.0, max(-1.0, A)), g / norm - A * h / b
