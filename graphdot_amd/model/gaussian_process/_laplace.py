"""Host side of laplace.hip, the fused passes of the Laplace approximation of
the classifier (gpc.py): compiles the kernels once (JIT cache of
graphdot_amd.hip.jit, IEEE arithmetic: no fast-math) and runs them on torch's
*current* stream of the matrices' device, in stream order with the torch
operations around them.  No launch here synchronises with the host.  Every
launch has a ``*_torch`` restatement on any device: the yardstick of the
kernels and the host path of the classifier."""
import numpy as np
from ...hip.source_module import STATIC, current_stream, suffix
from .._dense_host import _contract_planes, plane_strides, triangle_grid

_module = STATIC['laplace.hip']
precompile = _module.precompile
_BLOCK = 256
_WAVES = 4          # rows per workgroup of lp_build / lp_solve / lp_apply
_SUB = 4            # workgroups per tile (TILE / SUB columns each)
#: lp_planes runs tiles x SUB x chunks workgroups
grid = triangle_grid


def _square(name, A, n):
    import torch
    if not A.is_cuda:
        raise TypeError(f'{name}: a CUDA tensor expected; see the *_torch '
                        'restatements')
    if A.dtype != torch.float64 or tuple(A.shape) != (n, n):
        raise TypeError(f'{name}: ({n}, {n}) float64 expected')
    if n > 1 and A.stride() != (n, 1):
        raise ValueError(f'{name} must be row-major contiguous')


def _vector(name, v, m, dev):
    import torch
    if v.dtype != torch.float64 or tuple(v.shape) != (m,) or v.device != dev:
        raise TypeError(f'{name}: {m} float64 values on {dev} expected')
    return v.contiguous()


def _rows(n):
    return -(-n // _WAVES)


# -- one Newton step: build, (potrf.hip), solve, apply -------------------------------
def build(K, f, y, a, B=None, vec=None):
    """``(B, vec, sums)`` of `lp_build`: ``B = I + s K s`` (n, n), ``vec =
    [pi, s, b, g, K b]`` (5 n) at the latent values `f`, and ``sums = [a . f,
    sum log1p(exp(-(2 y - 1) f))]`` (2) for the `f` and `a` given.  `B` and
    `vec` are written into the tensors given, or into new ones."""
    import torch
    n = K.shape[0]
    _square('K', K, n)
    dev = K.device
    f, y, a = (_vector(name, v, n, dev)
               for name, v in (('f', f), ('y', y), ('a', a)))
    with torch.cuda.device(dev):
        if B is None:
            B = torch.empty((n, n), dtype=torch.float64, device=dev)
        if vec is None:
            vec = torch.empty(5 * n, dtype=torch.float64, device=dev)
        _square('B', B, n)
        vec = _vector('vec', vec, 5 * n, dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        if n:
            _module.launch('lp_build', _rows(n), _BLOCK, 'QqQQQQQQ',
                           K.data_ptr(), n, f.data_ptr(), y.data_ptr(),
                           a.data_ptr(), B.data_ptr(), vec.data_ptr(),
                           sums.data_ptr(), stream=current_stream(dev))
    return B, vec, sums


def build_torch(K, f, y, a, B=None, vec=None):
    import torch
    n = K.shape[0]
    pi = torch.sigmoid(f)
    w = pi * (1 - pi)
    s = torch.sqrt(w)
    g = y - pi
    b = w * f + g
    B = torch.eye(n, dtype=K.dtype, device=K.device) \
        + (s[:, None] * K) * s[None, :]
    sums = torch.stack(((a * f).sum(),
                        torch.log1p(torch.exp(-(2 * y - 1) * f)).sum()))
    return B, torch.cat((pi, s, b, g, K @ b)), sums


def solve(Binv, vec):
    """``a = b - s * (Binv (s * K b))`` (n) of `lp_solve`."""
    import torch
    n = Binv.shape[0]
    _square('Binv', Binv, n)
    dev = Binv.device
    vec = _vector('vec', vec, 5 * n, dev)
    with torch.cuda.device(dev):
        a = torch.empty(n, dtype=torch.float64, device=dev)
        if n:
            _module.launch('lp_solve', _rows(n), _BLOCK, 'QqQQ',
                           Binv.data_ptr(), n, vec.data_ptr(), a.data_ptr(),
                           stream=current_stream(dev))
    return a


def solve_torch(Binv, vec):
    n = Binv.shape[0]
    s, b, kb = vec[n:2 * n], vec[2 * n:3 * n], vec[4 * n:]
    return b - s * (Binv @ (s * kb))


def apply(K, a):
    """``f = K a`` (n) of `lp_apply`."""
    import torch
    n = K.shape[0]
    _square('K', K, n)
    dev = K.device
    a = _vector('a', a, n, dev)
    with torch.cuda.device(dev):
        f = torch.empty(n, dtype=torch.float64, device=dev)
        if n:
            _module.launch('lp_apply', _rows(n), _BLOCK, 'QqQQ',
                           K.data_ptr(), n, a.data_ptr(), f.data_ptr(),
                           stream=current_stream(dev))
    return f


def apply_torch(K, a):
    return K @ a


# -- the gradient: one contraction of the planes with M --------------------------
def _plane_list(P, planes, n, dev):
    import torch
    planes = np.asarray(planes, dtype=np.int64).ravel()
    if len(planes):
        if P is None or P.dim() != 3 or P.dtype not in (torch.float32,
                                                        torch.float64):
            raise TypeError('P: (n, n, m) float32 or float64 planes expected')
        if tuple(P.shape[:2]) != (n, n) or P.device != dev:
            raise ValueError(f'P: ({n}, {n}, m) planes on {dev} expected')
        if planes.min() < 0 or planes.max() >= P.shape[2]:
            raise IndexError('plane index out of range')
        if min(P.stride()) < 0:
            raise ValueError('P: negative strides')
    return planes


def contract(P, planes, Binv, s, a, u, g):
    """``d[k] = sum_ij M[i, j] P[i, j, planes[k]]`` with ``M = (a a^T - s
    Binv s + u g^T + g u^T) / 2`` as a float64 tensor on Binv's device
    (`lp_planes_*`, then `lp_reduce`); M is never stored.

    Binv: (n, n) float64 CUDA tensor, row-major contiguous, symmetric.  s, a,
    u, g: n float64 values on that device.  P: None or the (n, n, m)
    symmetric gradient planes in float32 or float64, any strides with
    positive values (read as they lie).  planes: indices into the m planes."""
    import torch
    n = Binv.shape[0]
    _square('Binv', Binv, n)
    dev = Binv.device
    planes = _plane_list(P, planes, n, dev)
    nt = len(planes)
    vecs = torch.cat([_vector(name, v, n, dev) for name, v in
                      (('s', s), ('a', a), ('u', u), ('g', g))])
    with torch.cuda.device(dev):
        out = torch.zeros(nt, dtype=torch.float64, device=dev)
        if n == 0 or nt == 0:
            return out
        stream = current_stream(dev)
        kc, ntiles, gz = grid(n, nt)
        nblk = ntiles * _SUB
        partial = torch.empty(nt * nblk, dtype=torch.float64, device=dev)
        pidx = torch.from_numpy(planes).to(dev)
        s_lane, s_col, s_k = plane_strides(P)
        _module.launch(
            f'lp_planes_{suffix(P.dtype)}_k{kc}', nblk * gz, _BLOCK,
            'QqqqqQiQQqQ', P.data_ptr(), n, s_lane, s_col, s_k,
            pidx.data_ptr(), nt, Binv.data_ptr(), vecs.data_ptr(), ntiles,
            partial.data_ptr(), stream=stream)
        _module.launch('lp_reduce', nt, _BLOCK, 'QqQ', partial.data_ptr(),
                       nblk, out.data_ptr(), stream=stream)
    return out


def weights_torch(Binv, s, a, u, g):
    """The weight matrix M itself (the restatement stores what the kernels
    form on the fly)."""
    import torch
    ug = torch.outer(u, g)
    return 0.5 * (torch.outer(a, a) - s[:, None] * Binv * s[None, :]
                  + ug + ug.T)


def contract_torch(P, planes, Binv, s, a, u, g):
    import torch
    planes = np.asarray(planes, dtype=np.int64).ravel()
    if not len(planes):
        return torch.zeros(0, dtype=torch.float64, device=Binv.device)
    dK = P if P.shape[2] == len(planes) and \
        np.array_equal(planes, np.arange(P.shape[2])) else \
        P.index_select(2, torch.as_tensor(planes, device=P.device))
    return _contract_planes(weights_torch(Binv, s, a, u, g),
                            dK.to(torch.float64))


# -- what stays in torch on either path ------------------------------------------
def third_order(K, Binv, vec):
    """``u = s2 - R K s2`` (n) with ``R = s Binv s`` and ``s2 = -(diag K -
    diag(K R K)) / 2 * pi (1 - pi)(1 - 2 pi)``: the one N^3 product of the
    gradient, ``Binv (s K)``, is a matrix product of the BLAS behind torch;
    R itself is not formed."""
    n = K.shape[0]
    pi, s = vec[:n], vec[n:2 * n]
    sK = s[:, None] * K
    q = (sK * (Binv @ sK)).sum(0)
    s2 = -0.5 * (K.diagonal() - q) * (pi * (1 - pi) * (1 - 2 * pi))
    return s2 - s * (Binv @ (s * (K @ s2)))
