"""What the host modules of the fused dense kernels share across the model
packages: the checks of a matrix and of a float64
buffer that a kernel reads as they lie, the strides a kernel is handed for a
symmetric matrix and for symmetric gradient planes, the grid of a pass over
the tiles on and above the diagonal, and the contraction of the planes that
the ``*_torch`` restatements share with the regressor.  A host module of a
model package imports from here, from `hip/` and from `kernel/`, never a
private name of another model package."""
from ..hip.source_module import chunk

_TILE = 64          # rows and columns per tile of a pass over the triangle


def _f64(name, t, shape, dev):
    import torch
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) \
            or t.device != dev:
        raise TypeError(f'{name}: {tuple(shape)} float64 on {dev} expected')
    return t.contiguous()


def _check_K(K):
    """n of a symmetric matrix the kernels can read as it lies."""
    import torch
    if not K.is_cuda:
        raise TypeError('K: a CUDA tensor expected; see the *_torch '
                        'restatements')
    if K.dim() != 2 or K.shape[0] != K.shape[1] \
            or K.dtype not in (torch.float32, torch.float64):
        raise TypeError('K: (n, n) float32 or float64 expected')
    n = K.shape[0]
    if n > 1 and K.stride() not in ((n, 1), (1, n)):
        raise ValueError('K must be contiguous along one of its indices')
    if K.data_ptr() % 16:
        raise ValueError('K must be 16-byte aligned')
    return n


def matrix_strides(K):
    """(k_lane, k_col) in elements: the lane axis is the one with the smaller
    stride (the matrix is symmetric)."""
    s0, s1 = K.stride()
    if K.shape[0] <= 1:
        s0 = s1 = 0
    return (s0, s1) if s0 <= s1 else (s1, s0)


def plane_strides(P):
    """(s_lane, s_col, s_k) in elements: the lane axis is whichever of the
    first two has the smaller stride (the planes are symmetric in them)."""
    s0, s1, s2 = P.stride()
    n = P.shape[0]
    if n <= 1:
        s0 = s1 = 0
    if P.shape[2] <= 1:
        s2 = 0
    return (s0, s1, s2) if s0 <= s1 else (s1, s0, s2)


def triangle_grid(n, nt):
    """(chunk size KC, tiles on and above the diagonal, chunks) of a pass
    over `nt` planes of an (n, n) symmetric matrix (`lp_planes`, `od_planes`,
    `ka_planes`).  A function of the shapes alone, so that the order of every
    sum is the same on every call."""
    kc = chunk(nt)
    nb = -(-n // _TILE)
    return kc, nb * (nb + 1) // 2, max(1, -(-nt // kc))


def _contract_planes(W, dK):
    """``sum_ij W[i, j] dK[i, j, k]`` for a *symmetric* W.  The kernel hands
    its gradient over plane by plane (element (i, j, k) at i + n j + n^2 k,
    reference _kernel.py:249-256): then the contraction is one matrix-vector
    product over contiguous rows, 0.03 ms for n = 1000 and six planes on an
    MI355X against 0.34 ms for multiply + reduce over the broadcast product
    (scripts/time_gpr_dense.py).  Any other layout: multiply + reduce (the
    einsum / GEMV form on a hyperparameter-fastest layout took 107 ms on
    rocBLAS)."""
    n0, n1, nt = dK.shape
    planes = dK.permute(2, 1, 0)                # [k][j][i]: W_ji = W_ij
    if planes.is_contiguous():
        return planes.reshape(nt, n0 * n1) @ W.reshape(n0 * n1)
    if dK.permute(2, 0, 1).is_contiguous():     # [k][i][j]
        return dK.permute(2, 0, 1).reshape(nt, n0 * n1) @ \
            W.contiguous().reshape(n0 * n1)
    return (W.unsqueeze(-1) * dK).sum((0, 1))
