"""Host side of lowrank.hip, the gradient contraction of the Nystrom
regressor: compiles the kernels once (JIT cache of graphdot_amd.hip.jit, IEEE
arithmetic: no fast-math) and runs them on torch's *current* stream of the
planes' device, in stream order with the torch operations around them.  Two
launches per call (the pass over the planes, the fixed-order reduction of
its per-workgroup sums) and no host synchronisation."""
import numpy as np
from ...hip.source_module import STATIC, chunk, current_stream, suffix

_module = STATIC['lowrank.hip']
_BLOCK = 256
_ROWS = 64           # rows per workgroup (one per lane)
_WAVES = 4           # columns per workgroup and step (one per wave)
_TARGET_BLOCKS = 2048          # workgroups to aim for (256 CUs x 8)


def grid(Nr, M, nt):
    """(chunk size KC, row tiles gx, column sets gy, chunks gz; the launch
    has gx gy gz workgroups): a function of the shapes alone, so that the
    order of every sum is the same on every call."""
    kc = chunk(nt)
    gz = -(-nt // kc)
    gx = -(-Nr // _ROWS)
    gy = max(1, min(-(-M // _WAVES), -(-_TARGET_BLOCKS // (gx * gz))))
    return kc, gx, gy, gz


def _check_planes(P):
    import torch
    if P.dim() != 3 or P.dtype not in (torch.float32, torch.float64):
        raise TypeError('P: (N, M, n) float32 or float64 planes expected')
    N, M, nt = P.shape
    if P.numel() > 0 and P.stride() != (1, N, N * M) and not (
            # (strides of unit dimensions do not matter)
            all(s == e or n == 1 for s, e, n in zip(
                P.stride(), (1, N, N * M), P.shape))):
        raise ValueError('P must be column-major planes: element (i, c, k) '
                         'at i + N c + N M k')


def contract(P, W, rows=None):
    """``out[k] = sum_{r, c} W[r, c] P[rows[r], c, k]`` on the GPU.

    P: (N, M, n) float32 or float64 CUDA tensor, column-major (the kernel's
    gradient planes as `device_cross_gram` hands them over); read in its own
    type.  W: (Nr, M) float64 (any layout; made column-major).  rows: None
    (Nr == N) or Nr indices into the rows of P (host array; checked against
    N here).  Returns a float64 tensor of n sums on P's device, enqueued on
    torch's current stream."""
    import torch
    _check_planes(P)
    N, M, nt = P.shape
    dev = P.device
    if rows is None:
        Nr = N
        rows_t = None
    else:
        rows = np.asarray(rows, dtype=np.int64).ravel()
        if len(rows) and (rows.min() < 0 or rows.max() >= N):
            raise IndexError('row index out of range')
        Nr = len(rows)
    if tuple(W.shape) != (Nr, M):
        raise ValueError(f'W: shape {(Nr, M)} expected, got {tuple(W.shape)}')
    if not P.is_cuda:
        raise TypeError('contract runs on CUDA tensors; see contract_torch')
    W = W.to(device=dev, dtype=torch.float64)
    if not (W.stride(0) == 1 and (M <= 1 or W.stride(1) >= max(Nr, 1))):
        W = W.t().contiguous().t()
    ldw = W.stride(1) if M > 1 else max(Nr, 1)
    with torch.cuda.device(dev):
        out = torch.zeros(nt, dtype=torch.float64, device=dev)
        if Nr == 0 or M == 0 or nt == 0:
            return out
        if rows is not None:
            rows_t = torch.from_numpy(rows).to(dev, non_blocking=False)
        stream = current_stream(dev)
        kc, gx, gy, gz = grid(Nr, M, nt)
        nblk = gx * gy
        partial = torch.empty(nt * nblk, dtype=torch.float64, device=dev)
        _module.launch(
            f'lr_contract_{suffix(P.dtype)}_k{kc}', gx * gy * gz, _BLOCK,
            'QqqiQqQqiiQ', P.data_ptr(), N, M, nt, W.data_ptr(), ldw,
            rows_t.data_ptr() if rows_t is not None else 0, Nr, gx, gy,
            partial.data_ptr(), stream=stream)
        _module.launch('lr_reduce', nt, _BLOCK, 'QqQ', partial.data_ptr(),
                       nblk, out.data_ptr(), stream=stream)
    return out


def contract_torch(P, W, rows=None):
    """The same sums by torch: the planes converted to float64, then one
    matrix-vector product (the `_contract_planes` route of gpr.py).  The
    CPU path of the regressor and the yardstick of the kernel."""
    import torch
    N, M, nt = P.shape
    if rows is not None:
        idx = torch.as_tensor(np.asarray(rows, dtype=np.int64),
                              device=P.device)
        P = P.index_select(0, idx)
    n0 = P.shape[0]
    W = W.to(device=P.device, dtype=torch.float64)
    planes = P.permute(2, 1, 0)
    if planes.is_contiguous():
        return planes.reshape(nt, n0 * M).to(torch.float64) @ \
            W.t().contiguous().reshape(n0 * M)
    return (W.unsqueeze(-1) * P.to(torch.float64)).sum((0, 1))
