"""Host side of field.hip, the fused weight-matrix kernels of the Gaussian
field regressor: compiles them once (JIT cache of graphdot_amd.hip.jit, IEEE
arithmetic: no fast-math) and runs them on torch's *current* stream of the
block's device, in stream order with the torch operations around them.  Two
launches per call (the pass over the block, the fixed-order reduction of its
per-workgroup sums) and no host synchronisation."""
import os
import struct
import threading
import numpy as np

_SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       'field.hip')
_FLAGS = ('-fno-fast-math',)
_BLOCK = 256
_ROWS = 64           # rows per workgroup (one per lane)
_WAVES = 4           # columns per workgroup and step (one per wave)
_CHUNKS = (1, 2, 4, 8, 16)     # planes per register chunk (template KC)
_TARGET_BLOCKS = 2048          # workgroups to aim for (256 CUs x 8)
#: the kernel-induced distance's constants (KernelInducedDistance)
HALF = 0.4999997
EPS = 1e-4
_lock = threading.Lock()
_kernels = None


def source():
    with open(_SOURCE) as f:
        return f.read()


def precompile():
    """Compile into the JIT cache (hipcc, no device needed)."""
    from ...hip import jit
    return jit.compile_source(source(), _FLAGS)


def _load():
    global _kernels
    with _lock:
        if _kernels is None:
            from ...hip import jit, runtime
            mod = runtime.Module(jit.load_image(precompile()))
            names = [f'gf_rowsums_{t}' for t in ('f32', 'f64')]
            names += [f'gf_contract_{a}_{b}_k{kc}' for a in ('f32', 'f64')
                      for b in ('f32', 'f64') for kc in _CHUNKS]
            names += ['gf_rowsums_reduce', 'gf_reduce']
            _kernels = {name: mod.function(name) for name in names}
            _kernels['module'] = mod
    return _kernels


def grid(Nr, Nc, n):
    """(chunk size KC, row tiles gx, column sets gy, chunks gz): a function
    of the shapes alone, so that the order of every sum is the same on every
    call.  (`n` = 0: gf_rowsums, one chunk.)"""
    kc = next(k for k in _CHUNKS if k >= min(max(n, 1), _CHUNKS[-1]))
    gz = max(1, -(-n // kc))
    gx = -(-Nr // _ROWS)
    gy = max(1, min(-(-Nc // _WAVES), -(-_TARGET_BLOCKS // (gx * gz))))
    return kc, gx, gy, gz


def _sfx(t):
    import torch
    if t.dtype == torch.float32:
        return 'f32'
    if t.dtype == torch.float64:
        return 'f64'
    raise TypeError(f'float32 or float64 expected, got {t.dtype}')


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
    _sfx(K)
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
    from ...hip import runtime
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
        stream = torch.cuda.current_stream().cuda_stream or None
        _, gx, gy, _ = grid(Nr, Nc, 0)
        ps = torch.empty(gy * Nr, dtype=torch.float64, device=dev)
        pt = torch.empty(gy * Nr, dtype=torch.float64, device=dev)
        fn = _load()
        runtime.launch(
            fn[f'gf_rowsums_{_sfx(K)}'], gx * gy, _BLOCK,
            struct.pack('@QqqqqQQdddiQQiiQQ', K.data_ptr(), K.stride(0),
                        K.stride(1), Nr, Nc, kr.data_ptr(), kc.data_ptr(),
                        half, float(sigma)**-2, float(smoothing),
                        int(bool(self_block)), _ptr(y), _ptr(W), gx, gy,
                        ps.data_ptr(), pt.data_ptr()),
            stream=stream)
        runtime.launch(
            fn['gf_rowsums_reduce'], -(-Nr // _BLOCK), _BLOCK,
            struct.pack('@QQqiQQ', ps.data_ptr(), pt.data_ptr(), Nr, gy,
                        s.data_ptr(), t.data_ptr()),
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
    from ...hip import runtime
    Nr, Nc, kr, kc = _check_block(K, kr, kc)
    dev = K.device
    planes = np.asarray(planes, dtype=np.int64).ravel()
    n = len(planes)
    if P.dim() != 3 or tuple(P.shape[:2]) != (Nr, Nc):
        raise ValueError(f'P: shape ({Nr}, {Nc}, n_planes) expected, '
                         f'got {tuple(P.shape)}')
    if P.device != dev:
        raise ValueError('P and K on different devices')
    _sfx(P)
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
        stream = torch.cuda.current_stream().cuda_stream or None
        kc_, gx, gy, gz = grid(Nr, Nc, n)
        nblk = gx * gy
        partial = torch.empty((n + 1) * nblk, dtype=torch.float64,
                              device=dev)
        fn = _load()
        sigma = float(sigma)
        runtime.launch(
            fn[f'gf_contract_{_sfx(K)}_{_sfx(P)}_k{kc_}'], gx * gy * gz,
            _BLOCK,
            struct.pack('@QqqqqQQQQddddiQQQQqqqQiQQQQiiQ',
                        K.data_ptr(), K.stride(0), K.stride(1), Nr, Nc,
                        kr.data_ptr(), kc.data_ptr(), _ptr(dkr), _ptr(dkc),
                        half, sigma**-2, sigma**-3, float(eps),
                        int(bool(self_block)), alpha.data_ptr(),
                        beta.data_ptr(), gamma.data_ptr(), P.data_ptr(),
                        P.stride(0), P.stride(1), P.stride(2), pk.data_ptr(),
                        n, _ptr(row), _ptr(col), _ptr(u), _ptr(v), gx, gy,
                        partial.data_ptr()),
            stream=stream)
        runtime.launch(fn['gf_reduce'], n + 1, _BLOCK,
                       struct.pack('@QqQ', partial.data_ptr(), nblk,
                                   out.data_ptr()),
                       stream=stream)
        # (the workspaces are freed into torch's cache on this stream: the
        # allocator hands them out again only behind these launches)
    return out
