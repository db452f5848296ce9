"""Host side of posterior.hip, the fused predictive mean and standard
deviation of a Gaussian process for a handful of candidates: compiles the
kernels once (JIT cache of graphdot_amd.hip.jit, IEEE arithmetic: no
fast-math) and runs them on torch's *current* stream of the inverse's device,
in stream order with the torch operations around them.  Two launches per call
(the rows of the inverse, the fixed-order reduction with the epilogue) and no
host synchronisation."""
from ...hip.source_module import (STATIC, CHUNKS as _CHUNKS, chunk,
                                   current_stream, suffix)

_module = STATIC['posterior.hip']
precompile = _module.precompile
_BLOCK = 256
_WAVES = 4          # rows of the inverse per workgroup of gp_rows (one per wave)


def source():
    return _module.source


def grid(n, b):
    """(chunk size KC, row blocks, chunks): gp_rows runs row blocks x chunks
    workgroups.  A function of the shapes alone, so that the order of every
    sum is the same on every call."""
    kc = chunk(b)
    return kc, -(-n // _WAVES), max(1, -(-b // kc))


def column_major(Ks):
    """`Ks` (b, n) with element (c, j) at c + j b, as the solver leaves its
    cross matrices: adopted as it lies, any other layout is copied."""
    b, n = Ks.shape
    if (b <= 1 or Ks.stride(0) == 1) and (n <= 1 or Ks.stride(1) == b):
        return Ks
    return Ks.t().contiguous().t()


def _check(Kinv, Ks, Ky, kss):
    import torch
    n = Kinv.shape[0]
    if Kinv.dtype != torch.float64 or tuple(Kinv.shape) != (n, n):
        raise TypeError('Kinv: (n, n) float64 expected')
    if Ks.dim() != 2 or Ks.shape[1] != n or Ks.dtype not in (torch.float32,
                                                             torch.float64):
        raise TypeError(f'Ks: (b, {n}) float32 or float64 expected')
    b = Ks.shape[0]
    if Ky.dtype != torch.float64 or tuple(Ky.shape) != (n,):
        raise TypeError(f'Ky: {n} float64 values expected')
    if kss.dtype != torch.float64 or tuple(kss.shape) != (b,):
        raise TypeError(f'kss: {b} float64 values expected')
    for name, t in (('Ks', Ks), ('Ky', Ky), ('kss', kss)):
        if t.device != Kinv.device:
            raise ValueError(f'Kinv and {name} must be on the same device')
    return n, b


def posterior(Kinv, Ks, Ky, kss, ymean=0.0, ystd=1.0, return_T=False):
    """``(out, T)``: ``out = [mean (b) | std (b)]`` as one float64 tensor on
    Kinv's device and ``T = Kinv Ks^T`` (n, b) or None, enqueued on torch's
    current stream, with ``mean = ystd Ks Ky + ymean`` and ``std = ystd
    sqrt(max(0, kss - diag(Ks Kinv Ks^T)))``.

    Kinv: (n, n) float64 CUDA tensor, row-major contiguous.  Ks: (b, n)
    float32 or float64, column-major (`column_major`).  Ky: (n,), kss: (b,)
    float64, contiguous."""
    import torch
    if not Kinv.is_cuda:
        raise TypeError('posterior runs on CUDA tensors; see posterior_torch')
    n, b = _check(Kinv, Ks, Ky, kss)
    if n > 1 and Kinv.stride() != (n, 1):
        raise ValueError('Kinv must be row-major contiguous')
    if Kinv.data_ptr() % 16:
        raise ValueError('Kinv must be 16-byte aligned')
    Ks = column_major(Ks)
    Ky, kss = Ky.contiguous(), kss.contiguous()
    dev = Kinv.device
    with torch.cuda.device(dev):
        out = torch.empty(2 * b, dtype=torch.float64, device=dev)
        T = torch.empty((n, b), dtype=torch.float64, device=dev) \
            if return_T else None
        if b == 0:
            return out, T
        if n == 0:
            out[:b] = float(ymean)
            out[b:] = float(ystd) * torch.sqrt(torch.clamp(kss, min=0))
            return out, T
        stream = current_stream(dev)
        kc, nblk, gz = grid(n, b)
        partial = torch.empty(2 * b * nblk, dtype=torch.float64, device=dev)
        _module.launch(
            f'gp_rows_{suffix(Ks.dtype)}_k{kc}', nblk * gz, _BLOCK,
            'QQQqiqQQ', Kinv.data_ptr(), Ks.data_ptr(), Ky.data_ptr(), n, b,
            nblk, partial.data_ptr(), T.data_ptr() if return_T else 0,
            stream=stream)
        _module.launch('gp_finish', b, _BLOCK, 'QqiQddQ', partial.data_ptr(),
                       nblk, b, kss.data_ptr(), float(ymean), float(ystd),
                       out.data_ptr(), stream=stream)
    return out, T


def posterior_torch(Kinv, Ks, Ky, kss, ymean=0.0, ystd=1.0, return_T=False):
    """The same by torch on any device: the yardstick of the kernels and the
    CPU path of `DevicePosterior`."""
    import torch
    _check(Kinv, Ks, Ky, kss)
    Ks = Ks.to(torch.float64)
    T = Kinv @ Ks.T
    q = (Ks.T * T).sum(0)
    mean = float(ystd) * (Ks @ Ky) + float(ymean)
    std = float(ystd) * torch.sqrt(torch.clamp(kss - q, min=0))
    return torch.cat((mean, std)), (T if return_T else None)
