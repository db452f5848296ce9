"""Host side of csrc/device/knn.h, the row-wise selection of the k nearest
neighbours over a kernel matrix where it lies and the sums the neighbour
models make of the lists: compiles the kernels once
(`TEXT_UNITS['knn']`; JIT cache of graphdot_amd.hip.jit, IEEE arithmetic: no
fast-math) and runs them on torch's *current* stream of the matrix's device,
in stream order with the torch operations around them.  No host
synchronisation between the launches of a call; the workspace of a split
search is ``(b, parts, k)`` entries from torch's allocator, and nothing of
size b x n is written.  The ``*_torch`` functions are the same chain through
torch on any device: the restatement the kernels are compared with, and the
path of CPU tensors, of k above `K_MOST` and of matrices the launches
decline.

With the self-similarities dq (b,) and dt (n,) the squared feature-space
distance is ``d2 = max(0, (dq[i] + dt[j]) - 2 K[i, j])``, and the neighbours
of a row are its k smallest candidates in the total order (d2, j): ties go to
the smaller column."""
from ...hip.source_module import TEXT_UNITS, current_stream, suffix

_module = TEXT_UNITS['knn']
precompile = _module.precompile
_BLOCK = 256
_WAVES = 4          # rows per workgroup of knn_merge
_ROWS = 32          # rows per strip of knn_topk
_TILE = 64          # columns per tile of knn_topk
#: most neighbours of the fused search: one list entry per lane
K_MOST = 64
#: most parts the columns are split into (knn_merge walks parts x k entries
#: per row with one wave)
PARTS_MOST = 64
#: the workgroups a search should have before its columns are split no further
#: (measured: scripts/time_neighbors.py --parts)
_WORKGROUPS = 512
WEIGHTS = ('uniform', 'distance')
#: the largest column the kernels' int entries hold
_N_MOST = 2 ** 31 - 1 - _TILE


def parts_for(b, n, parts=None):
    """Into how many parts `knn_topk_*` splits the columns of a (b, n)
    search: enough for `_WORKGROUPS` workgroups, one part per tile of 64
    columns and `PARTS_MOST` at the most -- or `parts` where one is given
    (the same lists with every one).  A function of the shape alone."""
    if parts is not None:
        if int(parts) != parts or not 1 <= parts <= PARTS_MOST:
            raise ValueError(f'parts: an integer from 1 to {PARTS_MOST} '
                             f'expected, got {parts}')
        return int(parts)
    strips = -(-b // _ROWS)
    tiles = -(-n // _TILE)
    return max(1, min(-(-_WORKGROUPS // max(strips, 1)), tiles, PARTS_MOST))


def _check(Ks, dq, dt, k, exclude_self):
    """(b, n) of checked arguments, any device."""
    import torch
    if not torch.is_tensor(Ks) or Ks.dim() != 2 \
            or Ks.dtype not in (torch.float32, torch.float64):
        raise TypeError('Ks: a (b, n) float32 or float64 tensor expected')
    b, n = Ks.shape
    for name, d, m in (('dq', dq, b), ('dt', dt, n)):
        if not torch.is_tensor(d) or d.dtype != torch.float64 \
                or tuple(d.shape) != (m,):
            raise TypeError(f'{name}: ({m},) float64 expected')
    if min(Ks.stride()) < 0:
        raise ValueError('Ks: negative strides')
    if exclude_self and b != n:
        raise ValueError('exclude_self: a square matrix expected, got '
                         f'{(b, n)}')
    most = n - 1 if exclude_self else n
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f'n_neighbors: a positive integer expected, got {k}')
    if k > most:
        raise ValueError(f'n_neighbors = {k} exceeds the {most} candidates')
    return b, n


def _lists(d2, idx, k, mode=None):
    import torch
    if d2.dtype != torch.float64 or idx.dtype != torch.int64 \
            or d2.dim() != 2 or d2.shape != idx.shape or d2.shape[1] < 1 \
            or d2.device != idx.device:
        raise TypeError('lists: (b, k) float64 squared distances and int64 '
                        'indices on one device expected')
    if mode is not None and mode not in WEIGHTS:
        raise ValueError(f'weights: one of {WEIGHTS} expected, got {mode!r}')
    return d2.contiguous(), idx.contiguous(), d2.shape[0], d2.shape[1]


def _table(name, t, n, dev, columns=False):
    import torch
    if not torch.is_tensor(t) or t.dtype != torch.float64 \
            or t.dim() != 1 + columns or (n is not None and t.shape[0] != n):
        raise TypeError(f'{name}: float64 with {n} rows expected')
    return t.to(dev).contiguous()


# -- the search ------------------------------------------------------------------------
def topk(Ks, dq, dt, k, exclude_self=False, parts=None):
    """``(d2 (b, k) float64, idx (b, k) int64, flag (1,) int32)`` on Ks's
    device, enqueued on torch's current stream (`knn_topk_*`, and `knn_merge`
    where the columns are split): per row the k smallest (d2, column) in
    ascending order; `flag` is not zero if some d2 is not finite before its
    clamp (the lists are meaningless then).  The lists of a row depend on
    that row's data alone.

    Ks: (b, n) float32 or float64 CUDA tensor, any strides without negative
    values (read as it lies).  dq (b,), dt (n,): float64, any device.
    ``k <= K_MOST``.  exclude_self: column i is no candidate of row i.
    parts: the split of the columns in the place of `parts_for`'s choice."""
    import torch
    b, n = _check(Ks, dq, dt, k, exclude_self)
    if not Ks.is_cuda:
        raise TypeError('Ks: a CUDA tensor expected; see topk_torch')
    if k > K_MOST:
        raise ValueError(f'n_neighbors = {k}: {K_MOST} at the most; see '
                         'topk_torch')
    if n > _N_MOST:
        raise ValueError(f'Ks: {_N_MOST} columns at the most')
    dev = Ks.device
    k = int(k)
    parts = parts_for(b, n, parts)
    dq, dt = dq.to(dev).contiguous(), dt.to(dev).contiguous()
    with torch.cuda.device(dev):
        d2 = torch.empty((b, k), dtype=torch.float64, device=dev)
        idx = torch.empty((b, k), dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if b == 0:
            return d2, idx, flag
        stream = current_stream(dev)
        if parts == 1:
            w2, widx = d2, idx
        else:
            w2 = torch.empty((b, parts, k), dtype=torch.float64, device=dev)
            widx = torch.empty((b, parts, k), dtype=torch.int64, device=dev)
        s_row, s_col = Ks.stride()
        _module.launch(f'knn_topk_{suffix(Ks.dtype)}', -(-b // _ROWS) * parts,
                       _BLOCK, 'QqqqqQQiiqQQQ', Ks.data_ptr(), b, n, s_row,
                       s_col, dq.data_ptr(), dt.data_ptr(), k,
                       int(bool(exclude_self)), parts, w2.data_ptr(),
                       widx.data_ptr(), flag.data_ptr(), stream=stream)
        if parts > 1:
            _module.launch('knn_merge', -(-b // _WAVES), _BLOCK, 'QQqqiQQ',
                           w2.data_ptr(), widx.data_ptr(), b, parts, k,
                           d2.data_ptr(), idx.data_ptr(), stream=stream)
    return d2, idx, flag


def topk_torch(Ks, dq, dt, k, exclude_self=False):
    """The same three tensors by torch on any device (the restatement writes
    the (b, n) matrix of d2 in double and sorts it: a stable sort, so that
    equal d2 stay in the order of their columns)."""
    import torch
    b, n = _check(Ks, dq, dt, k, exclude_self)
    dev = Ks.device
    dq, dt = dq.to(dev), dt.to(dev)
    d2 = (dq[:, None] + dt[None, :]) - 2.0 * Ks.to(torch.float64)
    if exclude_self:
        d2.diagonal().fill_(0.0)
    # (before the clamp, which would turn -inf into 0)
    flag = (~torch.isfinite(d2)).any().to(torch.int32).reshape(1)
    d2 = torch.where(d2 < 0.0, torch.zeros_like(d2), d2)
    if exclude_self:
        d2.diagonal().fill_(float('inf'))
    val, idx = torch.sort(d2, dim=1, stable=True)
    return val[:, :k].contiguous(), idx[:, :k].contiguous(), flag


def _declines(Ks, k):
    """Why the fused search is not for this call (None: it is)."""
    if not Ks.is_cuda:
        return 'not a CUDA tensor'
    if k > K_MOST:
        return f'more than {K_MOST} neighbours'
    if Ks.shape[1] > _N_MOST:
        return 'too many columns'
    return None


def search(Ks, dq, dt, k, exclude_self=False):
    """(``(d2, idx, flag)``, fused?): `topk` where it applies, `topk_torch`
    anywhere else."""
    if _declines(Ks, k) is None:
        return topk(Ks, dq, dt, k, exclude_self), True
    return topk_torch(Ks, dq, dt, k, exclude_self), False


# -- weighted means --------------------------------------------------------------------
def average(d2, idx, T, weights='uniform'):
    """``(b, m)`` weighted means of the rows ``T[idx[i, r]]`` of the (n, m)
    float64 table `T` (`knn_average`): weight 1 ('uniform') or 1 / d
    ('distance'; where neighbours of a row are at d == 0, 1 for those and 0
    for the rest), summed in rank order."""
    import torch
    d2, idx, b, k = _lists(d2, idx, None, weights)
    if not d2.is_cuda:
        raise TypeError('lists: CUDA tensors expected; see average_torch')
    dev = d2.device
    T = _table('T', T, None, dev, columns=True)
    n, m = T.shape
    with torch.cuda.device(dev):
        out = torch.empty((b, m), dtype=torch.float64, device=dev)
        if b * m:
            _module.launch('knn_average', -(-b * m // _BLOCK), _BLOCK,
                           'QQqiQqqiQ', d2.data_ptr(), idx.data_ptr(), b, k,
                           T.data_ptr(), n, m, WEIGHTS.index(weights),
                           out.data_ptr(), stream=current_stream(dev))
    return out


def weights_torch(d2, weights):
    """(b, k) weights of the lists, as `knn_average` takes them."""
    import torch
    if weights == 'uniform':
        return torch.ones_like(d2)
    d = torch.sqrt(d2)
    zero = d == 0.0
    return torch.where(zero.any(1, keepdim=True), zero.to(d2.dtype), 1.0 / d)


def average_torch(d2, idx, T, weights='uniform'):
    d2, idx, b, k = _lists(d2, idx, None, weights)
    T = _table('T', T, None, d2.device, columns=True)
    w = weights_torch(d2, weights)
    return (w[:, :, None] * T[idx]).sum(1) / w.sum(1, keepdim=True)


def mean(d2, idx, T, weights='uniform'):
    """(means, fused?)"""
    if d2.is_cuda:
        return average(d2, idx, T, weights), True
    return average_torch(d2, idx, T, weights), False


# -- local outlier factor ----------------------------------------------------------------
def lrd(d2, idx, kdist):
    """(b,) local reachability densities ``1 / (mean_r max(kdist[idx[i, r]],
    d[i, r]) + 1e-10)`` (`knn_lrd`); `kdist` (n,): the candidates' own k-th
    distances."""
    import torch
    d2, idx, b, k = _lists(d2, idx, None)
    if not d2.is_cuda:
        raise TypeError('lists: CUDA tensors expected; see lrd_torch')
    dev = d2.device
    kdist = _table('kdist', kdist, None, dev)
    with torch.cuda.device(dev):
        out = torch.empty(b, dtype=torch.float64, device=dev)
        if b:
            _module.launch('knn_lrd', -(-b // _BLOCK), _BLOCK, 'QQqiQqQ',
                           d2.data_ptr(), idx.data_ptr(), b, k,
                           kdist.data_ptr(), kdist.shape[0], out.data_ptr(),
                           stream=current_stream(dev))
    return out


def lrd_torch(d2, idx, kdist):
    import torch
    d2, idx, b, k = _lists(d2, idx, None)
    kdist = _table('kdist', kdist, None, d2.device)
    reach = torch.maximum(kdist[idx], torch.sqrt(d2))
    return 1.0 / (reach.sum(1) / k + 1e-10)


def ratio(idx, lrd_train, lrd_rows):
    """(b,) local outlier factors ``mean_r (lrd_train[idx[i, r]] /
    lrd_rows[i])`` (`knn_ratio`)."""
    import torch
    if not idx.is_cuda:
        raise TypeError('idx: a CUDA tensor expected; see ratio_torch')
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[1] < 1:
        raise TypeError('idx: (b, k) int64 expected')
    dev = idx.device
    idx = idx.contiguous()
    b, k = idx.shape
    lrd_train = _table('lrd_train', lrd_train, None, dev)
    lrd_rows = _table('lrd_rows', lrd_rows, b, dev)
    with torch.cuda.device(dev):
        out = torch.empty(b, dtype=torch.float64, device=dev)
        if b:
            _module.launch('knn_ratio', -(-b // _BLOCK), _BLOCK, 'QqiQqQQ',
                           idx.data_ptr(), b, k, lrd_train.data_ptr(),
                           lrd_train.shape[0], lrd_rows.data_ptr(),
                           out.data_ptr(), stream=current_stream(dev))
    return out


def ratio_torch(idx, lrd_train, lrd_rows):
    lrd_train = _table('lrd_train', lrd_train, None, idx.device)
    lrd_rows = _table('lrd_rows', lrd_rows, idx.shape[0], idx.device)
    return (lrd_train[idx] / lrd_rows[:, None]).sum(1) / idx.shape[1]


def factors(d2, idx, kdist, lrd_train=None):
    """(``(lof, lrd)`` of the rows, fused?): the local outlier factors of the
    rows whose lists are given, against the candidates' `kdist` and
    `lrd_train` -- or, with ``lrd_train=None``, of the candidates themselves
    (the lists of the `exclude_self` search: their own densities are the
    candidates')."""
    if d2.is_cuda:
        own = lrd(d2, idx, kdist)
        return (ratio(idx, own if lrd_train is None else lrd_train, own),
                own), True
    own = lrd_torch(d2, idx, kdist)
    return (ratio_torch(idx, own if lrd_train is None else lrd_train, own),
            own), False
