"""Host side of mst.h, the minimum spanning tree of the mutual-reachability
graph of a kernel matrix where it lies: compiles the
kernels once (`MODEL_UNITS['mst']`; JIT cache of graphdot_amd.hip.jit, IEEE
arithmetic: no fast-math) and runs them on torch's *current* stream of the
matrix's device as plain launches, in stream order with the torch operations
around them.  The host loop runs Boruvka rounds on the implicit graph: nothing
of size n x n is written, and one download per round (the number of
components and the flag word) decides whether another round follows.  The
``*_torch`` functions are the same chain through torch on any device: the
restatement the kernels are compared with, and the path of CPU tensors and of
matrices the launches decline.

With the self-similarities diag (n,) and the squared core distances c2 (n,),
``d2(i, j) = max(0, (diag[i] + diag[j]) - 2 K[i, j])``, ``s(i, j) = min(d2(i,
j), d2(j, i))`` and ``w2(i, j) = max(c2[i], c2[j], s(i, j))``.  Edges are
compared in the strict total order ``(w2, min(i, j), max(i, j))``; the tree
that is minimal in it is unique, so every correct chain gives the same edges
bit for bit.  There is no square root here."""
import numpy as np
from ...hip.source_module import MODEL_UNITS, current_stream, suffix

_module = MODEL_UNITS['mst']
precompile = _module.precompile
_BLOCK = 256
_ROWS = 32          # rows per strip of mst_rows
_TILE = 64          # columns per tile of mst_rows
#: the steps of one `mst_jump`
JUMP = 8
#: most parts the columns are split into
PARTS_MOST = 64
#: the workgroups a row pass should have before its columns are split no
#: further: the choice of the neighbour search, whose strips and tiles these
#: are
_WORKGROUPS = 512
#: the largest n: labels, candidates and edge ends are ints
_N_MOST = 2 ** 31 - 1 - _TILE
ENTRY_POINTS = ('mst_rows_f32', 'mst_rows_f64', 'mst_combine', 'mst_best_w',
                'mst_best_e', 'mst_hook', 'mst_jump', 'mst_relabel')
__all__ = ['ENTRY_POINTS', 'JUMP', 'PARTS_MOST', 'parts_for', 'rounds_most',
           'jumps_for', 'rows', 'rows_torch', 'cross_rows', 'cross_rows_torch',
           'new_edges', 'hook', 'hook_torch', 'spanning_tree', 'sort_edges']


def parts_for(b, n, parts=None):
    """Into how many parts `mst_rows_*` splits the columns of a (b, n) pass:
    enough for `_WORKGROUPS` workgroups, one part per tile of 64 columns and
    `PARTS_MOST` at the most -- or `parts` where one is given (the same
    candidates with every one).  A function of the shape alone."""
    if parts is not None:
        if int(parts) != parts or not 1 <= parts <= PARTS_MOST:
            raise ValueError(f'parts: an integer from 1 to {PARTS_MOST} '
                             f'expected, got {parts}')
        return int(parts)
    strips = -(-b // _ROWS)
    tiles = -(-n // _TILE)
    return max(1, min(-(-_WORKGROUPS // max(strips, 1)), tiles, PARTS_MOST))


def rounds_most(n):
    """``ceil(log2 n)``: a round at least halves the components."""
    return max(1, (int(n) - 1).bit_length())


def jumps_for(components):
    """The `mst_jump` launches that flatten a forest of `components` roots:
    its paths have fewer than `components` steps."""
    t, reach = 0, 1
    while reach < components:
        reach *= JUMP
        t += 1
    return t


# -- the argument checks ---------------------------------------------------------------
def _matrix(K, square):
    import torch
    if not torch.is_tensor(K) or K.dim() != 2 \
            or K.dtype not in (torch.float32, torch.float64) \
            or (square and K.shape[0] != K.shape[1]):
        raise TypeError('K: a%s float32 or float64 matrix expected'
                        % (' square' if square else ''))
    if min(K.stride()) < 0:
        raise ValueError('K: negative strides')
    return K.shape


def _vector(name, v, m, dev, dtype):
    import torch
    if not torch.is_tensor(v) or v.dtype != dtype or tuple(v.shape) != (m,) \
            or v.device != dev:
        raise TypeError(f'{name}: ({m},) {dtype} on {dev} expected')
    return v.contiguous()


def _check_rows(K, diag, c2, comp):
    import torch
    n, _ = _matrix(K, True)
    dev = K.device
    return (n, _vector('diag', diag, n, dev, torch.float64),
            _vector('c2', c2, n, dev, torch.float64),
            _vector('comp', comp, n, dev, torch.int32))


def _check_cross(Ks, dq, dt, cq, ct):
    import torch
    b, n = _matrix(Ks, False)
    dev, f64 = Ks.device, torch.float64
    return (b, n, _vector('dq', dq, b, dev, f64), _vector('dt', dt, n, dev, f64),
            _vector('cq', cq, b, dev, f64), _vector('ct', ct, n, dev, f64))


def _cuda(K):
    if not K.is_cuda:
        raise TypeError('a CUDA tensor expected; see the *_torch '
                        'restatements')
    if max(K.shape) > _N_MOST:
        raise ValueError(f'{_N_MOST} rows and columns at the most')


def _declines(K):
    """Why the fused chain is not for this matrix (None: it is)."""
    if not K.is_cuda:
        return 'not a CUDA tensor'
    if max(K.shape) > _N_MOST:
        return 'too many samples'
    return None


# -- the row pass ----------------------------------------------------------------------
def _rows(K, b, n, dq, dt, cq, ct, comp, parts, flag):
    import torch
    _cuda(K)
    dev = K.device
    parts = parts_for(b, n, parts)
    with torch.cuda.device(dev):
        w2 = torch.empty(b, dtype=torch.float64, device=dev)
        cand = torch.empty(b, dtype=torch.int32, device=dev)
        if flag is None:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if b == 0:
            return w2, cand, flag
        stream = current_stream(dev)
        if parts == 1:
            ws_w2, ws_j = w2, cand
        else:
            ws_w2 = torch.empty((b, parts), dtype=torch.float64, device=dev)
            ws_j = torch.empty((b, parts), dtype=torch.int32, device=dev)
        s_row, s_col = K.stride()
        _module.launch(f'mst_rows_{suffix(K.dtype)}', -(-b // _ROWS) * parts,
                       _BLOCK, 'QqqqqQQQQQqQQQ', K.data_ptr(), b, n, s_row,
                       s_col, dq.data_ptr(), dt.data_ptr(), cq.data_ptr(),
                       ct.data_ptr(), 0 if comp is None else comp.data_ptr(),
                       parts, ws_w2.data_ptr(), ws_j.data_ptr(),
                       flag.data_ptr(), stream=stream)
        if parts > 1:
            _module.launch('mst_combine', -(-b // _BLOCK), _BLOCK, 'QQqqQQ',
                           ws_w2.data_ptr(), ws_j.data_ptr(), b, parts,
                           w2.data_ptr(), cand.data_ptr(), stream=stream)
    return w2, cand, flag


def rows(K, diag, c2, comp, parts=None, flag=None):
    """``(w2 (n,) float64, cand (n,) int32, flag (1,) int32)`` on K's device
    (`mst_rows_*`, and `mst_combine` where the columns are split): per row i
    its smallest edge ``(w2(i, j), j)`` to a column j of another component,
    ``(inf, -1)`` where there is none; `flag` is not zero if some d2 is not
    finite before its clamp.

    K: (n, n) float32 or float64 CUDA tensor, any strides without negative
    values (read as it lies, both triangles).  diag, c2 (n,) float64, comp
    (n,) int32: the label of every sample's component.  parts: the split of
    the columns in the place of `parts_for`'s choice.  flag: a flag word to
    raise instead of a new one."""
    n, diag, c2, comp = _check_rows(K, diag, c2, comp)
    return _rows(K, n, n, diag, diag, c2, c2, comp, parts, flag)


def cross_rows(Ks, dq, dt, cq, ct, parts=None, flag=None):
    """The same three for the rows of a (b, n) cross matrix against all its
    columns, nothing symmetrised: ``w2 = max(cq[i], ct[j], d2(i, j))`` (the
    rectangular mode of `mst_rows_*`)."""
    b, n, dq, dt, cq, ct = _check_cross(Ks, dq, dt, cq, ct)
    return _rows(Ks, b, n, dq, dt, cq, ct, None, parts, flag)


def _d2_torch(K, dq, dt):
    """(d2 after the clamp, flag) by torch."""
    import torch
    d2 = (dq[:, None] + dt[None, :]) - 2.0 * K.to(torch.float64)
    bad = ~torch.isfinite(d2)
    d2 = torch.where(bad, torch.full_like(d2, float('inf')), d2)
    d2 = torch.where(d2 < 0.0, torch.zeros_like(d2), d2)
    return d2, bad.any().to(torch.int32).reshape(1)


def weights_torch(K, diag, c2):
    """(w2 (n, n), flag) by torch (the restatement writes the matrix)."""
    import torch
    d2, flag = _d2_torch(K, diag, diag)
    w2 = torch.maximum(torch.minimum(d2, d2.T),
                       torch.maximum(c2[:, None], c2[None, :]))
    return w2, flag


def _first_minimum(w2, allowed):
    """(value, column) per row of the first minimum among the allowed
    entries; (inf, -1) for a row without one."""
    import torch
    inf = torch.full_like(w2, float('inf'))
    val = torch.where(allowed, w2, inf).min(1).values
    hit = allowed & (w2 == val[:, None])
    cand = hit.to(torch.int8).argmax(1).to(torch.int32)
    none = ~hit.any(1)
    return (torch.where(none, inf[:, 0], val),
            torch.where(none, torch.full_like(cand, -1), cand))


def rows_torch(K, diag, c2, comp, flag=None, weights=None):
    """`rows` by torch on any device.  weights: `weights_torch`'s pair, for
    a loop that calls this every round."""
    n, diag, c2, comp = _check_rows(K, diag, c2, comp)
    w2, bad = weights_torch(K, diag, c2) if weights is None else weights
    val, cand = _first_minimum(w2, comp[:, None] != comp[None, :])
    return val, cand, bad if flag is None else flag | bad


def cross_rows_torch(Ks, dq, dt, cq, ct, flag=None):
    """`cross_rows` by torch on any device."""
    import torch
    b, n, dq, dt, cq, ct = _check_cross(Ks, dq, dt, cq, ct)
    d2, bad = _d2_torch(Ks, dq, dt)
    w2 = torch.maximum(d2, torch.maximum(cq[:, None], ct[None, :]))
    val, cand = _first_minimum(w2, torch.ones_like(w2, dtype=torch.bool))
    return val, cand, bad if flag is None else flag | bad


# -- a round behind the row pass -------------------------------------------------------
def new_edges(n, device):
    """``(w2 (n,) float64, a (n,) int32, b (n,) int32)``: the edge buffers of
    a run, nothing written yet (nan, -1, -1).  Slot r takes the edge by which
    root r vanishes."""
    import torch
    return (torch.full((n,), float('nan'), dtype=torch.float64, device=device),
            torch.full((n,), -1, dtype=torch.int32, device=device),
            torch.full((n,), -1, dtype=torch.int32, device=device))


def _check_hook(w2, cand, comp, edges):
    import torch
    if not torch.is_tensor(w2) or w2.dim() != 1:
        raise TypeError('w2: an (n,) float64 tensor expected')
    n, dev = w2.shape[0], w2.device
    out = [_vector('w2', w2, n, dev, torch.float64),
           _vector('cand', cand, n, dev, torch.int32),
           _vector('comp', comp, n, dev, torch.int32)]
    for name, e, dtype in zip(('edge w2', 'edge a', 'edge b'), edges,
                              (torch.float64, torch.int32, torch.int32)):
        _vector(name, e, n, dev, dtype)
        if not e.is_contiguous():
            raise ValueError(f'{name}: a contiguous buffer expected (it is '
                             'written in place)')
    return [n] + out


def hook(w2, cand, comp, edges, components=None):
    """``(comp' (n,) int32, count (workgroups,) int32)`` on the device of the
    candidates (`mst_best_w`, `mst_best_e`, `mst_hook`, `mst_jump`,
    `mst_relabel`): every component takes the smallest ``(w2, min, max)`` of
    its rows' candidates ``(w2[i], {i, cand[i]})`` and hooks its root to the
    other end's; of two that chose the same edge the smaller root stays; the
    forest is flattened and every sample relabelled.  ``count.sum()`` samples
    are their own label: the components left.  A root r that vanishes writes
    its edge into slot r of `edges` (`new_edges`), in place.

    comp: the labels, each the index of a sample of its component that
    carries its own label (a root).  components: how many there are (n if
    not given); it bounds the launches that flatten."""
    import torch
    n, w2, cand, comp = _check_hook(w2, cand, comp, edges)
    _cuda(w2)
    dev = w2.device
    grid = max(1, -(-n // _BLOCK))
    with torch.cuda.device(dev):
        out = torch.empty_like(comp)
        count = torch.zeros(grid, dtype=torch.int32, device=dev)
        if n == 0:
            return out, count
        stream = current_stream(dev)
        # (all bits set: the key of no candidate)
        best = torch.full((2, n), -1, dtype=torch.int64, device=dev)
        parent = torch.empty((2, n), dtype=torch.int32, device=dev)
        best_w, best_e = best[0].data_ptr(), best[1].data_ptr()
        _module.launch('mst_best_w', grid, _BLOCK, 'QQQqQ', w2.data_ptr(),
                       cand.data_ptr(), comp.data_ptr(), n, best_w,
                       stream=stream)
        _module.launch('mst_best_e', grid, _BLOCK, 'QQQqQQ', w2.data_ptr(),
                       cand.data_ptr(), comp.data_ptr(), n, best_w, best_e,
                       stream=stream)
        _module.launch('mst_hook', grid, _BLOCK, 'QqQQQQQQ', comp.data_ptr(),
                       n, best_w, best_e, parent[0].data_ptr(),
                       edges[0].data_ptr(), edges[1].data_ptr(),
                       edges[2].data_ptr(), stream=stream)
        at = 0
        for _ in range(jumps_for(n if components is None else components)):
            _module.launch('mst_jump', grid, _BLOCK, 'QqQ',
                           parent[at].data_ptr(), n,
                           parent[1 - at].data_ptr(), stream=stream)
            at = 1 - at
        _module.launch('mst_relabel', grid, _BLOCK, 'QQqQQ', comp.data_ptr(),
                       parent[at].data_ptr(), n, out.data_ptr(),
                       count.data_ptr(), stream=stream)
    return out, count


def hook_torch(w2, cand, comp, edges, components=None):
    """`hook` by torch on any device, the count as one number."""
    import torch
    n, w2, cand, comp = _check_hook(w2, cand, comp, edges)
    dev = w2.device
    i = torch.arange(n, dtype=torch.int64, device=dev)
    c, j = comp.to(torch.int64), cand.to(torch.int64)
    has = (j >= 0) & (j < n) & (w2 >= 0.0)
    inf = torch.full_like(w2, float('inf'))
    best_w = inf.clone().scatter_reduce_(
        0, c[has], w2[has], 'amin', include_self=True)
    least = has & (w2 == best_w[c])
    none = torch.iinfo(torch.int64).max
    key = torch.minimum(i, j) * n + torch.maximum(i, j)
    best_e = torch.full((n,), none, dtype=torch.int64, device=dev)
    best_e.scatter_reduce_(0, c[least], key[least], 'amin', include_self=True)
    chose = (c == i) & (best_e != none)
    e = torch.where(chose, best_e, torch.zeros_like(best_e))
    a, b = e // n, e % n
    other = torch.where(c[a] == i, c[b], c[a])
    stays = (best_e[other] == best_e) & (i < other)
    gone = chose & ~stays & (other != i)
    parent = torch.where(gone, other, i)
    edges[0][gone] = best_w[gone]
    edges[1][gone] = a[gone].to(torch.int32)
    edges[2][gone] = b[gone].to(torch.int32)
    m = n if components is None else components
    for _ in range(max(0, (m - 1).bit_length())):
        parent = parent[parent]
    out = parent[c]
    return out.to(torch.int32), (out == i).sum().to(torch.int32).reshape(1)


# -- the tree --------------------------------------------------------------------------
def spanning_tree(K, diag, c2, flag=None, fused=None, parts=None,
                  name='spanning_tree'):
    """``(w2 (n - 1,) float64, a (n - 1,), b (n - 1,) int64, fused?)`` as
    numpy arrays, ``a < b``, in the order ``(w2, a, b)``: the edges of the
    minimum spanning tree of the mutual-reachability graph in that order.

    At most `rounds_most(n)` rounds of `rows` and `hook` (fused: a CUDA
    matrix) or of their restatements; after each, one download of the number
    of components and the flag word.  A raised flag word -- `flag`, where one
    is handed in, and the row passes' -- is a ValueError; more rounds a
    RuntimeError.  After the last round the n edge slots are downloaded
    once."""
    import torch
    n, diag, c2, _ = _check_rows(
        K, diag, c2, torch.empty(K.shape[0], dtype=torch.int32,
                                 device=K.device))
    if n < 1:
        raise ValueError(f'{name}: an empty matrix')
    if fused is None:
        fused = _declines(K) is None
    dev = K.device
    comp = torch.arange(n, dtype=torch.int32, device=dev)
    edges = new_edges(n, dev)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    weights = None if fused or n < 2 else weights_torch(K, diag, c2)
    components, done = n, 0
    while components > 1:
        if done == rounds_most(n):
            raise RuntimeError(f'{name}: {components} components after '
                               f'{done} rounds of {n} samples')
        if fused:
            w2, cand, flag = rows(K, diag, c2, comp, parts=parts, flag=flag)
            comp, count = hook(w2, cand, comp, edges, components)
        else:
            w2, cand, flag = rows_torch(K, diag, c2, comp, flag=flag,
                                        weights=weights)
            comp, count = hook_torch(w2, cand, comp, edges, components)
        left, bad = torch.stack((count.sum(), flag.sum())).cpu().tolist()
        if bad:
            raise ValueError(f'{name}: the kernel matrix has entries that '
                             'are not finite')
        if not 1 <= left <= components // 2:
            raise RuntimeError(f'{name}: {left} components after '
                               f'{components}')
        components, done = left, done + 1
    if n == 1 and int(flag.sum()):
        raise ValueError(f'{name}: the kernel matrix has entries that are '
                         'not finite')
    down = torch.stack((edges[0], edges[1].to(torch.float64),
                        edges[2].to(torch.float64))).cpu().numpy()
    kept = down[1] >= 0
    if int(kept.sum()) != n - 1:
        raise RuntimeError(f'{name}: {int(kept.sum())} edges of {n} samples')
    return sort_edges(down[0][kept], down[1][kept].astype(np.int64),
                      down[2][kept].astype(np.int64)) + (fused,)


def sort_edges(w2, a, b):
    """The edges in the order ``(w2, a, b)``."""
    order = np.lexsort((b, a, w2))
    return w2[order], a[order], b[order]
