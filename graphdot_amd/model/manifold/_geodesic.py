"""Host side of geodesic.h, geodesic distances on the neighbourhood graph of a
kernel matrix where it lies: compiles the kernels once
(`MODEL_UNITS['geodesic']`; JIT cache of graphdot_amd.hip.jit, IEEE
arithmetic: no fast-math) and runs them on torch's *current* stream of the
matrix's device as plain launches, in stream order with the torch operations
around them and with no host synchronisation between them.  Two (n, n) double
buffers are written, G and B; K is never copied.  The ``*_torch`` functions
are the same chain through torch on any device: the restatement the kernels
are compared with, and the path of CPU tensors, of more than `K_MOST`
neighbours and of matrices the launches decline.

With the self-similarities diag (n,), ``d2(i, j) = max(0, (diag[i] +
diag[j]) - 2 K[i, j])``.  The graph has the edge {i, j} where j is in the
neighbour list of i or i in that of j, of length ``W[i, j] = sqrt(min(d2(i,
j), d2(j, i)))``; ``W[i, i] = 0`` and ``W = inf`` elsewhere.  G holds the
lengths of the shortest paths in W, ``B = -0.5 G * G``, and a new sample with
the list ``(d2_r, j_r)`` is at ``Gq[j] = min_r (sqrt(d2_r) + G[j_r, j])``
from training sample j."""
from ...hip.source_module import MODEL_UNITS, current_stream, suffix

_module = MODEL_UNITS['geodesic']
precompile = _module.precompile
_BLOCK = 256
#: rows and columns per tile of the graph and of Floyd-Warshall
TILE = 64
#: most neighbours per list of the fused chain: the lists are staged in LDS
K_MOST = 64
_FIN_ROWS = 16      # rows per workgroup of geo_finish
_EXT_ROWS = 16      # query rows per workgroup of geo_extend
#: the largest n: the labels and the staged lists are ints
_N_MOST = 2 ** 31 - 1 - TILE
ENTRY_POINTS = ('geo_graph_f32', 'geo_graph_f64', 'geo_fw_diag',
                'geo_fw_cross', 'geo_fw_rest', 'geo_finish', 'geo_extend')


def rounds(n):
    """R, the tiles along one side of an (n, n) matrix: the rounds of the
    blocked Floyd-Warshall algorithm."""
    return -(-n // TILE)


# -- the argument checks ---------------------------------------------------------------
def _check_graph(K, diag, idx):
    """(n, k) of checked arguments, any device."""
    import torch
    if not torch.is_tensor(K) or K.dim() != 2 or K.shape[0] != K.shape[1] \
            or K.dtype not in (torch.float32, torch.float64):
        raise TypeError('K: an (n, n) float32 or float64 tensor expected')
    n = K.shape[0]
    if min(K.stride()) < 0:
        raise ValueError('K: negative strides')
    if not torch.is_tensor(diag) or diag.dtype != torch.float64 \
            or tuple(diag.shape) != (n,) or diag.device != K.device:
        raise TypeError(f'diag: ({n},) float64 on {K.device} expected')
    if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() != 2 \
            or idx.shape[0] != n or idx.shape[1] < 1 \
            or idx.device != K.device:
        raise TypeError(f'idx: ({n}, k) int64 on {K.device} expected')
    return n, idx.shape[1]


def _square(name, G):
    import torch
    if not torch.is_tensor(G) or G.dtype != torch.float64 or G.dim() != 2 \
            or G.shape[0] != G.shape[1]:
        raise TypeError(f'{name}: an (n, n) float64 tensor expected')
    return G.shape[0]


def _check_lists(d2, idx, G):
    """(b, k, n) of checked arguments, any device."""
    import torch
    n = _square('G', G)
    if not torch.is_tensor(d2) or not torch.is_tensor(idx) \
            or d2.dtype != torch.float64 or idx.dtype != torch.int64 \
            or d2.dim() != 2 or d2.shape != idx.shape or d2.shape[1] < 1 \
            or d2.device != G.device or idx.device != G.device:
        raise TypeError('lists: (b, k) float64 squared distances and int64 '
                        f'indices on {G.device} expected')
    return d2.shape[0], d2.shape[1], n


def _cuda(name, t):
    if not t.is_cuda:
        raise TypeError(f'{name}: a CUDA tensor expected; see the *_torch '
                        'restatements')
    if t.shape[-1] > _N_MOST:
        raise ValueError(f'{name}: {_N_MOST} columns at the most')


def _declines(K, k):
    """Why the fused chain is not for this call (None: it is)."""
    if not K.is_cuda:
        return 'not a CUDA tensor'
    if k > K_MOST:
        return f'more than {K_MOST} neighbours'
    if K.shape[0] > _N_MOST:
        return 'too many samples'
    return None


# -- the graph -------------------------------------------------------------------------
def graph(K, diag, idx):
    """``W (n, n)`` float64 on K's device (`geo_graph_*`): the lengths of the
    edges of the neighbourhood graph, 0 on the diagonal and inf elsewhere,
    symmetric to the bit.

    K: (n, n) float32 or float64 CUDA tensor, any strides without negative
    values (read as it lies, both triangles).  diag (n,) float64.  idx (n,
    k) int64, ``k <= K_MOST``: the lists of the `exclude_self` search."""
    import torch
    n, k = _check_graph(K, diag, idx)
    _cuda('K', K)
    if k > K_MOST:
        raise ValueError(f'n_neighbors = {k}: {K_MOST} at the most; see '
                         'graph_torch')
    dev = K.device
    with torch.cuda.device(dev):
        W = torch.empty((n, n), dtype=torch.float64, device=dev)
        if n:
            diag, idx = diag.contiguous(), idx.contiguous()
            s_row, s_col = K.stride()
            _module.launch(f'geo_graph_{suffix(K.dtype)}', rounds(n) ** 2,
                           _BLOCK, 'QqqqQQiQ', K.data_ptr(), n, s_row, s_col,
                           diag.data_ptr(), idx.data_ptr(), k, W.data_ptr(),
                           stream=current_stream(dev))
    return W


def graph_torch(K, diag, idx):
    """The same matrix by torch on any device (the restatement writes the (n,
    n) matrix of d2 and a mask of the edges)."""
    import torch
    n, k = _check_graph(K, diag, idx)
    d2 = (diag[:, None] + diag[None, :]) - 2.0 * K.to(torch.float64)
    d2 = torch.where(d2 < 0.0, torch.zeros_like(d2), d2)
    d2 = torch.minimum(d2, d2.T)
    edge = torch.zeros((n, n), dtype=torch.bool, device=K.device)
    edge.scatter_(1, idx, True)
    edge = edge | edge.T
    W = torch.where(edge, torch.sqrt(d2), torch.full_like(d2, float('inf')))
    W.diagonal().fill_(0.0)
    return W


# -- the shortest paths ----------------------------------------------------------------
def shortest_paths(G):
    """The lengths of the shortest paths in the graph whose edge lengths `G`
    holds, *in place* (`geo_fw_diag`, `geo_fw_cross`, `geo_fw_rest`, the three
    of them per round, `rounds(n)` rounds); returns `G`.

    G: (n, n) float64 contiguous CUDA tensor, symmetric to the bit, 0 on the
    diagonal, inf where there is no edge, no negative entry."""
    import torch
    n = _square('G', G)
    _cuda('G', G)
    if not G.is_contiguous():
        raise ValueError('G: a contiguous matrix expected (it is updated in '
                         'place)')
    dev = G.device
    R = rounds(n)
    with torch.cuda.device(dev):
        stream = current_stream(dev)
        for p in range(R):
            # (a phase without workgroups is not launched: R == 1)
            for name, grid in (('geo_fw_diag', 1),
                               ('geo_fw_cross', 2 * (R - 1)),
                               ('geo_fw_rest', (R - 1) ** 2)):
                if grid:
                    _module.launch(name, grid, _BLOCK, 'Qqq', G.data_ptr(), n,
                                   p, stream=stream)
    return G


def shortest_paths_torch(G):
    """The same lengths by torch on any device, not in place: n steps of
    ``minimum(G, G[:, m] + G[m, :])``."""
    import torch
    n = _square('G', G)
    for m in range(n):
        G = torch.minimum(G, G[:, m:m + 1] + G[m:m + 1, :])
    return G


# -- B and the components --------------------------------------------------------------
def finish(G):
    """``(B (n, n) float64, label (n,) int32, count (workgroups,) int32)`` on
    G's device (`geo_finish`): ``B = -0.5 * (G * G)``, per row the smallest
    index it reaches -- the label of its component -- and per workgroup the
    rows that are their own label: ``count.sum()`` components."""
    import torch
    n = _square('G', G)
    _cuda('G', G)
    G = G.contiguous()
    dev = G.device
    with torch.cuda.device(dev):
        B = torch.empty_like(G)
        label = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.zeros(max(1, -(-n // _FIN_ROWS)), dtype=torch.int32,
                            device=dev)
        if n:
            _module.launch('geo_finish', count.shape[0], _BLOCK, 'QqQQQ',
                           G.data_ptr(), n, B.data_ptr(), label.data_ptr(),
                           count.data_ptr(), stream=current_stream(dev))
    return B, label, count


def finish_torch(G):
    """The same three by torch on any device, the count as one number."""
    import torch
    n = _square('G', G)
    label = torch.argmax(torch.isfinite(G).to(torch.int8), dim=1).to(
        torch.int32)
    own = label == torch.arange(n, dtype=torch.int32, device=G.device)
    return -0.5 * (G * G), label, own.sum().to(torch.int32).reshape(1)


def component_sizes(label):
    """The sizes of the components, in the order of their labels, from the
    downloaded labels."""
    import numpy as np
    return np.unique(np.asarray(label), return_counts=True)[1].tolist()


# -- out of sample ---------------------------------------------------------------------
def extend(d2, idx, G, distances=False):
    """``(Bq, Gq)`` (b, n) float64 on G's device (`geo_extend`): the
    geodesics of new samples to the training samples through their lists
    ``(d2, idx)`` (b, k), ``k <= K_MOST``, and ``Bq = -0.5 * (Gq * Gq)``.
    `Gq` is None unless `distances`."""
    import torch
    b, k, n = _check_lists(d2, idx, G)
    _cuda('G', G)
    if k > K_MOST:
        raise ValueError(f'n_neighbors = {k}: {K_MOST} at the most; see '
                         'extend_torch')
    dev = G.device
    G, d2, idx = G.contiguous(), d2.contiguous(), idx.contiguous()
    with torch.cuda.device(dev):
        Bq = torch.empty((b, n), dtype=torch.float64, device=dev)
        Gq = torch.empty_like(Bq) if distances else None
        if b * n:
            grid = -(-b // _EXT_ROWS) * -(-n // _BLOCK)
            _module.launch('geo_extend', grid, _BLOCK, 'QQqiQqQQ',
                           d2.data_ptr(), idx.data_ptr(), b, k, G.data_ptr(),
                           n, Bq.data_ptr(),
                           Gq.data_ptr() if distances else 0,
                           stream=current_stream(dev))
    return Bq, Gq


def extend_torch(d2, idx, G, distances=False):
    """The same by torch on any device, a (b, n) pass per rank of the
    lists."""
    import torch
    b, k, n = _check_lists(d2, idx, G)
    d = torch.sqrt(d2)
    Gq = torch.full((b, n), float('inf'), dtype=torch.float64,
                    device=G.device)
    for r in range(k):
        Gq = torch.minimum(Gq, d[:, r:r + 1] + G[idx[:, r]])
    return -0.5 * (Gq * Gq), (Gq if distances else None)
