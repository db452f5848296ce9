"""Host side of lloyd.hip, the kernel k-means iteration behind `KernelKMeans`:
compiles the kernels once (JIT cache of graphdot_amd.hip.jit, IEEE arithmetic:
no fast-math) and runs them on torch's *current* stream of the matrix's
device, in stream order with the torch operations around them.  No launch here
synchronises with the host.  Every launch has a ``*_torch`` restatement on any
device: the yardstick of the kernels and the host path of the model (DESIGN.md
section 28).

All R restarts travel together: labels are (R, n) int32, ``S[r, i, c] = sum
of K[i, j] over the j with labels[r, j] = c`` is (R, n, k) float64, and the
per-row-block shares ``part = [T (k) | counts (k)]`` are (R, row blocks, 2 k),
added up by every consumer in the same fixed order."""
import numpy as np
from ...hip.source_module import STATIC, chunk, current_stream, suffix
from .._dense_host import _check_K, _f64

_module = STATIC['lloyd.hip']
precompile = _module.precompile
_BLOCK = 256
_WAVE = 64
_ROWS = 16          # rows of K per workgroup of kkm_accumulate
KMAX = 64           # most clusters
INITS = ('k-means++', 'farthest')
#: the host looks at `info` after every CHECK_EVERY rounds (one download of
#: 4 R numbers)
CHECK_EVERY = 4


def grid(n, k):
    """(chunk size KC, chunks, row blocks of accumulate, blocks of assign): a
    function of the shapes alone, so that the order of every sum is the same
    on every call."""
    kc = chunk(k)
    return kc, -(-k // kc), -(-n // _ROWS), -(-n // _BLOCK)


def _i32(name, t, shape, dev):
    import torch
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) \
            or t.device != dev:
        raise TypeError(f'{name}: {tuple(shape)} int32 on {dev} expected')
    return t.contiguous()


def _check_k(k, n):
    if int(k) != k or not 1 <= k <= min(KMAX, n):
        raise ValueError(f'n_clusters = {k}: an integer with 1 <= n_clusters '
                         f'<= min({KMAX}, n = {n}) expected')
    return int(k)


def _diag(K):
    import torch
    return K.diagonal().to(torch.float64)


# -- the start ---------------------------------------------------------------------
def _seed_args(k, n, init, u, seeds):
    """(mode, R, u (R, k) float64 or None, seeds (R, k) int32 or None) as numpy
    arrays, checked."""
    if init not in INITS + ('given',):
        raise ValueError(f'init: one of {INITS} or an array of seed indices '
                         f'expected, got {init!r}')
    if init == 'given':
        seeds = np.asarray(seeds)
        if seeds.dtype.kind not in 'iu' or seeds.ndim not in (1, 2) \
                or seeds.shape[-1] != k:
            raise ValueError(f'init: integer seed indices of shape ({k},) or '
                             f'(R, {k}) expected')
        seeds = np.atleast_2d(seeds)
        if seeds.shape[0] < 1 or seeds.min() < 0 or seeds.max() >= n:
            raise ValueError(f'init: seed indices from 0 to {n - 1} expected')
        if any(len(set(row)) != k for row in seeds.tolist()):
            raise ValueError('init: repeated seed indices')
        return 2, seeds.shape[0], None, np.ascontiguousarray(seeds, np.int32)
    u = np.ascontiguousarray(u, dtype=np.float64)
    if u.ndim != 2 or u.shape[1] != k or u.shape[0] < 1 \
            or not np.all((u >= 0) & (u < 1)):
        raise ValueError(f'u: (R, {k}) numbers in [0, 1) expected')
    return INITS.index(init), u.shape[0], u, None


def seed(K, k, init='k-means++', u=None, seeds=None):
    """``(seeds (R, k) int32, labels (R, n) int32, mind (R, n))`` of
    `kkm_seed_*`: k seed samples per restart, every sample labelled with its
    nearest seed (the lowest cluster on a tie) and its squared distance
    ``mind`` to that seed, ``(K_ii + K_jj) - 2 K_ij`` clamped at 0.

    init 'k-means++': seed 0 is ``floor(u[r, 0] n)`` and seed t the smallest
    i whose inclusive prefix sum of mind exceeds ``u[r, t] total`` (the lowest
    index not chosen yet if the total is 0); 'farthest': seed t is ``argmax
    mind`` (the lowest index on a tie); 'given': `seeds` are taken as they
    are.  `u`: (R, k) in [0, 1)."""
    import torch
    n = _check_K(K)
    k = _check_k(k, n)
    mode, R, u, given = _seed_args(k, n, init, u, seeds)
    dev = K.device
    with torch.cuda.device(dev):
        ud = torch.zeros((R, k), dtype=torch.float64, device=dev) \
            if u is None else torch.from_numpy(u).to(dev)
        sd = torch.zeros((R, k), dtype=torch.int32, device=dev) \
            if given is None else torch.from_numpy(given).to(dev)
        lab = torch.empty((R, n), dtype=torch.int32, device=dev)
        mind = torch.empty((R, n), dtype=torch.float64, device=dev)
        _module.launch(f'kkm_seed_{suffix(K.dtype)}', R, _BLOCK, 'QqiiQQQQ',
                       K.data_ptr(), n, k, mode, ud.data_ptr(), sd.data_ptr(),
                       lab.data_ptr(), mind.data_ptr(),
                       stream=current_stream(dev))
    return sd, lab, mind


def seed_torch(K, k, init='k-means++', u=None, seeds=None):
    """The same with `torch.cumsum` for the prefix sums (their order is not
    the kernel's: the chosen index can differ where ``u total`` falls within
    the rounding of a prefix)."""
    import torch
    n = K.shape[0]
    k = _check_k(k, n)
    mode, R, u, given = _seed_args(k, n, init, u, seeds)
    K = K.to(torch.float64)
    d = _diag(K)
    out = np.zeros((R, k), dtype=np.int32)
    lab = torch.zeros((R, n), dtype=torch.int32, device=K.device)
    mind = torch.zeros((R, n), dtype=torch.float64, device=K.device)
    for r in range(R):
        for t in range(k):
            if mode == 2:
                j = int(given[r, t])
            elif t == 0:
                j = min(n - 1, int(u[r, 0] * n))
            elif mode == 1:
                j = int(torch.argmax(mind[r]))
            else:
                cum = torch.cumsum(mind[r], 0)
                total = float(cum[-1])
                x = u[r, t] * total
                if not x < total:
                    x = total * (1.0 - np.finfo(np.float64).eps)
                hit = torch.nonzero(cum > x)
                if total > 0 and len(hit):
                    j = int(hit[0])
                else:
                    j = min(set(range(n)) - set(out[r, :t].tolist()))
            out[r, t] = j
            dist = torch.clamp_min((d + d[j]) - 2.0 * K[j], 0.0)
            dist = torch.where(torch.isnan(dist), torch.zeros_like(dist), dist)
            if t == 0:
                mind[r] = dist
            else:
                closer = dist < mind[r]
                mind[r] = torch.where(closer, dist, mind[r])
                lab[r] = torch.where(closer, torch.full_like(lab[r], t), lab[r])
    return torch.from_numpy(out).to(K.device), lab, mind


# -- one round: accumulate, assign, reduce ---------------------------------------------
def _check_labels(labels, n):
    import torch
    if not torch.is_tensor(labels) or labels.dim() != 2 \
            or labels.shape[1] != n or labels.shape[0] < 1:
        raise ValueError(f'labels: (R, {n}) expected')
    return labels.shape[0]


def accumulate(K, labels, k, out=None):
    """``(S, part)`` of `kkm_accumulate_*`: ``S`` (R, n, k) and ``part`` (R,
    row blocks, 2 k), per block of 16 rows the shares of ``T[c] = sum of S[i,
    c] over the i with label c`` and of the cluster sizes.

    K: (n, n) float32 or float64 CUDA tensor, symmetric, contiguous along
    either index, 16-byte aligned (read as it lies).  labels: (R, n) int32 in
    {0..k-1} (the caller's to guarantee).  `out`: the pair of tensors to write
    into (new ones otherwise)."""
    import torch
    n = _check_K(K)
    k = _check_k(k, n)
    dev = K.device
    R = _check_labels(labels, n)
    labels = _i32('labels', labels, (R, n), dev)
    kc, nch, nrb, _ = grid(n, k)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty((R, n, k), dtype=torch.float64, device=dev),
                   torch.empty((R, nrb, 2 * k), dtype=torch.float64,
                               device=dev))
        S = _f64('S', out[0], (R, n, k), dev)
        part = _f64('part', out[1], (R, nrb, 2 * k), dev)
        _module.launch(f'kkm_accumulate_{suffix(K.dtype)}_k{kc}',
                       R * nch * nrb, _BLOCK, 'QqiQQQ', K.data_ptr(), n, k,
                       labels.data_ptr(), S.data_ptr(), part.data_ptr(),
                       stream=current_stream(dev))
    return S, part


def accumulate_torch(K, labels, k, out=None):
    """The same as one product of K with the one-hot matrices of all restarts
    (one row block)."""
    import torch
    R, n = labels.shape
    Z = torch.nn.functional.one_hot(labels.long(), k).to(torch.float64)
    S = (K.to(torch.float64) @ Z.permute(1, 0, 2).reshape(n, R * k)) \
        .reshape(n, R, k).permute(1, 0, 2).contiguous()
    part = torch.cat(((S * Z).sum(1), Z.sum(1)), dim=1)
    return S, part[:, None, :]


def assign(K, labels, S, part, out=None):
    """``(next, apart)`` of `kkm_assign_*`: the next labels ``argmin_c d2(i,
    c)`` (the lowest cluster on a tie, never an empty one), ``d2(i, c) = K_ii
    - 2 S_ic / n_c + T_c / n_c^2``, and ``apart`` (R, 3, blocks): per block of
    256 samples the shares of the number of changed labels, of the inertia
    ``sum_i (K_ii - S[i, l_i] / n_{l_i})`` of the labels *used*, and of the
    number of samples with a K_ii or an S that is not finite."""
    import torch
    n = _check_K(K)
    dev = K.device
    R = _check_labels(labels, n)
    labels = _i32('labels', labels, (R, n), dev)
    if S.dim() != 3 or not 1 <= S.shape[2] <= min(KMAX, max(n, 1)):
        raise ValueError(f'S: (R, n, k) with 1 <= k <= {KMAX} expected')
    k = S.shape[2]
    S = _f64('S', S, (R, n, k), dev)
    if part.dim() != 3 or part.shape[1] < 1:
        raise ValueError(f'part: ({R}, row blocks, {2 * k}) expected')
    part = _f64('part', part, (R, part.shape[1], 2 * k), dev)
    nab = grid(n, k)[3]
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty((R, n), dtype=torch.int32, device=dev),
                   torch.empty((R, 3, nab), dtype=torch.float64, device=dev))
        nxt = _i32('next', out[0], (R, n), dev)
        apart = _f64('apart', out[1], (R, 3, nab), dev)
        if nxt.data_ptr() == labels.data_ptr():
            raise ValueError('the next labels cannot overwrite the labels')
        _module.launch(f'kkm_assign_{suffix(K.dtype)}', R * nab, _BLOCK,
                       'QqiQQQqQQ', K.data_ptr(), n, k, labels.data_ptr(),
                       S.data_ptr(), part.data_ptr(), part.shape[1],
                       nxt.data_ptr(), apart.data_ptr(),
                       stream=current_stream(dev))
    return nxt, apart


def totals_torch(part):
    """(T (R, k), counts (R, k)) of the shares `part`."""
    k = part.shape[2] // 2
    tot = part.sum(1)
    return tot[:, :k], tot[:, k:]


def distances_torch(diag, S, T, counts):
    """d2 (R, n, k); +inf for an empty cluster and where it is NaN."""
    import torch
    c = counts[:, None, :]
    d2 = diag[None, :, None] - 2.0 * (S / c) + (T / (counts * counts))[:, None]
    return torch.where((c > 0) & ~torch.isnan(d2), d2,
                       torch.full_like(d2, float('inf')))


def assign_torch(K, labels, S, part, out=None):
    import torch
    diag = _diag(K)
    T, counts = totals_torch(part)
    nxt = torch.argmin(distances_torch(diag, S, T, counts), dim=2) \
        .to(torch.int32)
    own = torch.gather(S, 2, labels.long()[:, :, None])[:, :, 0] \
        / torch.gather(counts, 1, labels.long())
    bad = ~(torch.isfinite(S).all(2) & torch.isfinite(diag)[None, :])
    apart = torch.stack(((nxt != labels).sum(1).to(torch.float64),
                         (diag[None, :] - own).sum(1),
                         bad.sum(1).to(torch.float64)), dim=1)
    return nxt, apart[:, :, None]


def reduce(apart, info, round):
    """Adds the shares of `apart` up into ``info (R, 4) = [changed, inertia,
    status, stamp]`` in place (`kkm_reduce`): the status stays set once a
    share of it was, and the stamp becomes `round` the first time nothing
    changed."""
    import torch
    if not apart.is_cuda:
        raise TypeError('apart: a CUDA tensor expected; see reduce_torch')
    dev = apart.device
    if apart.dim() != 3 or apart.shape[1] != 3 or apart.shape[2] < 1:
        raise ValueError('apart: (R, 3, blocks) expected')
    R = apart.shape[0]
    apart = _f64('apart', apart, apart.shape, dev)
    info = _f64('info', info, (R, 4), dev)
    with torch.cuda.device(dev):
        _module.launch('kkm_reduce', R, _BLOCK, 'QqiQ', apart.data_ptr(),
                       apart.shape[2], int(round), info.data_ptr(),
                       stream=current_stream(dev))
    return info


def reduce_torch(apart, info, round):
    import torch
    tot = apart.sum(2)
    status = (info[:, 2] != 0) | (tot[:, 2] != 0)
    info[:, 0], info[:, 1] = tot[:, 0], tot[:, 1]
    info[:, 2] = status.to(torch.float64)
    first = (info[:, 3] == 0) & (tot[:, 0] == 0) & ~status
    info[:, 3] = torch.where(first, torch.full_like(info[:, 3], float(round)),
                             info[:, 3])
    return info


class Result:
    """What `iterate` found.  Per restart: `labels` (R, n) int32 and `S` (R,
    n, k), `T`, `counts` (R, k) (tensors where the matrix is; the labels the
    last round *used* and their sums), `inertia`, `n_iter`, `status`,
    `converged` (numpy); `best`: the restart of lowest inertia among those
    without a status (the lowest index on a tie); `seeds` (R, k) or None;
    `rounds` run and `looks` the host took."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def start_labels(labels0, n, k):
    """(R, n) int32 numpy start labels, checked."""
    lab = np.asarray(labels0)
    if lab.dtype.kind not in 'iu' or lab.ndim not in (1, 2) \
            or lab.shape[-1] != n or lab.size == 0:
        raise ValueError(f'labels0: integers of shape ({n},) or (R, {n}) '
                         f'expected, got {lab.dtype} {lab.shape}')
    if lab.min() < 0 or lab.max() >= k:
        raise ValueError(f'labels0: labels from 0 to {k - 1} expected')
    return np.ascontiguousarray(np.atleast_2d(lab), dtype=np.int32)


def iterate(K, k, labels0=None, init='k-means++', n_init=10, max_iter=300,
            random_state=0, u=None):
    """Kernel k-means from `labels0` ((n,) or (R, n)) or from the seeding
    `init` ('k-means++', 'farthest' or seed indices (k,) or (R, k)) with
    `n_init` restarts, whose uniform numbers `u` (R, k) are drawn from
    `random_state` once: the HIP launches for a CUDA matrix, their
    restatements for a CPU one.  Three launches per round on the current
    stream and no download, except that of ``info`` (4 R numbers) after every
    `CHECK_EVERY`-th round (4, 8, 12, ...) and after the last one.  A restart
    has converged in the first round that changes none of its labels; the run
    ends at the first look at which every restart has converged or carries a
    status (a K_ii or S that is not finite), or after `max_iter` rounds."""
    import torch
    n = K.shape[0]
    k = _check_k(k, n)
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f'max_iter: a positive integer expected, got '
                         f'{max_iter}')
    if K.is_cuda:
        f_seed, f_acc, f_asg, f_red = seed, accumulate, assign, reduce
    else:
        f_seed, f_acc, f_asg, f_red = (seed_torch, accumulate_torch,
                                       assign_torch, reduce_torch)
        K = K.to(torch.float64)
    seeds = None
    if labels0 is not None:
        first = torch.from_numpy(start_labels(labels0, n, k)).to(K.device)
    else:
        if not isinstance(init, str):
            init, given = 'given', init
        else:
            given = None
            if u is None:
                if int(n_init) != n_init or n_init < 1:
                    raise ValueError('n_init: a positive integer expected, '
                                     f'got {n_init}')
                u = np.random.default_rng(random_state).random(
                    (int(n_init), k))
        seeds, first, _ = f_seed(K, k, init, u, given)
    R = first.shape[0]
    # (the labels are read while the next ones are written: two alternate)
    lab = [first, torch.empty_like(first)]
    info = torch.zeros((R, 4), dtype=torch.float64, device=K.device)
    apart = torch.empty((R, 3, grid(n, k)[3]), dtype=torch.float64,
                        device=K.device) if K.is_cuda else None
    o_acc = None
    looks = 0
    for it in range(1, int(max_iter) + 1):
        used = lab[(it - 1) % 2]
        o_acc = S, part = f_acc(K, used, k, o_acc)
        lab[it % 2], shares = f_asg(K, used, S, part,
                                    (lab[it % 2], apart) if K.is_cuda else None)
        f_red(shares, info, it)
        if it % CHECK_EVERY and it != max_iter:
            continue
        h = info.cpu().numpy()
        looks += 1
        if np.all((h[:, 3] > 0) | (h[:, 2] != 0)):
            break
    status = (h[:, 2] != 0).astype(np.int64)
    converged = h[:, 3] > 0
    inertia = h[:, 1].copy()
    T, counts = totals_torch(part)
    return Result(
        labels=used, S=S, T=T, counts=counts, inertia=inertia,
        n_iter=np.where(converged, h[:, 3], it).astype(np.int64),
        status=status, converged=converged, seeds=seeds, rounds=it,
        looks=looks,
        best=int(np.argmin(np.where((status == 0) & ~np.isnan(inertia),
                                    inertia, np.inf))))


# -- new rows ----------------------------------------------------------------------
def predict(Ks, labels, T, counts):
    """``(D, arg)`` of `kkm_predict_*`: ``D[z, c] = -2 S_zc / n_c + T_c /
    n_c^2`` (b, k) float64 (+inf for an empty cluster), ``S_zc`` the sum of
    ``Ks[z, i]`` over the i with label c, and its argmin (b,) int32 (the
    lowest cluster on a tie), in one launch.

    Ks: (b, n) float32 or float64 CUDA tensor, any positive strides (read as
    it lies; column-major, as the solver leaves it, is the coalesced one).
    labels: (n,) int32; T, counts: (k,) float64."""
    import torch
    if not labels.is_cuda:
        raise TypeError('labels: a CUDA tensor expected; see predict_torch')
    dev = labels.device
    n = labels.shape[0]
    labels = _i32('labels', labels, (n,), dev)
    if T.dim() != 1 or not 1 <= T.shape[0] <= KMAX:
        raise ValueError(f'T: (k,) with 1 <= k <= {KMAX} expected')
    k = T.shape[0]
    T, counts = _f64('T', T, (k,), dev), _f64('counts', counts, (k,), dev)
    if Ks.dim() != 2 or Ks.shape[1] != n \
            or Ks.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'Ks: (b, {n}) float32 or float64 expected')
    if Ks.device != dev:
        raise ValueError('Ks and labels must be on the same device')
    if min(Ks.stride()) < 0:
        raise ValueError('Ks: negative strides')
    b = Ks.shape[0]
    with torch.cuda.device(dev):
        D = torch.empty((b, k), dtype=torch.float64, device=dev)
        arg = torch.empty((b,), dtype=torch.int32, device=dev)
        if b:
            _module.launch(
                f'kkm_predict_{suffix(Ks.dtype)}_k{chunk(k)}',
                -(-b // _WAVE), _BLOCK, 'QqqqqQQQiQQ', Ks.data_ptr(), b, n,
                Ks.stride(0), Ks.stride(1), labels.data_ptr(), T.data_ptr(),
                counts.data_ptr(), k, D.data_ptr(), arg.data_ptr(),
                stream=current_stream(dev))
    return D, arg


def predict_torch(Ks, labels, T, counts):
    import torch
    k = T.shape[0]
    Z = torch.nn.functional.one_hot(labels.long(), k).to(torch.float64)
    D = -2.0 * ((Ks.to(torch.float64) @ Z) / counts) + T / (counts * counts)
    D = torch.where((counts > 0) & ~torch.isnan(D), D,
                    torch.full_like(D, float('inf')))
    return D, torch.argmin(D, dim=1).to(torch.int32)
