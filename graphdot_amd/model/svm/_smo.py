"""Host side of smo.hip, the SMO solver and the decision sums behind
`KernelSVC`: compiles the kernels once (JIT cache of graphdot_amd.hip.jit,
IEEE arithmetic: no fast-math) and runs them on torch's *current* stream of
the matrix's device, in stream order with the torch operations around them.
Both launches have a ``*_torch`` restatement on any device: the yardstick of
the kernels and the host path of the model.

A batch of P problems shares the (n, n) matrix: ``y`` (P, n) int8 in {+1, -1}
and the upper bounds ``U`` (P, n) float64, ``U = 0`` for a sample that is not
part of the problem.  Each minimises ``f(alpha) = 1/2 sum alpha_i alpha_j y_i
y_j K_ij - sum alpha_i`` subject to ``0 <= alpha <= U`` and ``y^T alpha = 0``
by SMO with the second-order working-set rule of Fan, Chen and Lin (the rule
libsvm uses), every choice taking the lowest index on a tie, all of it in
double whatever the type of K.

The fused path keeps ``G`` and ``alpha`` of a problem in LDS: 16 bytes per
sample of the 64 KB of static LDS, less 512 bytes for what the four waves
exchange in the two reductions of a step, so ``NMAX = (65536 - 512) / 16 =
4064``.  Larger matrices, CPU tensors and other devices take `smo_torch`.

Below the decision sums: the same solver entered with a given start (`smo_from`,
`one_class_start`: the one-class problem needs nothing else), and epsilon-SVR
on svr.hip (`smo2`, `smo2_torch`), whose 2n variables
over the n samples take 32 bytes of LDS per sample: ``NMAX2 = NMAX // 2``."""
import numpy as np
from ...hip.source_module import STATIC, chunk, current_stream, suffix
from .._dense_host import _check_K, _f64

_module = STATIC['smo.hip']
precompile = _module.precompile
_BLOCK = 256
_WAVE = 64
_LDS = 65536        # static LDS of a workgroup
_EXCHANGE = 512     # of which the reductions' exchange
NMAX = (_LDS - _EXCHANGE) // 16
TAU = 1e-12         # the curvature where K_ii + K_jj - 2 K_ij is not positive
#: steps per launch: the host looks at `info` (4 P numbers) after each
SLICE = 2048


class Result:
    """`alpha`, `G` (P, n) and `info` (P, 4) = [steps, m, M, status] as
    tensors where the matrix is; `slices`: the launches (looks of the host)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def stopped(info, tol, max_iter):
    """(P,) bool from `info` as a numpy array."""
    with np.errstate(invalid='ignore'):
        return (info[:, 3] != 0) | (info[:, 1] - info[:, 2] < tol) \
            | (info[:, 0] >= max_iter)


def _check_batch(y, U, n):
    import torch
    if not torch.is_tensor(y) or y.dtype != torch.int8 or y.dim() != 2 \
            or y.shape[1] != n or y.shape[0] < 1:
        raise TypeError(f'y: (P, {n}) int8 expected')
    if not torch.is_tensor(U) or U.dtype != torch.float64 \
            or U.shape != y.shape:
        raise TypeError(f'U: {tuple(y.shape)} float64 expected')
    return y.shape[0]


def _check_limits(tol, max_iter, steps=1):
    if not tol > 0:
        raise ValueError(f'tol: a positive number expected, got {tol}')
    for name, v in (('max_iter', max_iter), ('steps', steps)):
        if int(v) != v or v < 1:
            raise ValueError(f'{name}: a positive integer expected, got {v}')


def _info0(P, device):
    """info (P, 4) = [0, inf, -inf, 0] of a batch before its first step."""
    import torch
    info = torch.zeros((P, 4), dtype=torch.float64, device=device)
    info[:, 1], info[:, 2] = float('inf'), float('-inf')
    return info


def start(P, n, device):
    """(state (P, 2, n) = [alpha = 0 | G = -1], `_info0`) of a batch before
    its first step."""
    import torch
    state = torch.zeros((P, 2, n), dtype=torch.float64, device=device)
    state[:, 1] = -1.0
    return state, _info0(P, device)


def smo_slice(K, y, U, state, info, tol, steps, max_iter):
    """One launch of `svm_smo_*`: at most `steps` steps of every problem that
    has not stopped, on `state` and `info` in place."""
    import torch
    n = _check_K(K)
    if n > NMAX:
        raise ValueError(f'n = {n}: at most NMAX = {NMAX} on the fused path; '
                         'see smo_torch')
    dev = K.device
    P = _check_batch(y, U, n)
    _check_limits(tol, max_iter, steps)
    if y.device != dev or U.device != dev:
        raise ValueError('K, y and U must be on the same device')
    y, U = y.contiguous(), U.contiguous()
    state = _f64('state', state, (P, 2, n), dev)
    info = _f64('info', info, (P, 4), dev)
    with torch.cuda.device(dev):
        _module.launch(f'svm_smo_{suffix(K.dtype)}', P, _BLOCK, 'QiQQQQdqq',
                       K.data_ptr(), n, y.data_ptr(), U.data_ptr(),
                       state.data_ptr(), info.data_ptr(), float(tol),
                       int(steps), int(max_iter), stream=current_stream(dev))
    return state, info


def _relaunch(launch, state, info, tol, max_iter):
    """`launch()` advances `state` and `info` in place by a slice: again until
    every problem has stopped, the host looking at `info` after each."""
    slices = 0
    while True:
        launch()
        slices += 1
        if stopped(info.cpu().numpy(), tol, max_iter).all():
            break
    return Result(alpha=state[:, 0], G=state[:, 1], info=info, slices=slices)


def smo(K, y, U, tol=1e-3, max_iter=1_000_000, steps=SLICE):
    """The batch solved by relaunching `svm_smo_*` until every problem has
    stopped (``m - M < tol``, `max_iter` steps, or a status): one download of
    `info` per launch, nothing else.

    K: (n, n) float32 or float64 CUDA tensor, n <= NMAX, symmetric, contiguous
    along either index, 16-byte aligned (read as it lies)."""
    n = _check_K(K)
    P = _check_batch(y, U, n)
    _check_limits(tol, max_iter, steps)
    y, U = y.contiguous(), U.contiguous()
    state, info = start(P, n, K.device)
    return _relaunch(
        lambda: smo_slice(K, y, U, state, info, tol, steps, max_iter),
        state, info, tol, max_iter)


def _pair(ai, aj, Gi, Gj, Ui, Uj, differ, q):
    """libsvm's update of a pair along the constraint, clipped to its box, for
    every problem at once."""
    import torch
    w = torch.where
    zero = torch.zeros_like(ai)
    # y_i != y_j
    delta, diff = (-Gi - Gj) / q, ai - aj
    ni, nj = ai + delta, aj + delta
    c = diff > 0
    t = c & (nj < 0)
    ni, nj = w(t, diff, ni), w(t, zero, nj)
    t = ~c & (ni < 0)
    ni, nj = w(t, zero, ni), w(t, -diff, nj)
    c = diff > Ui - Uj
    t = c & (ni > Ui)
    ni, nj = w(t, Ui, ni), w(t, Ui - diff, nj)
    t = ~c & (nj > Uj)
    ni, nj = w(t, Uj + diff, ni), w(t, Uj, nj)
    # y_i == y_j
    delta, tot = (Gi - Gj) / q, ai + aj
    si, sj = ai - delta, aj + delta
    c = tot > Ui
    t = c & (si > Ui)
    si, sj = w(t, Ui, si), w(t, tot - Ui, sj)
    t = ~c & (sj < 0)
    si, sj = w(t, tot, si), w(t, zero, sj)
    c = tot > Uj
    t = c & (sj > Uj)
    si, sj = w(t, tot - Uj, si), w(t, Uj, sj)
    t = ~c & (si < 0)
    si, sj = w(t, zero, si), w(t, tot, sj)
    ni, nj = w(differ, ni, si), w(differ, nj, sj)
    # (the partner is a rounded difference: the clamp keeps it in its box)
    return torch.minimum(torch.clamp_min(ni, 0.0), Ui), \
        torch.minimum(torch.clamp_min(nj, 0.0), Uj)


def _loop_torch(K, s, U, state, info, tol, max_iter, rows):
    """The same rule with torch operations on N variables with the signs `s`
    (P, N) int8 and the bounds `U` (P, N), from a given `state` (P, 2, N) and
    `info`, all problems advancing together (one that has stopped is left
    unchanged); one look per step.  `rows(t)`: the (P, N) rows of the
    variables `t` (P,); `K` gives the diagonal."""
    import torch
    P, N = s.shape
    dev = K.device
    diag = K.diagonal().to(torch.float64)
    diag = diag.repeat(N // len(diag))
    sf = s.to(torch.float64)
    pos = s > 0
    alpha, G = state[:, 0], state[:, 1]
    inf = torch.full((P, N), float('inf'), dtype=torch.float64, device=dev)
    done = info[:, 0].clone()
    status = info[:, 3] != 0
    if not bool(torch.isfinite(diag).all()):
        status[:] = True
    col = torch.arange(P, device=dev)
    looks = 0
    while True:
        v = -sf * G
        up = torch.where(pos, alpha < U, alpha > 0)
        low = torch.where(pos, alpha > 0, alpha < U)
        m, i = torch.where(up, v, -inf).max(1)       # (the first on a tie)
        M = torch.where(low, v, inf).min(1).values
        status |= ~torch.isfinite(G).all(1)
        run = ~status & ~(m - M < tol) & (done < max_iter)
        looks += 1
        if not bool(run.any()):
            break
        Ki = rows(i)
        b = m[:, None] - v
        a = (diag[i][:, None] + diag[None, :]) - 2.0 * Ki
        a = torch.where(a <= 0, torch.full_like(a, TAU), a)
        cand = low & (v < m[:, None])
        obj = torch.where(cand, -(b * b) / a, inf)
        none = ~cand.any(1) | torch.isnan(obj).any(1)
        j = torch.where(torch.isnan(obj), inf, obj).argmin(1)
        Kj = rows(j)
        ai, aj = alpha[col, i], alpha[col, j]
        ni, nj = _pair(ai, aj, G[col, i], G[col, j], U[col, i], U[col, j],
                       s[col, i] != s[col, j], a[col, j])
        status |= run & none
        run &= ~none
        zero = torch.zeros_like(ai)
        si = torch.where(run, sf[col, i] * (ni - ai), zero)
        sj = torch.where(run, sf[col, j] * (nj - aj), zero)
        alpha[col, i] = torch.where(run, ni, ai)
        alpha[col, j] = torch.where(run, nj, alpha[col, j])
        G[:] = torch.where(run[:, None],
                           G + sf * (Ki * si[:, None] + Kj * sj[:, None]), G)
        done += run.to(torch.float64)
    info[:, 0], info[:, 1], info[:, 2] = done, m, M
    info[:, 3] = status.to(torch.float64)
    return Result(alpha=alpha, G=G, info=info, slices=looks)


def smo_torch(K, y, U, tol=1e-3, max_iter=1_000_000):
    """`_loop_torch` on the n samples from `start`."""
    import torch
    n = K.shape[0]
    P = _check_batch(y, U, n)
    _check_limits(tol, max_iter)
    K = K.to(torch.float64)
    dev = K.device
    return _loop_torch(K, y.to(dev), U.to(dev), *start(P, n, dev), tol,
                       max_iter, lambda t: K.index_select(0, t))


def _as_it_lies(K):
    """K where the kernels can read it as it lies (contiguous along one index,
    16-byte aligned: what `_check_K` asks for), else a copy that is."""
    n = K.shape[0]
    if n > 1 and K.stride() not in ((n, 1), (1, n)) or K.data_ptr() % 16:
        return K.contiguous()
    return K


def solve(K, y, U, tol, max_iter):
    """(Result, fused?): `smo` for a CUDA matrix of n <= NMAX, `smo_torch`
    anywhere else."""
    n = K.shape[0]
    if K.is_cuda and n <= NMAX:
        return smo(_as_it_lies(K), y.to(K.device), U.to(K.device), tol,
                   max_iter), True
    return smo_torch(K, y, U, tol, max_iter), False


# -- decision values --------------------------------------------------------------
def decide(Ks, coef, b):
    """``out[p, r] = sum_j Ks[r, j] coef[p, j] + b[p]`` (P, nb) float64 of
    `svm_decide_*`, the n terms split over four waves and added in order.

    Ks: (nb, n) float32 or float64 CUDA tensor, any positive strides (read as
    it lies).  coef: (P, n), b: (P,) float64."""
    import torch
    if not coef.is_cuda:
        raise TypeError('coef: a CUDA tensor expected; see decide_torch')
    dev = coef.device
    if coef.dim() != 2 or coef.shape[0] < 1:
        raise ValueError('coef: (P, n) expected')
    P, n = coef.shape
    coef, b = _f64('coef', coef, (P, n), dev), _f64('b', b, (P,), dev)
    if Ks.dim() != 2 or Ks.shape[1] != n \
            or Ks.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'Ks: (nb, {n}) float32 or float64 expected')
    if Ks.device != dev:
        raise ValueError('Ks and coef must be on the same device')
    if min(Ks.stride()) < 0:
        raise ValueError('Ks: negative strides')
    nb = Ks.shape[0]
    kc = chunk(P)
    with torch.cuda.device(dev):
        out = torch.empty((P, nb), dtype=torch.float64, device=dev)
        if nb:
            _module.launch(
                f'svm_decide_{suffix(Ks.dtype)}_k{kc}',
                -(-nb // _WAVE) * -(-P // kc), _BLOCK, 'QqqqqQQiQ',
                Ks.data_ptr(), nb, n, Ks.stride(0), Ks.stride(1),
                coef.data_ptr(), b.data_ptr(), P, out.data_ptr(),
                stream=current_stream(dev))
    return out


def decide_torch(Ks, coef, b):
    """The same, the n terms added one after the other in index order: a
    sample whose coefficient is zero adds an exact zero, so the values on a
    matrix and on its sub-matrix without such samples are the same bits."""
    import torch
    Ks = Ks.to(torch.float64)
    P, n = coef.shape
    out = torch.zeros((P, Ks.shape[0]), dtype=torch.float64, device=Ks.device)
    for j in range(n):
        out += coef[:, j, None] * Ks[None, :, j]
    return out + b[:, None]


# -- a given start: the one-class problem -------------------------------------------
def _check_state(state, info, P, n, dev):
    return _f64('state', state, (P, 2, n), dev), _f64('info', info, (P, 4), dev)


def smo_from(K, y, U, state, info, tol=1e-3, max_iter=1_000_000, steps=SLICE):
    """`smo` entered with a given `state` (P, 2, n) = [alpha | G] and `info`
    (both advanced in place): any linear term and any feasible start, for `G =
    Q alpha + p` is all the kernel knows of them."""
    n = _check_K(K)
    P = _check_batch(y, U, n)
    _check_limits(tol, max_iter, steps)
    y, U = y.contiguous(), U.contiguous()
    state, info = _check_state(state, info, P, n, K.device)
    return _relaunch(
        lambda: smo_slice(K, y, U, state, info, tol, steps, max_iter),
        state, info, tol, max_iter)


def smo_torch_from(K, y, U, state, info, tol=1e-3, max_iter=1_000_000):
    """`smo_torch` entered with a given `state` and `info` (advanced in
    place)."""
    import torch
    n = K.shape[0]
    P = _check_batch(y, U, n)
    _check_limits(tol, max_iter)
    K = K.to(torch.float64)
    dev = K.device
    state, info = _check_state(state, info, P, n, dev)
    return _loop_torch(K, y.to(dev), U.to(dev), state, info, tol, max_iter,
                       lambda t: K.index_select(0, t))


def solve_from(K, y, U, state, info, tol, max_iter):
    """(Result, fused?) from a given start: `smo_from` for a CUDA matrix of n
    <= NMAX, `smo_torch_from` anywhere else."""
    n = K.shape[0]
    dev = K.device
    if K.is_cuda and n <= NMAX:
        return smo_from(_as_it_lies(K), y.to(dev), U.to(dev), state, info,
                        tol, max_iter), True
    return smo_torch_from(K, y, U, state, info, tol, max_iter), False


def one_class_start(K, nu, U):
    """(state (P, 2, n) = [alpha0 | G0 = K alpha0], info (P, 4) = [0, inf,
    -inf, 0]) of the one-class problems ``min 1/2 a^T K a``, ``0 <= a <= U``,
    ``sum a = nu[p] l`` over the l members (``U > 0``) of row p, where K is:
    libsvm's start on the members in index order, the first ``int(nu l)`` at
    1 and the next at the remainder.  `G0` is one `svm_decide_*` launch with
    zero intercepts on a CUDA matrix, `decide_torch` anywhere else.

    K: (n, n) float32 or float64; nu: (P,) and U: (P, n) float64 tensors."""
    import torch
    if not torch.is_tensor(K) or K.dim() != 2 or K.shape[0] != K.shape[1] \
            or K.dtype not in (torch.float32, torch.float64):
        raise TypeError('K: (n, n) float32 or float64 expected')
    n = K.shape[0]
    P = _check_batch2(U, n)
    if not torch.is_tensor(nu) or nu.dtype != torch.float64 \
            or nu.shape != (P,):
        raise TypeError(f'nu: ({P},) float64 expected')
    nu, member = nu.cpu().numpy(), (U > 0).cpu().numpy()
    if not np.all((nu > 0) & (nu <= 1)):
        raise ValueError('nu: numbers in (0, 1] expected')
    a0 = np.zeros((P, n))
    for p in range(P):
        idx = np.flatnonzero(member[p])
        total = nu[p] * len(idx)
        full = int(total)
        a0[p, idx[:full]] = 1.0
        if full < len(idx):
            a0[p, idx[full]] = total - full
    dev = K.device
    state = torch.empty((P, 2, n), dtype=torch.float64, device=dev)
    state[:, 0] = torch.from_numpy(a0).to(dev)
    zero = torch.zeros(P, dtype=torch.float64, device=dev)
    alpha0 = state[:, 0].contiguous()
    state[:, 1] = decide(K, alpha0, zero) if K.is_cuda \
        else decide_torch(K, alpha0, zero)
    return state, _info0(P, dev)


# -- 2n variables over the n samples: epsilon-SVR -----------------------------------
_module2 = STATIC['svr.hip']
#: the LDS budget of svr.hip: G and alpha of both variables of a sample
NMAX2 = NMAX // 2


def _check_batch2(U, n):
    import torch
    if not torch.is_tensor(U) or U.dtype != torch.float64 or U.dim() != 2 \
            or U.shape[1] != n or U.shape[0] < 1:
        raise TypeError(f'U: (P, {n}) float64 expected')
    return U.shape[0]


def start2(z, eps, device):
    """(state (P, 2, 2n) = [alpha = 0 | G = (eps - z, eps + z)], info (P, 4) =
    [0, inf, -inf, 0]) of a batch of epsilon-SVR problems before their first
    step: the targets `z` (P, n) and the tube widths `eps` (P,) reach the
    solver through G alone."""
    import torch
    if not torch.is_tensor(z) or z.dtype != torch.float64 or z.dim() != 2 \
            or z.shape[0] < 1 or z.shape[1] < 1:
        raise TypeError('z: (P, n) float64 expected')
    P, n = z.shape
    if not torch.is_tensor(eps) or eps.dtype != torch.float64 \
            or eps.shape != (P,):
        raise TypeError(f'eps: ({P},) float64 expected')
    if not bool(torch.isfinite(z).all()) \
            or not bool((torch.isfinite(eps) & (eps >= 0)).all()):
        raise ValueError('z: finite numbers, eps: finite numbers >= 0 expected')
    z, eps = z.to(device), eps.to(device)
    state = torch.zeros((P, 2, 2 * n), dtype=torch.float64, device=device)
    state[:, 1, :n] = eps[:, None] - z
    state[:, 1, n:] = eps[:, None] + z
    return state, _info0(P, device)


def smo2_slice(K, U, state, info, tol, steps, max_iter):
    """One launch of `svm_smo2_*`: at most `steps` steps of every problem that
    has not stopped, on `state` (P, 2, 2n) and `info` in place."""
    import torch
    n = _check_K(K)
    if n > NMAX2:
        raise ValueError(f'n = {n}: at most NMAX2 = {NMAX2} on the fused '
                         'path; see smo2_torch')
    dev = K.device
    P = _check_batch2(U, n)
    _check_limits(tol, max_iter, steps)
    if U.device != dev:
        raise ValueError('K and U must be on the same device')
    U = U.contiguous()
    state = _f64('state', state, (P, 2, 2 * n), dev)
    info = _f64('info', info, (P, 4), dev)
    with torch.cuda.device(dev):
        _module2.launch(f'svm_smo2_{suffix(K.dtype)}', P, _BLOCK, 'QiQQQdqq',
                        K.data_ptr(), n, U.data_ptr(), state.data_ptr(),
                        info.data_ptr(), float(tol), int(steps),
                        int(max_iter), stream=current_stream(dev))
    return state, info


def smo2(K, U, z, eps, tol=1e-3, max_iter=1_000_000, steps=SLICE):
    """The batch of epsilon-SVR problems solved by relaunching `svm_smo2_*`
    until every problem has stopped: one download of `info` per launch,
    nothing else.  `alpha` and `G` of the result are (P, 2n): a, then a*.

    K: (n, n) float32 or float64 CUDA tensor, n <= NMAX2, symmetric,
    contiguous along either index, 16-byte aligned (read as it lies).  U: (P,
    n) the bound of both variables of a sample; z: (P, n); eps: (P,)."""
    n = _check_K(K)
    P = _check_batch2(U, n)
    _check_limits(tol, max_iter, steps)
    U = U.contiguous()
    state, info = start2(z, eps, K.device)
    if state.shape != (P, 2, 2 * n):
        raise TypeError(f'z: ({P}, {n}) float64 expected')
    return _relaunch(
        lambda: smo2_slice(K, U, state, info, tol, steps, max_iter),
        state, info, tol, max_iter)


def smo2_torch(K, U, z, eps, tol=1e-3, max_iter=1_000_000):
    """The same rule with torch operations on any device, all problems
    advancing together: variable t has the sign +1 below n and -1 from n on,
    the bound ``U[t mod n]`` and the row ``K[t mod n]`` laid out twice."""
    import torch
    n = K.shape[0]
    P = _check_batch2(U, n)
    _check_limits(tol, max_iter)
    K = K.to(torch.float64)
    dev = K.device
    state, info = start2(z, eps, dev)
    if state.shape != (P, 2, 2 * n):
        raise TypeError(f'z: ({P}, {n}) float64 expected')
    s = torch.ones((P, 2 * n), dtype=torch.int8, device=dev)
    s[:, n:] = -1
    return _loop_torch(K, s, U.to(dev).repeat(1, 2), state, info, tol,
                       max_iter, lambda t: K.index_select(0, t % n).repeat(1, 2))


def solve2(K, U, z, eps, tol, max_iter):
    """(Result, fused?): `smo2` for a CUDA matrix of n <= NMAX2, `smo2_torch`
    anywhere else."""
    n = K.shape[0]
    if K.is_cuda and n <= NMAX2:
        return smo2(_as_it_lies(K), U.to(K.device), z, eps, tol,
                    max_iter), True
    return smo2_torch(K, U, z, eps, tol, max_iter), False
