"""Host side of tsne.h, exact t-SNE on a kernel matrix where it lies (DESIGN.md
section 38): compiles the kernels once (`FILE_UNITS['tsne']`; JIT cache of
graphdot_amd.hip.jit, IEEE arithmetic: no fast-math) and runs them on torch's
*current* stream of the matrix's device as plain launches, in stream order with
the torch operations around them.  Nothing of size n x n is written: the
calibration leaves three numbers per row, a pass over the pairs ``(parts, n, 2
d + 2)`` partial sums, and the descent downloads three numbers every
`N_ITER_CHECK` steps and synchronises nowhere else.  The ``*_torch`` functions
are the same chain through torch on any device, with the (n, n) matrix of P
stored: the restatement the kernels are compared with, and the path of CPU
tensors, of embeddings that have neither two nor three columns and of matrices
the launches decline.

With the self-similarities diag (n,), ``d2 = max(0, (diag[i] + diag[j]) - 2
K[i, j])``.  Per row the calibration gives ``beta``, ``m = min_{j != i} d2``
and ``rZ = 1 / sum_{j != i} exp(-beta (d2 - m))``; the joint probability of a
pair is ``p = max((e_ij rZ_i + e_ji rZ_j) / (2 n), eps)``, and with ``w = 1 /
(1 + |y_i - y_j|^2)`` a pass over the pairs gives per row, in the columns of F,
``A = sum p w (y_i - y_j)`` (d columns), ``R = sum w^2 (y_i - y_j)`` over the
pairs with ``w >= tau`` (d columns), ``z = sum w`` and the number of pairs
with ``w < tau``; ``tau = 2 eps n (n - 1)``."""
import contextlib
import math
from collections import namedtuple

from ...hip.source_module import FILE_UNITS, current_stream, suffix
from .._dense_host import matrix_strides

_module = FILE_UNITS['tsne']
precompile = _module.precompile
_BLOCK = 256
_WAVES = 4          # rows per workgroup of tsne_calibrate
_ROWS = 32          # rows per strip of a pass over the pairs
_TILE = 64          # columns per tile
#: most parts the columns are split into
PARTS_MOST = 64
#: the workgroups a pass should have before its columns are split no further
_WORKGROUPS = 512
#: the embedding dimensions of the fused path
DIMS = (2, 3)
EPS = 2.220446049250313e-16     # np.finfo(float).eps
#: steps and tolerance of the bisection (scikit-learn's)
N_STEPS = 100
ENTROPY_TOL = 1e-5
#: the descent (scikit-learn's `_gradient_descent` and `TSNE`)
N_ITER_CHECK = 50
EXPLORATION_ITER = 250
MOMENTA = (0.5, 0.8)
ENTRY_POINTS = tuple(
    [f'tsne_calibrate_{s}' for s in ('f32', 'f64')]
    + [f'tsne_{k}_{s}_d{d}' for k in ('forces', 'kl') for s in ('f32', 'f64')
       for d in DIMS]
    + [f'tsne_update_d{d}' for d in DIMS] + ['tsne_zq', 'tsne_look'])


def parts_for(n, parts=None):
    """Into how many parts a pass over the pairs splits the columns of an (n,
    n) matrix: enough for `_WORKGROUPS` workgroups, one part per tile of 64
    columns and `PARTS_MOST` at the most -- or `parts` where one is given.  A
    function of the shape alone."""
    if parts is not None:
        if int(parts) != parts or not 1 <= parts <= PARTS_MOST:
            raise ValueError(f'parts: an integer from 1 to {PARTS_MOST} '
                             f'expected, got {parts}')
        return int(parts)
    strips = -(-n // _ROWS)
    tiles = -(-n // _TILE)
    return max(1, min(-(-_WORKGROUPS // max(strips, 1)), tiles, PARTS_MOST))


def tau_for(n):
    """The w below which a pair's q may be the clamp: ``eps Zq <= tau``,
    since ``Zq <= n (n - 1)`` up to its rounding."""
    return 2.0 * EPS * n * (n - 1)


def _check(K, diag, tables=(), Y=None):
    """n of checked arguments, any device."""
    import torch
    if not torch.is_tensor(K) or K.dim() != 2 or K.shape[0] != K.shape[1] \
            or K.dtype not in (torch.float32, torch.float64):
        raise TypeError('K: an (n, n) float32 or float64 tensor expected')
    n = K.shape[0]
    if n < 2:
        raise ValueError(f'K: at least two samples expected, got {n}')
    for name, t in (('diag', diag),) + tuple(tables):
        if not torch.is_tensor(t) or t.dtype != torch.float64 \
                or tuple(t.shape) != (n,) or t.device != K.device:
            raise TypeError(f'{name}: ({n},) float64 on {K.device} expected')
    if Y is not None and (not torch.is_tensor(Y) or Y.dtype != torch.float64
                          or Y.dim() != 2 or Y.shape[0] != n
                          or Y.shape[1] < 1 or Y.device != K.device):
        raise TypeError(f'Y: ({n}, d) float64 on {K.device} expected')
    return n


def _declines(K, d=2):
    """Why the fused chain is not for this call (None: it is).  The
    calibration stages a row in LDS where it fits and reads the matrix again
    where it does not, so the shape sets no limit."""
    import torch
    if not K.is_cuda:
        return 'not a CUDA tensor'
    if K.dtype not in (torch.float32, torch.float64):
        return 'neither float32 nor float64'
    if d not in DIMS:
        return f'n_components not in {DIMS}'
    n = K.shape[0]
    if n > 1 and K.stride() not in ((n, 1), (1, n)):
        return 'not contiguous along one of its indices'
    return None


def _fused(K, d):
    why = _declines(K, d)
    if why is not None:
        raise TypeError(f'K: {why}; see the *_torch restatements')


# -- the calibration -------------------------------------------------------------------
def calibrate(K, diag, perplexity):
    """``(beta, m, rZ (n,) float64, steps (n,) int32, flag (1,) int32)`` on
    K's device, enqueued on torch's current stream (`tsne_calibrate_*`): per
    row the bisection for the entropy ``log(perplexity)``; `steps` is `N_STEPS`
    where it did not get within `ENTROPY_TOL`; `flag` is not zero if some d2
    is not finite before its clamp.  A row's numbers depend on that row's
    data alone."""
    import torch
    n = _check(K, diag)
    _fused(K, DIMS[0])
    dev = K.device
    with torch.cuda.device(dev):
        beta, m, rZ = (torch.empty(n, dtype=torch.float64, device=dev)
                       for _ in range(3))
        steps = torch.empty(n, dtype=torch.int32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        k_lane, k_col = matrix_strides(K)
        diag = diag.contiguous()
        _module.launch(f'tsne_calibrate_{suffix(K.dtype)}', -(-n // _WAVES),
                       _BLOCK, 'QqqqQdQQQQQ', K.data_ptr(), n, k_lane, k_col,
                       diag.data_ptr(), math.log(perplexity), beta.data_ptr(),
                       m.data_ptr(), rZ.data_ptr(), steps.data_ptr(),
                       flag.data_ptr(), stream=current_stream(dev))
    return beta, m, rZ, steps, flag


def _d2_torch(K, diag):
    """(d2 (n, n) float64 with +inf on the diagonal and for what is not
    finite, flag)"""
    import torch
    d2 = (diag[:, None] + diag[None, :]) - 2.0 * K.to(torch.float64)
    d2.diagonal().fill_(0.0)
    bad = ~torch.isfinite(d2)
    flag = bad.any().to(torch.int32).reshape(1)
    d2 = torch.where(d2 < 0.0, torch.zeros_like(d2), d2)
    d2 = torch.where(bad, torch.full_like(d2, float('inf')), d2)
    d2.diagonal().fill_(float('inf'))
    return d2, flag


def calibrate_torch(K, diag, perplexity):
    """The same five tensors by torch on any device: all rows advance
    together, one (n, n) pass per step of the bisection."""
    import torch
    n = _check(K, diag)
    d2, flag = _d2_torch(K, diag)
    inf = float('inf')
    m = d2.min(dim=1).values
    r = d2 - m[:, None]
    live = torch.isfinite(r) & (r != 0.0)
    # (the terms at d2 == m are counted, not added: see tsne.h)
    c0 = (r == 0.0).sum(1).to(torch.float64)
    r = torch.where(live, r, torch.zeros_like(r))
    target = math.log(perplexity)
    beta = torch.ones_like(m)
    lo, hi = torch.full_like(m, -inf), torch.full_like(m, inf)
    steps = torch.zeros(n, dtype=torch.int32, device=K.device)
    done = torch.zeros(n, dtype=torch.bool, device=K.device)
    Z = torch.ones_like(m)
    for _ in range(N_STEPS):
        e = torch.where(live, torch.exp(-beta[:, None] * r),
                        torch.zeros_like(r))
        Zn = c0 + e.sum(1)
        H = torch.log(Zn) + beta * (r * e).sum(1) / Zn
        Z = torch.where(done, Z, Zn)
        diff = H - target
        done = done | (diff.abs() <= ENTROPY_TOL)
        steps = steps + (~done).to(torch.int32)
        move = ~done & (steps < N_STEPS)
        if not bool(move.any()):
            break
        up = diff > 0.0
        nlo = torch.where(move & up, beta, lo)
        nhi = torch.where(move & ~up, beta, hi)
        nb = torch.where(
            up, torch.where(hi == inf, beta * 2.0, (beta + hi) / 2.0),
            torch.where(lo == -inf, beta / 2.0, (beta + lo) / 2.0))
        beta = torch.where(move, nb, beta)
        lo, hi = nlo, nhi
        done = done | (steps >= N_STEPS)
    return beta, m, 1.0 / Z, steps, flag


# -- the pass over the pairs -----------------------------------------------------------
def _pass_args(K, diag, beta, m, rZ, Y, parts):
    k_lane, k_col = matrix_strides(K)
    return ('QqqqQQQQQq', K.data_ptr(), K.shape[0], k_lane, k_col,
            diag.data_ptr(), beta.data_ptr(), m.data_ptr(), rZ.data_ptr(),
            Y.data_ptr(), parts)


def forces(K, diag, beta, m, rZ, Y, parts=None):
    """``F (parts, n, 2 d + 2)`` float64, the partial sums of the rows over
    the parts of the columns (`tsne_forces_*`; the columns of F are A, R, z
    and the number of pairs below tau).  The exaggeration is no argument: it
    scales A where the sums are used (`step`, `objective`).

    K: (n, n) float32 or float64 CUDA tensor, contiguous along one index and
    symmetric (read as it lies).  Y: (n, d) float64, d in `DIMS`."""
    import torch
    n = _check(K, diag, (('beta', beta), ('m', m), ('rZ', rZ)), Y)
    d = Y.shape[1]
    _fused(K, d)
    dev = K.device
    parts = parts_for(n, parts)
    with torch.cuda.device(dev):
        F = torch.empty((parts, n, 2 * d + 2), dtype=torch.float64,
                        device=dev)
        fmt, *args = _pass_args(K, diag.contiguous(), beta.contiguous(),
                                m.contiguous(), rZ.contiguous(),
                                Y.contiguous(), parts)
        _module.launch(f'tsne_forces_{suffix(K.dtype)}_d{d}',
                       -(-n // _ROWS) * parts, _BLOCK, fmt + 'dQ', *args,
                       tau_for(n), F.data_ptr(), stream=current_stream(dev))
    return F


def _pairs_torch(K, diag, beta, m, rZ, Y):
    """(P (n, n) with a zero diagonal, W likewise, dY (n, n, d))"""
    import torch
    n = K.shape[0]
    d2, _ = _d2_torch(K, diag)
    E = torch.exp(-beta[:, None] * (d2 - m[:, None])) * rZ[:, None]
    P = torch.clamp_min((E + E.T) / (2.0 * n), EPS)
    P.diagonal().fill_(0.0)
    dY = Y[:, None, :] - Y[None, :, :]
    W = 1.0 / (1.0 + (dY * dY).sum(2))
    W.diagonal().fill_(0.0)
    return P, W, dY


def forces_torch(K, diag, beta, m, rZ, Y, P=None):
    """The same sums by torch on any device, as one part: (1, n, 2 d + 2).
    `P`: the stored matrix of `_pairs_torch`, where the caller keeps it."""
    import torch
    n = _check(K, diag, (('beta', beta), ('m', m), ('rZ', rZ)), Y)
    if P is None:
        P, W, dY = _pairs_torch(K, diag, beta, m, rZ, Y)
    else:
        dY = Y[:, None, :] - Y[None, :, :]
        W = 1.0 / (1.0 + (dY * dY).sum(2))
        W.diagonal().fill_(0.0)
    near = W >= tau_for(n)
    A = ((P * W)[:, :, None] * dY).sum(1)
    R = (torch.where(near, W * W, torch.zeros_like(W))[:, :, None] * dY).sum(1)
    tail = (~near).sum(1).to(torch.float64) - 1.0       # (less the diagonal)
    return torch.cat((A, R, W.sum(1)[:, None], tail[:, None]), 1)[None]


# -- the step --------------------------------------------------------------------------
class State:
    """The embedding `Y` (n, d), the `update` and the `gains` of the descent,
    float64 on one device; `spare` is where the next Y is written."""

    def __init__(self, Y):
        import torch
        self.Y = Y.to(torch.float64).contiguous().clone()
        self.spare = torch.empty_like(self.Y)
        self.restart()

    def restart(self):
        import torch
        self.update = torch.zeros_like(self.Y)
        self.gains = torch.ones_like(self.Y)


def _check_F(F, Y):
    import torch
    n, d = Y.shape
    if not torch.is_tensor(F) or F.dtype != torch.float64 or F.dim() != 3 \
            or tuple(F.shape[1:]) != (n, 2 * d + 2) or F.device != Y.device \
            or not 1 <= F.shape[0] <= PARTS_MOST:
        raise TypeError(f'F: (parts, {n}, {2 * d + 2}) float64 on {Y.device} '
                        'expected')
    return F.contiguous()


def _update(F, Y, spare, update, gains, a, momentum, learning_rate,
            grad=None, g2=None):
    n, d = Y.shape
    _module.launch(f'tsne_update_d{d}', -(-n // _BLOCK), _BLOCK,
                   'QqqQQQQddddQQ', F.data_ptr(), F.shape[0], n, Y.data_ptr(),
                   spare.data_ptr(), update.data_ptr(), gains.data_ptr(), a,
                   momentum, learning_rate, tau_for(n),
                   0 if grad is None else grad.data_ptr(),
                   0 if g2 is None else g2.data_ptr(),
                   stream=current_stream(Y.device))


def step(state, F, a, momentum, learning_rate, g2=None):
    """Advance `state` by one step from the partial sums `F` of its Y
    (`tsne_update_*`): the gains, the update and the new Y.  `g2` (n,)
    float64: takes the squared norms of the rows of the gains-scaled
    gradient."""
    import torch
    if not state.Y.is_cuda or state.Y.shape[1] not in DIMS:
        raise TypeError('state: (n, 2) or (n, 3) CUDA tensors expected; see '
                        'step_torch')
    F = _check_F(F, state.Y)
    with torch.cuda.device(state.Y.device):
        _update(F, state.Y, state.spare, state.update, state.gains, float(a),
                float(momentum), float(learning_rate), g2=g2)
    state.Y, state.spare = state.spare, state.Y


def _grad_torch(F, Y, a):
    """(grad (n, d), Zq) from the partial sums: the tail pairs by a second
    (n, n) pass where a row counted any."""
    import torch
    n, d = Y.shape
    S = F[0].clone()
    for p in range(1, F.shape[0]):
        S = S + F[p]
    A, R, z, tail = S[:, :d], S[:, d:2 * d], S[:, 2 * d], S[:, 2 * d + 1]
    Zq = z.sum()
    corr = torch.zeros_like(A)
    if bool((tail > 0.0).any()):
        dY = Y[:, None, :] - Y[None, :, :]
        W = 1.0 / (1.0 + (dY * dY).sum(2))
        far = W < tau_for(n)
        far.diagonal().fill_(False)
        qw = torch.where(far, torch.clamp_min(W / Zq, EPS) * W,
                         torch.zeros_like(W))
        corr = (qw[:, :, None] * dY).sum(1)
    return 4.0 * ((a * A - R / Zq) - corr), Zq


def step_torch(state, F, a, momentum, learning_rate, g2=None):
    import torch
    F = _check_F(F, state.Y)
    grad, _ = _grad_torch(F, state.Y, a)
    inc = state.update * grad < 0.0
    gains = torch.where(inc, state.gains + 0.2, state.gains * 0.8)
    state.gains = torch.clamp_min(gains, 0.01)
    grad = state.gains * grad
    state.update = momentum * state.update - learning_rate * grad
    state.Y = state.Y + state.update
    if g2 is not None:
        g2.copy_((grad * grad).sum(1))


# -- the objective ---------------------------------------------------------------------
def _look(K, diag, beta, m, rZ, Y, F, a, flag, g2):
    """(3,) float64 on the device: the KL of Y whose partial sums are F, the
    sum of g2 and the flag word (`tsne_zq`, `tsne_kl_*`, `tsne_look`)."""
    import torch
    dev = K.device
    n, d = Y.shape
    parts = F.shape[0]
    stream = current_stream(dev)
    zq = torch.empty(1, dtype=torch.float64, device=dev)
    klp = torch.empty((parts, n), dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    _module.launch('tsne_zq', 1, _BLOCK, 'QqqiQ', F.data_ptr(), parts, n,
                   2 * d + 2, zq.data_ptr(), stream=stream)
    fmt, *args = _pass_args(K, diag, beta, m, rZ, Y, parts)
    _module.launch(f'tsne_kl_{suffix(K.dtype)}_d{d}', -(-n // _ROWS) * parts,
                   _BLOCK, fmt + 'dQQ', *args, float(a), zq.data_ptr(),
                   klp.data_ptr(), stream=stream)
    _module.launch('tsne_look', 1, _BLOCK, 'QqQqQQ', klp.data_ptr(),
                   parts * n, 0 if g2 is None else g2.data_ptr(),
                   0 if g2 is None else n, flag.data_ptr(), out.data_ptr(),
                   stream=stream)
    return out


def objective(K, diag, beta, m, rZ, Y, a, parts=None):
    """``(KL (1,), grad (n, d))`` float64 on K's device: the divergence of
    the exaggerated P from Q and its gradient with respect to Y (`forces`,
    `tsne_update_*` for the gradient alone, `_look`)."""
    import torch
    Y = Y.contiguous()
    F = forces(K, diag, beta, m, rZ, Y, parts)
    dev = K.device
    with torch.cuda.device(dev):
        grad = torch.empty_like(Y)
        _update(F, Y, Y, Y, Y, float(a), 0.0, 0.0, grad=grad)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        out = _look(K, diag.contiguous(), beta.contiguous(), m.contiguous(),
                    rZ.contiguous(), Y, F, a, flag, None)
    return out[:1], grad


def _kl_torch(P, W, a, Zq):
    import torch
    Q = torch.clamp_min(W / Zq, EPS)
    aP = a * P
    T = aP * torch.log(torch.clamp_min(aP, EPS) / Q)
    T.diagonal().fill_(0.0)
    return T.sum().reshape(1)


def objective_torch(K, diag, beta, m, rZ, Y, a):
    _check(K, diag, (('beta', beta), ('m', m), ('rZ', rZ)), Y)
    P, W, _ = _pairs_torch(K, diag, beta, m, rZ, Y)
    F = forces_torch(K, diag, beta, m, rZ, Y, P)
    grad, Zq = _grad_torch(F, Y, a)
    return _kl_torch(P, W, a, Zq), grad


# -- the descent -----------------------------------------------------------------------
Descent = namedtuple('Descent', 'Y n_iter kl looks fused stopped')


def descend(K, diag, beta, m, rZ, flag, Y0, max_iter, early_exaggeration,
            learning_rate, n_iter_without_progress, min_grad_norm,
            fused=None):
    """scikit-learn's two phases of `_gradient_descent` from `Y0`:
    `Descent(Y, n_iter, kl, looks, fused, stopped)` with the final embedding
    on K's device, the steps taken, the KL of Y at exaggeration 1, the
    downloads made, whether the HIP chain ran and why the descent ended
    early (None: it did not).  ValueError if `flag` is up; it is read with
    the first download."""
    import torch
    n = _check(K, diag, (('beta', beta), ('m', m), ('rZ', rZ)), Y0)
    d = Y0.shape[1]
    if fused is None:
        fused = _declines(K, d) is None
    elif fused:
        _fused(K, d)
    dev = K.device
    state = State(Y0)
    g2 = torch.empty(n, dtype=torch.float64, device=dev)
    P = None if fused else _pairs_torch(K, diag, beta, m, rZ, state.Y)[0]
    diag, beta, m, rZ = (t.contiguous() for t in (diag, beta, m, rZ))
    looks, stopped, it = 0, None, 0

    def look(a, Y, F, with_norm):
        """(KL, squared norm of g2) of the embedding Y whose sums are F, from
        one download."""
        nonlocal looks
        if fused:
            out = _look(K, diag, beta, m, rZ, Y, F, a, flag,
                        g2 if with_norm else None)
        else:
            W = _pairs_torch(K, diag, beta, m, rZ, Y)[1]
            Zq = _grad_torch(F, Y, a)[1]
            out = torch.cat((_kl_torch(P, W, a, Zq),
                             g2.sum().reshape(1) if with_norm
                             else torch.zeros_like(g2[:1]),
                             flag.to(torch.float64)))
        kl, sq, bad = out.cpu().tolist()
        looks += 1
        if bad != 0.0:
            raise ValueError('the kernel matrix has entries that are not '
                             'finite')
        return kl, sq

    def sums():
        if fused:
            return forces(K, diag, beta, m, rZ, state.Y)
        return forces_torch(K, diag, beta, m, rZ, state.Y, P)

    advance = step if fused else step_torch
    with torch.cuda.device(dev) if K.is_cuda else contextlib.nullcontext():
        explore = min(EXPLORATION_ITER, max_iter)
        for phase, (end, a, patience) in enumerate((
                (explore, early_exaggeration, EXPLORATION_ITER),
                (max_iter, 1.0, n_iter_without_progress))):
            if stopped is not None or it >= end:
                continue
            state.restart()
            best, best_it = float('inf'), it
            while it < end:
                check = (it + 1) % N_ITER_CHECK == 0
                # (the step writes the new Y elsewhere: the old one is whole
                # until the step after, and the look is of the old one)
                Y, F = state.Y, sums()
                advance(state, F, a, MOMENTA[phase], learning_rate,
                        g2 if check else None)
                it += 1
                if not check:
                    F = None        # (released before the next is allocated)
                    continue
                kl, sq = look(a, Y, F, True)
                F = None
                if kl < best:
                    best, best_it = kl, it - 1
                elif it - 1 - best_it > patience:
                    stopped = 'no progress'
                    break
                if math.sqrt(sq) <= min_grad_norm:
                    stopped = 'gradient norm'
                    break
        kl, _ = look(1.0, state.Y, sums(), False)
    return Descent(state.Y, it, kl, looks, fused, stopped)
