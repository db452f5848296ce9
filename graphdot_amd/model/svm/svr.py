"""Support vector regression and novelty detection on top of the kernel
protocol.

The reference has neither; the meaning of every attribute is that of
scikit-learn's ``SVR(kernel='precomputed')`` and
``OneClassSVM(kernel='precomputed')`` (libsvm's epsilon-SVR and one-class SVM),
on the Gram matrix alone.

`KernelSVR` solves, over the 2n variables ``a_t`` and ``a*_t`` of the n
samples,

    f(a, a*) = 1/2 c^T K c + eps sum(a + a*) - z^T c,   c = a - a*
    subject to 0 <= a_t, a*_t <= C, sum(a - a*) = 0

and predicts ``sum_j c_j K(z, j) + b``.  In `cross_val_score` the problems of
every value of C, every epsilon and every fold are rows of one batch over the
one matrix, a held-out sample having the upper bound 0.  `KernelOneClassSVM`
solves ``min 1/2 a^T K a`` subject to ``0 <= a <= 1``, ``sum a = nu n`` from
libsvm's start, and decides by ``sum_j a_j K(z, j) - rho``.

On the GPU, for a kernel with `device_gram`, the matrix is adopted where the
solver wrote it and the batch is solved by svr.hip (the one-class problem by
smo.hip), a workgroup per problem, nothing of size n x n written or
downloaded; decision values are one launch on the `device_cross_gram` matrix.
Anywhere else, and above `_smo.NMAX2` (one-class: `_smo.NMAX`) samples, the
same rule runs through torch."""
import time
import warnings
import numpy as np
from .._matrices import KernelMatrices
from . import _smo
from .svc import KernelSVC


def _torch():
    import torch
    return torch


class _Machine(KernelMatrices):
    """What the two models share: the parameters of the solver, the checks
    around a solve and the decision sums."""

    def _configure(self, kernel, tol, max_iter, kernel_options, device):
        if not tol > 0:
            raise ValueError(f'tol: a positive number expected, got {tol}')
        if int(max_iter) != max_iter or max_iter < 1:
            raise ValueError('max_iter: a positive integer expected, got '
                             f'{max_iter}')
        self.kernel = kernel
        self.tol = float(tol)
        self.max_iter = int(max_iter)
        self.kernel_options = dict(kernel_options or {})
        self.device = device

    @property
    def _name(self):
        return type(self).__name__

    def _timed_gram(self, X):
        """(K, adopted?, seconds)"""
        torch = _torch()
        t = time.perf_counter()
        K, adopted = self._gram(X)
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        lo, hi = torch.aminmax(K)
        if not bool(torch.isfinite(lo) & torch.isfinite(hi)):
            raise ValueError(f'{self._name}: the kernel matrix has entries '
                             'that are not finite')
        return K, adopted, time.perf_counter() - t

    def _download(self, r):
        """(alpha, G, info) of a `_smo.Result` as numpy arrays, after the
        error and the warning its `info` asks for."""
        info = r.info.cpu().numpy()
        if (info[:, 3] != 0).any():
            raise ValueError(f'{self._name}: the kernel matrix has entries '
                             'that are not finite')
        late = int((~(info[:, 1] - info[:, 2] < self.tol)).sum())
        if late:
            warnings.warn(
                f'{self._name}: {late} of {len(info)} problems had not '
                f'reached tol = {self.tol} after {self.max_iter} steps',
                UserWarning)
        return r.alpha.cpu().numpy(), r.G.cpu().numpy(), info

    def _keep(self, K, X, coef, b):
        """What the decision values need, where the matrix was."""
        torch = _torch()
        self._n = K.shape[0]
        self.X = None if self._precomputed else np.asarray(X)
        self._state = (
            torch.from_numpy(np.ascontiguousarray(coef[None])).to(K.device),
            torch.tensor([b], dtype=torch.float64, device=K.device))

    def _decisions(self, Z):
        """(b,) ``sum_j coef_j K(z, j) + intercept``."""
        if not hasattr(self, '_state'):
            raise ValueError(f'{self._name}: predict before fit')
        coef, b = self._state
        Ks = self._cross(Z, coef.device)
        fused = _smo.decide if coef.is_cuda else _smo.decide_torch
        return fused(Ks, coef, b).cpu().numpy()[0]


class KernelSVR(_Machine):
    """An epsilon support vector regressor of graphs under a kernel.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, Y=None)``; the device path asks for
        ``device_gram`` / ``device_cross_gram``), or ``'precomputed'``: then
        `fit` takes the (n, n) kernel matrix and `predict` a (b, n) cross
        matrix, as numpy arrays or torch tensors (CPU or CUDA, float32 or
        float64; a tensor is worked on where it lies).
    C: the upper bound of the dual variables, positive.
    epsilon: the half-width of the tube inside which a residual costs
        nothing, not negative.
    tol: the stopping criterion ``m - M < tol`` of libsvm.
    max_iter: most steps of a problem; `fit` warns about one that reached it.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the matrix lies and the solver runs.

    After `fit`: `dual_coef_` (n,; ``a - a*``), `intercept_`, `support_`,
    `n_iter_`, `objective_`, `gap_` (the final ``m - M``), `last_timing`."""

    def __init__(self, kernel, C=1.0, epsilon=0.1, tol=1e-3,
                 max_iter=1_000_000, kernel_options=None, device='auto'):
        if not C > 0:
            raise ValueError(f'C: a positive number expected, got {C}')
        if not epsilon >= 0:
            raise ValueError('epsilon: a number that is not negative '
                             f'expected, got {epsilon}')
        self._configure(kernel, tol, max_iter, kernel_options, device)
        self.C = float(C)
        self.epsilon = float(epsilon)

    # -- the batch -----------------------------------------------------------------
    @staticmethod
    def _targets(y, n):
        z = np.asarray(y, dtype=np.float64)
        if z.shape != (n,):
            raise ValueError(f'y: {n} targets expected, got shape {z.shape}')
        if not np.all(np.isfinite(z)):
            raise ValueError('y: finite targets expected')
        return z

    def _solve(self, K, U, z, eps):
        """(coef (P, n), intercepts, objectives, info, slices, fused?) of
        the problems `U` (P, n), `eps` (P,) with the targets `z` (n,)."""
        torch = _torch()
        P, n = U.shape
        zs = np.tile(z, (P, 1))
        r, fused = _smo.solve2(K, torch.from_numpy(U), torch.from_numpy(zs),
                               torch.from_numpy(eps), self.tol, self.max_iter)
        alpha, G, info = self._download(r)
        # KernelSVC's rule on the 2n variables: the mean of v = -s G over the
        # free ones in index order, (m + M) / 2 where there are none
        s = np.repeat(np.array([1, -1], dtype=np.int8), n)[None, :]
        b = KernelSVC._finish(s, np.tile(U, 2), alpha, G, info)[1]
        p = np.concatenate((eps[:, None] - zs, eps[:, None] + zs), axis=1)
        return alpha[:, :n] - alpha[:, n:], b, \
            0.5 * (alpha * (G + p)).sum(1), info, r.slices, fused

    # -- the model -----------------------------------------------------------------
    def fit(self, X, y):
        """Train on the graphs (or the samples of the precomputed kernel
        matrix) `X` with the real targets `y`."""
        K, adopted, t_kernel = self._timed_gram(X)
        t = time.perf_counter()
        n = K.shape[0]
        z = self._targets(y, n)
        coef, b, objective, info, slices, fused = self._solve(
            K, np.full((1, n), self.C), z, np.array([self.epsilon]))
        self.dual_coef_ = coef[0]
        self.intercept_ = float(b[0])
        self.support_ = np.flatnonzero(coef[0] != 0)
        self.n_iter_ = int(info[0, 0])
        self.objective_ = float(objective[0])
        self.gap_ = float(info[0, 1] - info[0, 2])
        self._keep(K, X, coef[0], b[0])
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'slices': slices, 'adopted': adopted,
                            'fused': fused}
        return self

    def predict(self, Z):
        """(b,) the values at the graphs `Z` (or at the rows of a
        precomputed (b, n) cross matrix)."""
        return self._decisions(Z)

    def score(self, Z, y):
        """The coefficient of determination R^2 of `predict(Z)` against `y`."""
        got = self.predict(Z)
        y = self._targets(y, len(got))
        return float(1.0 - ((y - got) ** 2).sum() / ((y - y.mean()) ** 2).sum())

    # -- all values of C and epsilon and all folds in one batch -----------------------
    def cross_val_score(self, X, y, Cs, epsilons, cv=5, random_state=0):
        """(len(Cs), len(epsilons), folds) R^2 on the held-out samples: the
        problems of every value of C, every epsilon and every fold are solved
        as one batch over the one Gram matrix of `X`, and the held-out rows
        scored with the decision sums on that matrix.  `cv`: a number of
        folds (a shuffle drawn from `random_state`, dealt out in turn), or a
        list of (train, test) index arrays.  The model's own `C` and
        `epsilon` are not used, and the model is not fitted."""
        torch = _torch()
        Cs = np.atleast_1d(np.asarray(Cs, dtype=np.float64))
        if Cs.ndim != 1 or not len(Cs) or not np.all(Cs > 0):
            raise ValueError('Cs: positive numbers expected')
        es = np.atleast_1d(np.asarray(epsilons, dtype=np.float64))
        if es.ndim != 1 or not len(es) or not np.all(es >= 0):
            raise ValueError('epsilons: numbers that are not negative expected')
        K, adopted, t_kernel = self._timed_gram(X)
        t = time.perf_counter()
        n = K.shape[0]
        z = self._targets(y, n)
        # (one class: the whole set shuffled once and dealt out in turn)
        folds = KernelSVC._folds(np.zeros(n, dtype=np.int64), cv, random_state)
        member = np.zeros((len(folds), n), dtype=bool)
        held = np.zeros((len(folds), n), dtype=bool)
        for f, (train, test) in enumerate(folds):
            member[f, train] = True
            held[f, test] = True
            if (member[f] & held[f]).any():
                raise ValueError(f'cv: fold {f} tests on samples it trains on')
        shape = (len(Cs), len(es), len(folds))
        U = np.array(np.broadcast_to(
            Cs[:, None, None, None] * member[None, None], shape + (n,)))
        eps = np.array(np.broadcast_to(es[None, :, None], shape))
        coef, b, _, info, slices, fused = self._solve(
            K, U.reshape(-1, n), z, eps.reshape(-1))
        decide = _smo.decide if K.is_cuda else _smo.decide_torch
        D = decide(K, torch.from_numpy(np.ascontiguousarray(coef)).to(K.device),
                   torch.from_numpy(b).to(K.device)).reshape(shape + (n,))
        # R^2 of every (C, epsilon, fold) on its held-out samples, where the
        # matrix is
        test = torch.from_numpy(held).to(D.device)
        zt = torch.from_numpy(z).to(D.device)
        count = test.sum(1)
        mean = (test * zt).sum(1) / count
        total = (test * (zt[None] - mean[:, None]) ** 2).sum(1)
        rest = (test[None, None] * (zt - D) ** 2).sum(3)
        r2 = 1.0 - rest / total
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'slices': slices, 'adopted': adopted,
                            'fused': fused, 'problems': len(b),
                            'steps': int(info[:, 0].sum())}
        return r2.cpu().numpy()


class KernelOneClassSVM(_Machine):
    """A one-class support vector machine of graphs under a kernel: novelty
    detection.

    Parameters
    ----------
    kernel, tol, max_iter, kernel_options, device: as for `KernelSVR`.
    nu: in (0, 1]: an upper bound of the share of training samples outside
        the boundary and a lower bound of the share of support vectors.

    After `fit`: `dual_coef_` (n,; ``0 <= a <= 1``, ``sum a = nu n``),
    `intercept_` (``-rho``), `support_`, `n_iter_`, `objective_` (``1/2 a^T K
    a``), `gap_`, `last_timing`."""

    def __init__(self, kernel, nu=0.5, tol=1e-3, max_iter=1_000_000,
                 kernel_options=None, device='auto'):
        if not 0 < nu <= 1:
            raise ValueError(f'nu: a number in (0, 1] expected, got {nu}')
        self._configure(kernel, tol, max_iter, kernel_options, device)
        self.nu = float(nu)

    def fit(self, X, y=None):
        """Train on the graphs (or the samples of the precomputed kernel
        matrix) `X`; `y` is ignored."""
        torch = _torch()
        K, adopted, t_kernel = self._timed_gram(X)
        t = time.perf_counter()
        n = K.shape[0]
        ones = np.ones((1, n), dtype=np.int8)
        U = torch.ones((1, n), dtype=torch.float64, device=K.device)
        state, info = _smo.one_class_start(
            K, torch.tensor([self.nu], dtype=torch.float64), U)
        r, fused = _smo.solve_from(K, torch.from_numpy(ones), U, state, info,
                                   self.tol, self.max_iter)
        alpha, G, info = self._download(r)
        b = KernelSVC._finish(ones, np.ones((1, n)), alpha, G, info)[1]
        self.dual_coef_ = alpha[0]
        self.intercept_ = float(b[0])
        self.support_ = np.flatnonzero(alpha[0] != 0)
        self.n_iter_ = int(info[0, 0])
        self.objective_ = float(0.5 * (alpha[0] * G[0]).sum())
        self.gap_ = float(info[0, 1] - info[0, 2])
        self._keep(K, X, alpha[0], b[0])
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'slices': r.slices, 'adopted': adopted,
                            'fused': fused}
        return self

    def decision_function(self, Z):
        """(b,) ``sum_j a_j K(z, j) + intercept_``: positive inside."""
        return self._decisions(Z)

    def score_samples(self, Z):
        """(b,) the decision values without the intercept."""
        return self._decisions(Z) - self.intercept_

    def predict(self, Z):
        """(b,) +1 where the decision value is positive, else -1."""
        return np.where(self._decisions(Z) > 0, 1, -1)
