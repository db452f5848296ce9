"""Support vector classification on top of the kernel protocol.

The reference has no such model; the meaning of every attribute is that of
scikit-learn's ``SVC(kernel='precomputed', decision_function_shape='ovo')``
(libsvm's C-SVC), on the Gram matrix alone.  Two classes
give one dual problem, k classes the k (k - 1) / 2 one-vs-one problems in the
order (0, 1), (0, 2), ..., (k - 2, k - 1), the lower class being +1; problem p
minimises

    f(alpha) = 1/2 sum_ij alpha_i alpha_j y_i y_j K_ij - sum_i alpha_i
    subject to 0 <= alpha_i <= U_i = C class_weight[class of i], y^T alpha = 0

with ``U_i = 0`` for the samples of the other classes, and its decision value
is ``sum_j y_j alpha_j K(z, j) + b``.  All problems -- in `cross_val_score`
those of every value of C and every fold as well -- are rows of one batch over
the one matrix.

On the GPU, for a kernel with `device_gram`, the matrix is adopted where the
solver wrote it (float or double, its own layout) and the batch is solved by
smo.hip, a workgroup per problem, nothing of size n x n written or downloaded;
decision values are one launch on the `device_cross_gram` matrix.  Anywhere
else, and above `_smo.NMAX` samples, the same rule runs through torch
(`_smo.smo_torch`, `_smo.decide_torch`)."""
import time
import warnings
import numpy as np
from .._matrices import KernelMatrices
from . import _smo


def _torch():
    import torch
    return torch


def _pairs(k):
    return np.array([(a, b) for a in range(k) for b in range(a + 1, k)],
                    dtype=np.int64).reshape(-1, 2)


def _votes(D, pairs, k):
    """(b,) class indices from the (P, b) pairwise decision values: one vote
    per pair (a positive value for the first class of the pair), the most
    votes win, the lowest class index on a tie."""
    votes = np.zeros((k, D.shape[1]), dtype=np.int64)
    for p, (a, b) in enumerate(pairs):
        first = D[p] > 0
        votes[a] += first
        votes[b] += ~first
    return votes.argmax(0)


class KernelSVC(KernelMatrices):
    """A support vector classifier of graphs under a kernel.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, Y=None)``; the device path asks for
        ``device_gram`` / ``device_cross_gram``), or ``'precomputed'``: then
        `fit` takes the (n, n) kernel matrix and `predict` a (b, n) cross
        matrix, as numpy arrays or torch tensors (CPU or CUDA, float32 or
        float64; a tensor is worked on where it lies).
    C: the upper bound of the dual variables, positive.
    tol: the stopping criterion ``m - M < tol`` of libsvm.
    class_weight: None, 'balanced' (``n / (k * count of the class)``, as in
        scikit-learn) or a dict from a label to its weight (1 where absent);
        ``U_i = C class_weight[class of i]``.
    max_iter: most steps of a problem; `fit` warns about one that reached it.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the matrix lies and the solver runs.

    After `fit`: `classes_` (sorted), `pairs_` (P, 2), `dual_coef_` (P, n;
    ``y alpha``, zero outside the pair), `intercept_` (P,), `support_`,
    `n_support_` (k,), `n_iter_`, `objective_`, `gap_` (P,; the final ``m -
    M``), `last_timing`."""

    def __init__(self, kernel, C=1.0, tol=1e-3, class_weight=None,
                 max_iter=1_000_000, kernel_options=None, device='auto'):
        if not C > 0:
            raise ValueError(f'C: a positive number expected, got {C}')
        if not tol > 0:
            raise ValueError(f'tol: a positive number expected, got {tol}')
        if int(max_iter) != max_iter or max_iter < 1:
            raise ValueError('max_iter: a positive integer expected, got '
                             f'{max_iter}')
        if not (class_weight is None or class_weight == 'balanced'
                or isinstance(class_weight, dict)):
            raise ValueError("class_weight: None, 'balanced' or a dict "
                             f'expected, got {class_weight!r}')
        self.kernel = kernel
        self.C = float(C)
        self.tol = float(tol)
        self.class_weight = class_weight
        self.max_iter = int(max_iter)
        self.kernel_options = dict(kernel_options or {})
        self.device = device

    # -- the batch -----------------------------------------------------------------
    @staticmethod
    def _encode(y, n):
        """(classes (sorted), codes (n,) int64)"""
        labels = list(y)
        if len(labels) != n:
            raise ValueError(f'y: {n} labels expected, got {len(labels)}')
        classes = sorted(set(labels))
        if len(classes) < 2:
            raise ValueError('KernelSVC: at least two distinct labels '
                             f'expected, got {classes}')
        code = {c: k for k, c in enumerate(classes)}
        return classes, np.array([code[v] for v in labels], dtype=np.int64)

    def _weights(self, classes, codes, member):
        """(k,) class weights for the samples `member` (bool (n,))."""
        k = len(classes)
        if self.class_weight is None:
            return np.ones(k)
        count = np.bincount(codes[member], minlength=k)
        if isinstance(self.class_weight, dict):
            unknown = [c for c in self.class_weight if c not in classes]
            if unknown:
                raise ValueError(f'class_weight: labels {unknown} are not '
                                 f'among the classes {classes}')
            return np.array([float(self.class_weight.get(c, 1.0))
                             for c in classes])
        return member.sum() / (k * np.maximum(count, 1).astype(np.float64))

    @staticmethod
    def _problems(codes, pairs, bound):
        """(y (P, n) int8, U (P, n)) of the class pairs for the per-sample
        bounds `bound` (n,; zero: not a member)."""
        first = codes[None, :] == pairs[:, :1]
        second = codes[None, :] == pairs[:, 1:]
        y = np.where(first, 1, -1).astype(np.int8)
        return y, np.where(first | second, bound[None, :], 0.0)

    def _solve(self, K, y, U):
        """(alpha, G, info as numpy arrays, slices, fused?)"""
        torch = _torch()
        lo, hi = torch.aminmax(K)
        if not bool(torch.isfinite(lo) & torch.isfinite(hi)):
            raise ValueError('KernelSVC: the kernel matrix has entries that '
                             'are not finite')
        r, fused = _smo.solve(K, torch.from_numpy(y), torch.from_numpy(U),
                              self.tol, self.max_iter)
        info = r.info.cpu().numpy()
        if (info[:, 3] != 0).any():
            raise ValueError('KernelSVC: the kernel matrix has entries that '
                             'are not finite')
        late = int((~(info[:, 1] - info[:, 2] < self.tol)).sum())
        if late:
            warnings.warn(
                f'KernelSVC: {late} of {len(info)} problems had not reached '
                f'tol = {self.tol} after {self.max_iter} steps', UserWarning)
        return r.alpha.cpu().numpy(), r.G.cpu().numpy(), info, r.slices, fused

    @staticmethod
    def _finish(y, U, alpha, G, info):
        """(coef = y alpha, intercept, objective): the intercept is the mean
        of ``v = -y G`` over the free samples (0 < alpha < U) in index order,
        ``(m + M) / 2`` where there are none."""
        yf = y.astype(np.float64)
        v = -yf * G
        free = (alpha > 0) & (alpha < U)
        count = free.sum(1)
        total = np.cumsum(np.where(free, v, 0.0), axis=1)[:, -1]
        b = np.where(count > 0, total / np.maximum(count, 1),
                     (info[:, 1] + info[:, 2]) / 2)
        return yf * alpha, b, 0.5 * (alpha * (G - 1.0)).sum(1)

    # -- the model -----------------------------------------------------------------
    def fit(self, X, y):
        """Train on the graphs (or the samples of the precomputed kernel
        matrix) `X` with the labels `y` (any hashable values)."""
        torch = _torch()
        t = time.perf_counter()
        K, adopted = self._gram(X)
        n = K.shape[0]
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        classes, codes = self._encode(y, n)
        k = len(classes)
        pairs = _pairs(k)
        w = self._weights(classes, codes, np.ones(n, dtype=bool))
        ys, U = self._problems(codes, pairs, self.C * w[codes])
        alpha, G, info, slices, fused = self._solve(K, ys, U)
        coef, b, objective = self._finish(ys, U, alpha, G, info)
        self.classes_ = np.asarray(classes)
        self.pairs_ = pairs
        self.dual_coef_ = coef
        self.intercept_ = b
        self.support_ = np.flatnonzero((coef != 0).any(0))
        self.n_support_ = np.bincount(codes[self.support_], minlength=k)
        self.n_iter_ = info[:, 0].astype(np.int64)
        self.objective_ = objective
        self.gap_ = info[:, 1] - info[:, 2]
        self._n = n
        self.X = None if self._precomputed else np.asarray(X)
        # what `decision_function` needs, where the matrix was
        self._state = (torch.from_numpy(coef).to(K.device),
                       torch.from_numpy(b).to(K.device))
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'slices': slices, 'adopted': adopted,
                            'fused': fused}
        return self

    def _decisions(self, Z):
        """(P, b) pairwise decision values, positive for the first class."""
        if not hasattr(self, '_state'):
            raise ValueError('KernelSVC: predict before fit')
        coef, b = self._state
        Ks = self._cross(Z, coef.device)
        fused = _smo.decide if coef.is_cuda else _smo.decide_torch
        return fused(Ks, coef, b).cpu().numpy()

    def decision_function(self, Z):
        """Pairwise decision values in the shape and sign of scikit-learn's
        ``decision_function_shape='ovo'``: (b, P), positive for the first
        class of the pair, for more than two classes; (b,), positive for
        ``classes_[1]``, for two."""
        D = self._decisions(Z)
        return -D[0] if len(self.classes_) == 2 else D.T.copy()

    def predict(self, Z):
        """(b,) the class of each of the graphs `Z` (or of the rows of a
        precomputed (b, n) cross matrix): one vote per pair, the most votes
        win, the lowest class on a tie."""
        D = self._decisions(Z)
        return self.classes_[_votes(D, self.pairs_, len(self.classes_))]

    def score(self, Z, y):
        """The accuracy of `predict(Z)` against the labels `y`."""
        got = self.predict(Z)
        y = list(y)
        if len(y) != len(got):
            raise ValueError(f'y: {len(got)} labels expected, got {len(y)}')
        return float(np.mean([g == v for g, v in zip(got.tolist(), y)]))

    # -- all values of C and all folds in one batch ----------------------------------
    @staticmethod
    def _folds(codes, cv, random_state):
        """[(train, test)] index arrays: `cv` as given, or that many
        stratified folds (each class shuffled once and dealt out in turn)."""
        n = len(codes)
        if not isinstance(cv, (int, np.integer)):
            folds = [(np.asarray(a, dtype=np.int64), np.asarray(b, np.int64))
                     for a, b in cv]
            for a, b in folds:
                if a.ndim != 1 or b.ndim != 1 or not len(a) or not len(b) \
                        or min(a.min(), b.min()) < 0 \
                        or max(a.max(), b.max()) >= n:
                    raise ValueError('cv: pairs of non-empty index arrays '
                                     f'from 0 to {n - 1} expected')
            if not folds:
                raise ValueError('cv: at least one fold expected')
            return folds
        if cv < 2:
            raise ValueError(f'cv: at least two folds expected, got {cv}')
        rng = np.random.default_rng(random_state)
        fold = np.empty(n, dtype=np.int64)
        at = 0
        for c in range(codes.max() + 1):
            idx = rng.permutation(np.flatnonzero(codes == c))
            fold[idx] = (at + np.arange(len(idx))) % cv
            at += len(idx)
        return [(np.flatnonzero(fold != f), np.flatnonzero(fold == f))
                for f in range(cv)]

    def cross_val_score(self, X, y, Cs, cv=5, random_state=0):
        """(len(Cs), folds) accuracies on the held-out samples: the problems
        of every value of C, every fold and every class pair are solved as
        one batch over the one Gram matrix of `X`, and the held-out rows
        scored with the decision sums on that matrix.  `cv`: a number of
        stratified folds drawn from `random_state`, or a list of (train,
        test) index arrays.  The model's own `C` is not used, and the model
        is not fitted."""
        torch = _torch()
        Cs = np.atleast_1d(np.asarray(Cs, dtype=np.float64))
        if Cs.ndim != 1 or not len(Cs) or not np.all(Cs > 0):
            raise ValueError('Cs: positive numbers expected')
        t = time.perf_counter()
        K, adopted = self._gram(X)
        n = K.shape[0]
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        classes, codes = self._encode(y, n)
        k = len(classes)
        pairs = _pairs(k)
        folds = self._folds(codes, cv, random_state)
        ys, Us = [], []
        held = np.zeros((len(folds), n), dtype=bool)
        for f, (train, test) in enumerate(folds):
            member = np.zeros(n, dtype=bool)
            member[train] = True
            held[f, test] = True
            if (member & held[f]).any():
                raise ValueError(f'cv: fold {f} tests on samples it trains on')
            if len(np.unique(codes[member])) != k:
                raise ValueError(f'cv: fold {f} does not train on every class')
        for C in Cs:
            for f, (train, test) in enumerate(folds):
                member = np.zeros(n, dtype=bool)
                member[train] = True
                w = self._weights(classes, codes, member)
                yp, Up = self._problems(codes, pairs,
                                        np.where(member, C * w[codes], 0.0))
                ys.append(yp)
                Us.append(Up)
        ys, U = np.concatenate(ys), np.concatenate(Us)
        alpha, G, info, slices, fused = self._solve(K, ys, U)
        coef, b, _ = self._finish(ys, U, alpha, G, info)
        decide = _smo.decide if K.is_cuda else _smo.decide_torch
        D = decide(K, torch.from_numpy(coef).to(K.device),
                   torch.from_numpy(b).to(K.device))
        # the votes of every (C, fold) on all n samples, where the matrix is
        D = D.reshape(len(Cs), len(folds), len(pairs), n)
        votes = torch.zeros((len(Cs), len(folds), k, n), dtype=torch.int64,
                            device=D.device)
        for p, (a, c) in enumerate(pairs):
            first = D[:, :, p] > 0
            votes[:, :, a] += first
            votes[:, :, c] += ~first
        right = votes.argmax(2) == torch.from_numpy(codes).to(D.device)
        test = torch.from_numpy(held).to(D.device)
        acc = (right & test[None]).sum(2) / test.sum(1)[None]
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'slices': slices, 'adopted': adopted,
                            'fused': fused, 'problems': len(ys),
                            'steps': int(info[:, 0].sum())}
        return acc.cpu().numpy()
