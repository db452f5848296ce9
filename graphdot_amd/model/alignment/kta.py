"""Centred kernel-target alignment on top of the kernel protocol: a
label-driven criterion for a kernel's hyperparameters that needs no model fit.

The reference has no such model; the quantity is that of Cortes, Mohri and
Rostamizadeh, "Algorithms for learning kernels based on centered alignment"
(JMLR 13, 2012).  With ``H = I - 11^T / n``, the (n, k)
target columns T (one-hot class indicators, or the regression targets),
``Tc = H T``, ``L_c = Tc Tc^T`` and ``K_c = H K H``,

    A = <K_c, L_c> / (||K_c||_F ||L_c||_F)

lies in [-1, 1], is invariant under ``K -> c K + d 11^T`` (c > 0), and its
gradient is

    dA / dtheta_p = g_p / (||K_c|| ||L_c||) - A h_p / ||K_c||^2,
    g_p = <dK_p, L_c>,  h_p = <dK_p, K_c>

(the planes enter uncentred: H is a projector).  `theta` is the kernel's
log-scale `theta` everywhere, and the gradient is the kernel's linear-scale
one times ``exp(theta)``, as in
``GaussianProcessRegressor.log_marginal_likelihood``.

On the GPU, for a kernel with `device_gram`, the matrix and the gradient
planes are adopted where the solver wrote them (float or double, its own
layout) and the sums are three launches of alignment.hip with one download of
``2 + 2 m`` doubles, nothing of size n x n written or downloaded.  Anywhere
else, and above `_align.KMAX` target columns, the same chain runs through
torch (`_align.alignment_torch`)."""
import time
import warnings
import numpy as np
from .._device_kernel import active_planes, device_call, on_device
from .._fit import multistart
from .._matrices import KernelMatrices
from . import _align

TASKS = ('auto', 'classification', 'regression')


def _torch():
    import torch
    return torch


class KernelTargetAlignment(KernelMatrices):
    """The centred alignment of a kernel with labels or regression targets,
    and the hyperparameters that maximise it.

    Parameters
    ----------
    kernel: kernel instance (``kernel(X, eval_gradient=False)``, ``theta``,
        ``bounds``, ``clone_with_theta``; the device path asks for
        ``device_gram``), or ``'precomputed'``: then `fit` and `alignment`
        take the (n, n) symmetric kernel matrix as a numpy array or a torch
        tensor (CPU or CUDA, float32 or float64; a tensor is worked on where
        it lies) and give the value only.  The kernel is never modified.
    optimizer: str, True or None
        Method for ``scipy.optimize.minimize``, which minimises ``-A`` within
        ``kernel.bounds``; True means L-BFGS-B; None: `fit` evaluates the
        alignment at the kernel's own theta.
    n_restarts_optimizer: int
        Further starts from ``theta + randn(n_theta)``, clipped to the bounds.
    task: 'auto', 'classification' or 'regression'
        Under 'auto' a numpy array of a float type, (n,) or (n, k), holds
        regression targets, and anything else labels (any hashable values).
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (host path).
    device: 'auto', 'cuda', 'cpu': where the matrix lies and the sums run.

    After `fit`: `alignment_`, `theta_`, `kernel_` (``kernel.
    clone_with_theta(theta_)``; None for a precomputed matrix), `task_`,
    `classes_` (classification: a list in the order of first appearance),
    `optimization_result` (with an optimizer),
    `last_timing`."""

    def __init__(self, kernel, optimizer=None, n_restarts_optimizer=0,
                 task='auto', kernel_options=None, device='auto'):
        if task not in TASKS:
            raise ValueError(f'task: one of {TASKS} expected, got {task!r}')
        if int(n_restarts_optimizer) != n_restarts_optimizer \
                or n_restarts_optimizer < 0:
            raise ValueError('n_restarts_optimizer: a non-negative integer '
                             f'expected, got {n_restarts_optimizer}')
        self.kernel = kernel
        self.optimizer = 'L-BFGS-B' if optimizer is True else optimizer
        self.n_restarts_optimizer = int(n_restarts_optimizer)
        self.task = task
        self.kernel_options = dict(kernel_options or {})
        self.device = device
        if self._precomputed and self.optimizer:
            raise ValueError("kernel='precomputed' has no hyperparameters: "
                             'optimizer must be None')

    # -- targets -------------------------------------------------------------------
    def _task_of(self, y):
        if self.task != 'auto':
            return self.task
        return 'regression' if isinstance(y, np.ndarray) \
            and y.dtype.kind == 'f' else 'classification'

    def _targets(self, y):
        """(task, classes or None, Tc (n, k) float64, ||L_c||_F) of the
        labels or regression targets `y`."""
        task = self._task_of(y)
        if task == 'regression':
            T = np.array(y, dtype=np.float64)
            if T.ndim == 1:
                T = T[:, None]
            if T.ndim != 2 or T.shape[1] < 1:
                raise ValueError('y: (n,) or (n, k) regression targets '
                                 f'expected, got the shape {T.shape}')
            if not np.all(np.isfinite(T)):
                raise ValueError('KernelTargetAlignment: the regression '
                                 'targets have entries that are not finite')
            classes = None
        else:
            if isinstance(y, np.ndarray) and y.ndim != 1:
                raise ValueError('y: a 1-D sequence of labels expected, got '
                                 f'the shape {y.shape}')
            labels = y.tolist() if isinstance(y, np.ndarray) else list(y)
            # (in the order of their first appearance: labels need no order,
            # and the alignment does not depend on theirs)
            classes = list(dict.fromkeys(labels))
            if len(classes) < 2:
                raise ValueError('KernelTargetAlignment: at least two '
                                 f'distinct labels expected, got {classes}')
            code = {c: k for k, c in enumerate(classes)}
            T = np.zeros((len(labels), len(classes)))
            T[np.arange(len(labels)), [code[v] for v in labels]] = 1.0
        if len(T) < 2:
            raise ValueError('KernelTargetAlignment: at least two samples '
                             f'expected, got {len(T)}')
        Tc = np.ascontiguousarray(T - T.mean(0))
        # ||Tc Tc^T||_F = ||Tc^T Tc||_F: a k x k product
        return task, classes, Tc, float(np.linalg.norm(Tc.T @ Tc))

    # -- the matrix and the planes ---------------------------------------------------
    def _inputs(self, kernel, X, jac):
        """(K, planes, plane indices, adopted?) as tensors where the algebra
        runs."""
        torch = _torch()
        none = np.zeros(0, dtype=np.int64)
        if self._precomputed:
            K = self._given(X, (None, None))
            if K.shape[0] != K.shape[1]:
                raise ValueError('precomputed: a square matrix expected, got '
                                 f'{tuple(K.shape)}')
            return K, None, none, False
        la = self._dense()
        if on_device(la, self.kernel_options):
            out = device_call(kernel, 'device_gram', X, eval_gradient=jac)
            if out is not None:
                # adopted where the solver wrote them, in its arithmetic and
                # layout; valid until the next evaluation on that backend.
                # A graph kernel hands over all its columns, of which the
                # active ones are read
                Kd, dKd = out if jac else (out, None)
                K = torch.as_tensor(Kd, device=la.device)
                if dKd is None:
                    return K, None, none, True
                P = torch.as_tensor(dKd, device=la.device)
                return K, P, active_planes(kernel, P.shape[2]), True
        if jac:
            K, dK = kernel(X, eval_gradient=True, **self.kernel_options)
            P = la.tensor(dK)
            return la.tensor(K), P, np.arange(P.shape[2]), False
        return la.tensor(kernel(X, **self.kernel_options)), None, none, False

    def _evaluate(self, kernel, X, targets, jac):
        """(A, dA / d theta in linear scale or None)"""
        torch = _torch()
        _, _, Tc, Lnorm = targets
        t = time.perf_counter()
        K, P, planes, adopted = self._inputs(kernel, X, jac)
        if K.is_cuda:
            torch.cuda.synchronize(K.device)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        if K.shape[0] != len(Tc):
            raise ValueError(f'y: {K.shape[0]} targets expected, got '
                             f'{len(Tc)}')
        sums, fused = _align.solve(K, torch.from_numpy(Tc), P, planes)
        sums = sums.cpu().numpy()               # the one download
        m = len(planes)
        A, grad = _align.value_and_gradient(
            sums[0], sums[1], sums[2:2 + m], sums[2 + m:], Lnorm)
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'adopted': adopted, 'fused': fused}
        return A, (grad if jac else None)

    # -- the criterion ---------------------------------------------------------------
    def alignment(self, theta=None, X=None, y=None, eval_gradient=False,
                  clone_kernel=True):
        """The centred alignment of the kernel at the log-scale
        hyperparameters `theta` (None: the kernel's own) with the targets `y`
        on the graphs `X` (None: those of `fit`), and with `eval_gradient`
        its gradient w.r.t. `theta`.  `clone_kernel=False` moves the model's
        own kernel to `theta` instead of a clone.  With a precomputed kernel
        `X` is the matrix, and only the value exists."""
        if (X is None or y is None) and not hasattr(self, '_fitted'):
            raise ValueError('KernelTargetAlignment: X and y, or fit first')
        X = self._fitted[0] if X is None else X
        targets = self._fitted[1] if y is None else self._targets(y)
        jac = eval_gradient is True
        if self._precomputed:
            if theta is not None or jac:
                raise ValueError("kernel='precomputed' has no "
                                 'hyperparameters: the value only')
            return self._evaluate(None, X, targets, False)[0]
        theta = np.array(self.kernel.theta if theta is None else theta,
                         dtype=float)
        if clone_kernel is True:
            kernel = self.kernel.clone_with_theta(theta)
        else:
            self.kernel.theta = theta
            kernel = self.kernel
        A, grad = self._evaluate(kernel, np.asarray(X), targets, jac)
        return (A, grad * np.exp(theta)) if jac else A

    def fit(self, X, y, tol=1e-5):
        """Evaluate the alignment with the targets `y` on the graphs (or the
        precomputed kernel matrix) `X`; with an optimizer, at the
        hyperparameters that maximise it (`tol`: the optimizer's
        tolerance)."""
        targets = self._targets(y)
        self.task_ = targets[0]
        if targets[1] is not None:
            self.classes_ = list(targets[1])
        elif hasattr(self, 'classes_'):
            del self.classes_
        self._fitted = (X if self._precomputed else np.asarray(X), targets)
        if self._precomputed:
            self.theta_, self.kernel_ = None, None
            self.alignment_ = self.alignment()
            return self
        x0 = np.array(self.kernel.theta, dtype=float)
        theta = x0
        if self.optimizer:
            theta = self._optimize(x0, tol)
        self.theta_ = theta
        self.kernel_ = self.kernel.clone_with_theta(theta)
        self.alignment_ = self.alignment(theta)
        return self

    def _optimize(self, x0, tol):
        """The best of the minimisations of ``-A`` from `x0` and the extra
        starts; `x0` itself where none of them got above its alignment."""
        bounds = np.asarray(self.kernel.bounds, dtype=float)
        first = []

        def objective(t):
            A, grad = self.alignment(t, eval_gradient=True)
            first.append(A)
            return -A, -grad

        def starts():
            yield x0
            for _ in range(self.n_restarts_optimizer):
                yield np.clip(x0 + np.random.randn(len(x0)), bounds[:, 0],
                              bounds[:, 1])
        best = multistart(objective, starts(), self.optimizer, bounds, tol)
        #: the optimiser's report (scipy OptimizeResult: nit, nfev, fun)
        self.optimization_result = best
        if not best.success:
            warnings.warn('KernelTargetAlignment: the optimizer stopped '
                          f'without converging: {best.message}', UserWarning)
        # (the first evaluation of the first start is at x0)
        if not -best.fun >= first[0]:
            return x0
        return np.array(best.x, dtype=float)

    def score(self, X, y):
        """The alignment of the fitted `kernel_` with the targets `y` on the
        graphs `X` (with a precomputed kernel: of the matrix `X`)."""
        if not hasattr(self, '_fitted'):
            raise ValueError('KernelTargetAlignment: score before fit')
        if self._precomputed:
            return self.alignment(X=X, y=y)
        return self.alignment(self.theta_, X=X, y=y)
