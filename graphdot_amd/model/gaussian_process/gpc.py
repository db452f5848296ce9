"""Binary Gaussian process classification on top of the kernel protocol.

The reference has no classifier; the meaning of every method is that of
scikit-learn's ``GaussianProcessClassifier``: Rasmussen & Williams,
"Gaussian Processes for Machine Learning", algorithms 3.1 (Newton iteration
for the mode of the Laplace approximation, logistic link), 3.2 (latent mean
and variance) and 5.1 (the approximate log marginal likelihood and its
gradient), and the five-term error-function integral of Williams & Barber
for the predictive probability:

* the objective is the approximate log marginal likelihood ``-a.f / 2 - sum
  log1p(exp(-(2y - 1) f)) - log|L_B|`` (to be maximised; `fit` minimises its
  negative), and its gradient is taken w.r.t. the log-scale hyperparameters:
  the kernel's linear-scale gradient times ``exp(theta)``, as in
  ``GaussianProcessRegressor.log_marginal_likelihood``;
* the mode search starts from ``f = 0`` (or the last mode with
  `warm_start`), stops when the objective grows by less than ``1e-10`` or
  after `max_iter_predict` steps, and returns the objective of the step
  before the one that stopped it together with the temporaries of the last
  step, as scikit-learn does;
* ``B = I + s K s`` has no eigenvalue below 1: no jitter, no pseudo-inverse.
  A NaN in the kernel matrix gives a NaN objective.

On the GPU, for a kernel with `device_gram`, a Newton step is three launches
of laplace.hip around potrf.hip's factor-and-invert with one small download,
and the gradient is one fused pass over the kernel's gradient planes where
they lie.  Anywhere else the same chain runs through torch
(`_laplace.*_torch`)."""
import time
import numpy as np
from scipy.special import erf
from .._device_kernel import (device_call, on_device, as_float64,
                              active_planes)
from ._base import GaussianProcessRegressorBase
from .gpr import _torch
from . import _laplace, _posterior

#: Williams & Barber: sigmoid(x) ~ sum_k COEFS_k (erf(LAMBDAS_k x) + 1) / 2
LAMBDAS = np.array([0.41, 0.4, 0.37, 0.44, 0.39])[:, np.newaxis]
COEFS = np.array([-1854.8214151, 3516.89893646, 221.29346712, 128.12323805,
                  -2010.49422654])[:, np.newaxis]


def _usable(label):
    return label is not None and not (isinstance(label, (float, np.floating))
                                      and np.isnan(label))


class _Mode:
    """The mode search's result: the objective `value`, and of its last step
    ``vec = [pi, s, b, g, K b]``, `Binv`, `a` and the new latent values `f`
    as tensors on the algebra's device, `steps` Newton steps."""

    def __init__(self, value, K, vec, Binv, a, f, steps):
        self.value, self.K, self.vec, self.Binv = value, K, vec, Binv
        self.a, self.f, self.steps = a, f, steps
        self.n = len(a)

    def part(self, k):
        return self.vec[k * self.n:(k + 1) * self.n]


class GaussianProcessClassifier(GaussianProcessRegressorBase):
    """Binary Gaussian process classification by the Laplace approximation
    with the logistic link.  Two classes only: multi-class one-vs-rest is
    out of scope.

    Parameters
    ----------
    kernel: kernel instance (the protocol of ``GaussianProcessRegressor``).
    optimizer: str, True, None or callable
        Method for ``scipy.optimize.minimize``; True means L-BFGS-B; None
        disables hyperparameter optimisation in ``fit``.
    max_iter_predict: int
        Most Newton steps of one mode search.
    warm_start: bool
        Start each mode search from the mode of the one before.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation.

    After `fit`: `classes_` (sorted; the second one is the positive class),
    `pi_` (the training samples' probabilities at the mode),
    `log_marginal_likelihood_value_`.  `y` reads back as 0 / 1.  The dense
    algebra runs where `device` ('auto', 'cuda', 'cpu'; an attribute) says.
    """

    def __init__(self, kernel, optimizer=None, max_iter_predict=100,
                 warm_start=False, kernel_options={}):
        super().__init__(kernel, None, optimizer, False, '+', kernel_options,
                         'auto')
        self.max_iter_predict = max_iter_predict
        self.warm_start = warm_start

    # -- labels --------------------------------------------------------------------
    @staticmethod
    def _classes(labels):
        classes = sorted(set(v for v in labels if _usable(v)))
        if len(classes) != 2:
            raise ValueError(
                'GaussianProcessClassifier is a binary classifier: two '
                f'distinct labels expected, got {len(classes)} ({classes})')
        return classes

    @staticmethod
    def _encode(labels, classes):
        """None for an unusable label, 0.0 / 1.0 for the two `classes`."""
        code = {c: float(k) for k, c in enumerate(classes)}
        labels = list(labels)
        unknown = [v for v in labels if _usable(v) and v not in code]
        if unknown:
            raise ValueError(f'labels {unknown} are not among the classes '
                             f'{classes}')
        return [code[v] if _usable(v) else None for v in labels]

    def _kept(self, X, mask):
        X = np.asarray(X)
        return X if mask.all() else X[mask]

    # -- the mode of the Laplace approximation ---------------------------------------
    def _device_inputs(self, la, kernel, X, jac):
        """(K, planes, plane indices) as device tensors straight from the
        kernel's device buffers, or None where the kernel has no device path
        (the host path then runs the same algebra through torch)."""
        if not on_device(la, self.kernel_options):
            return None
        torch = _torch()
        out = device_call(kernel, 'device_gram', X, eval_gradient=jac)
        if out is None:
            return None
        Kd, dKd = out if jac else (out, None)
        K = as_float64(Kd, la.device).contiguous()
        if dKd is None:
            return K, None, np.zeros(0, dtype=np.int64)
        # the planes as stored (float or double, the kernel's layout); a
        # graph kernel hands over all its columns, of which the active ones
        # are read
        P = torch.as_tensor(dKd, device=la.device)
        return K, P, active_planes(kernel, P.shape[2])

    def _inputs(self, la, kernel, X, jac):
        """(K, planes, plane indices, fused?)."""
        dev = self._device_inputs(la, kernel, X, jac)
        if dev is not None:
            return (*dev, la.native(dev[0]))
        if jac:
            K, dK = self._gramian(0, X, kernel=kernel, jac=True)
            P = la.tensor(dK)
            return la.tensor(K), P, np.arange(P.shape[2]), False
        return la.tensor(self._gramian(0, X, kernel=kernel)), None, \
            np.zeros(0, dtype=np.int64), False

    def _posterior_mode(self, la, K, y, fused):
        """Newton's iteration (algorithm 3.1) on tensors of the algebra's
        device.  Fused: per step `lp_solve`, `lp_apply` and the `lp_build`
        of the next step (which also sums this step's objective) behind
        potrf.hip's in-place factor-and-invert, then ONE download: the
        factorisation's head and the two sums."""
        torch = _torch()
        n = len(y)
        yt = torch.as_tensor(y, dtype=torch.float64, device=la.device)
        f0 = getattr(self, '_f_cached', None) if self.warm_start else None
        if f0 is not None and f0.shape == (n,):
            f = torch.as_tensor(f0, dtype=torch.float64, device=la.device)
        else:
            f = torch.zeros(n, dtype=torch.float64, device=la.device)
        a = torch.zeros_like(f)
        if fused:
            from . import _potrf
            build, solve, apply = (_laplace.build, _laplace.solve,
                                   _laplace.apply)
        else:
            build, solve, apply = (_laplace.build_torch,
                                   _laplace.solve_torch,
                                   _laplace.apply_torch)
        B, vec, _ = build(K, f, yt, a)
        spare = None
        value = -np.inf
        steps = 0
        last = None
        for _ in range(self.max_iter_predict):
            steps += 1
            if fused:
                # (B is scratch: the factor overwrites it, and the build
                # below writes the next step's B into the same memory)
                Binv, head, nb = _potrf.factor_inverse_(B)
            else:
                L, info = torch.linalg.cholesky_ex(B)
                Binv = torch.cholesky_inverse(L)
                logdet = 2.0 * float(torch.log(torch.diagonal(L)).sum()) \
                    if int(info) == 0 else float('nan')
            a = solve(Binv, vec)
            f = apply(K, a)
            B, vec_next, sums = build(K, f, yt, a, *(
                (B, spare) if fused else ()))
            if fused:
                logdet, sums = _potrf.logdet(
                    torch.cat((_potrf.packed_head(head, nb),
                               sums)).cpu().numpy(), nb)
            else:
                sums = sums.cpu().numpy()
            lml = -0.5 * float(sums[0]) - float(sums[1]) - 0.5 * logdet
            last = (vec, Binv, a, f)
            if lml - value < 1e-10:
                break
            value = lml
            vec, spare = vec_next, vec
        if last is None:
            raise ValueError('max_iter_predict must be at least 1')
        self._f_cached = last[3].cpu().numpy()
        return _Mode(value, K, *last, steps)

    def _gradient(self, mode, P, planes, fused):
        """d objective / d theta in linear scale: ``sum_ij M_ij P_ijk``
        (algorithm 5.1 as one contraction)."""
        u = _laplace.third_order(mode.K, mode.Binv, mode.vec)
        contract = _laplace.contract if fused else _laplace.contract_torch
        return contract(P, planes, mode.Binv, mode.part(1), mode.a, u,
                        mode.part(3)).cpu().numpy()

    def _evaluate(self, kernel, X, y, jac):
        la = self._dense()
        t = time.perf_counter()
        K, P, planes, fused = self._inputs(la, kernel, X, jac)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        mode = self._posterior_mode(la, K, y, fused)
        grad = self._gradient(mode, P, planes, fused) if jac else None
        self.last_timing = {'kernel': t_kernel,
                            'linalg': time.perf_counter() - t,
                            'newton_steps': mode.steps, 'fused': fused}
        return mode, grad

    def log_marginal_likelihood(self, theta=None, X=None, y=None,
                                eval_gradient=False, clone_kernel=True,
                                verbose=False):
        """The Laplace approximation of the log marginal likelihood at the
        log-scale hyperparameters `theta` (and its gradient w.r.t. `theta`).
        `y`: labels among `classes_` (or, before any `fit`, any two, sorted
        for this call alone: the model is left unfitted)."""
        if y is not None:
            y = list(y)
            classes = getattr(self, 'classes_', None)
            y = self._encode(y, self._classes(y) if classes is None
                             else classes)
        theta, X, y, y_mask, kernel = self._prologue(theta, X, y,
                                                     clone_kernel)
        if len(np.unique(y)) != 2:
            raise ValueError('both classes must be among the labels')
        jac = eval_gradient is True
        mode, grad = self._evaluate(kernel, self._kept(X, y_mask), y, jac)
        if jac:
            grad = grad * np.exp(theta)
        if verbose:
            t = self.last_timing
            print(f'logZ {mode.value:12.5g}  Newton steps {mode.steps:3d}  '
                  + (f'|dlogZ| {np.linalg.norm(grad):12.5g}  ' if jac else '')
                  + f't_kernel {t["kernel"]:8.2g} s  '
                  f't_linalg {t["linalg"]:8.2g} s')
        return (mode.value, grad) if jac else mode.value

    def _negative_lml(self, theta, eval_gradient=True, clone_kernel=False,
                      verbose=False):
        value, grad = self.log_marginal_likelihood(
            theta, eval_gradient=True, clone_kernel=clone_kernel,
            verbose=verbose)
        return -value, -grad

    # -- fitting ---------------------------------------------------------------------
    def fit(self, X, y, tol=1e-5, repeat=1, theta_jitter=1.0, verbose=False):
        """Train: optionally maximise the approximate log marginal
        likelihood over the hyperparameters, then find the mode and keep
        ``R = s B^-1 s`` and ``g = y - pi`` for the predictions.  `y`: two
        distinct labels of any hashable type; None / NaN are masked out."""
        y = list(y)
        self.classes_ = self._classes(y)
        self.X = X
        self.y = self._encode(y, self.classes_)
        self._f_cached = None
        if self.optimizer:
            self._optimize(self._negative_lml, 'likelihood', tol, repeat,
                           theta_jitter, verbose)
        mode, _ = self._evaluate(self.kernel,
                                 self._kept(self._X, self._y_mask), self._y,
                                 False)
        s = mode.part(1)
        R = (s[:, None] * mode.Binv * s[None, :]).contiguous()
        g = mode.part(3).contiguous()
        self.log_marginal_likelihood_value_ = mode.value
        self.pi_ = mode.part(0).cpu().numpy()
        self.R = R.cpu().numpy()
        self.g = g.cpu().numpy()
        # (the device copies ride on the algebra object, which is not saved)
        self._dense().latent_posterior = (self.R, R, g)
        return self

    # -- prediction ------------------------------------------------------------------
    def _resident(self, la):
        """(R, g) on the algebra's device: stored there by `fit`, uploaded
        once after a `load` or a change of device."""
        held = getattr(la, 'latent_posterior', None)
        if held is None or held[0] is not self.R:
            held = la.latent_posterior = (
                self.R, la.tensor(np.ascontiguousarray(self.R)),
                la.tensor(self.g))
        return held[1:]

    def latent(self, Z, return_std=False):
        """Mean ``f* = k*^T (y - pi)`` of the latent function at `Z`, and
        with `return_std` its standard deviation ``sqrt(max(0, k** - k*^T R
        k*))``: the variance is clamped at 0 on either path, as
        posterior.hip does."""
        if not hasattr(self, 'R'):
            raise RuntimeError('Model not trained.')
        torch = _torch()
        la = self._dense()
        R, g = self._resident(la)
        Xk = self._kept(self._X, self._y_mask)
        Ks = kss = None
        if on_device(la, self.kernel_options):
            Ks = device_call(self.kernel, 'device_cross_gram', Z, Xk)
            if Ks is not None and return_std is True:
                kss = device_call(self.kernel, 'device_diag', Z)
        if Ks is None or (return_std is True and kss is None):
            Ks = la.tensor(self._gramian(None, Z, Xk))
            if return_std is True:
                kss = la.tensor(self._gramian(0, Z, diag=True))
        Ks = torch.as_tensor(Ks, device=la.device)
        if return_std is not True:
            # (the mean alone does not touch R: one b x n product)
            return (Ks.to(torch.float64) @ g).cpu().numpy()
        kss = as_float64(kss, la.device)
        fused = _posterior.posterior if R.is_cuda \
            else _posterior.posterior_torch
        out = fused(R, Ks, g, kss)[0].cpu().numpy()
        b = len(out) // 2
        return out[:b], out[b:]

    def predict(self, Z):
        """The more probable of `classes_` at each of `Z`."""
        f = self.latent(Z)
        return np.where(f > 0, self.classes_[1], self.classes_[0])

    def predict_proba(self, Z):
        """(b, 2) probabilities of `classes_` at `Z`: the logistic link
        averaged over the latent Gaussian, by the five-term error-function
        integral (on the host).  With the variance v the terms are ``erf(
        lambda f* / sqrt(1 + 2 v lambda^2)) / 2``: scikit-learn's expression
        with its common factors cancelled, finite at v = 0."""
        mean, std = self.latent(Z, return_std=True)
        integrals = 0.5 * erf(LAMBDAS * mean
                              / np.sqrt(1 + 2 * std**2 * LAMBDAS**2))
        p = (COEFS * integrals).sum(axis=0) + 0.5 * COEFS.sum()
        return np.vstack((1 - p, p)).T
