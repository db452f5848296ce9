"""Gaussian process regression in the Nystrom low-rank approximation: the
behaviour of the reference's
``graphdot.model.gaussian_process.LowRankApproximateGPR``
(model/gaussian_process/nystrom.py) -- same constructor, ``C`` property,
``fit / predict / predict_loocv / log_marginal_likelihood``, masked targets
and ``normalize_y`` as in `GaussianProcessRegressor`.

The kernel matrix of N training samples is approximated through a core set of
m << N samples, ``K ~ Kxc Kcc^-1 Kxc^T = F F^T`` with ``F = Kxc R`` and
``R R^T = Kcc^-1``; nothing of size N x N is ever formed.  What differs from
the reference:

* the spectrum of F comes from a thin QR of F and the SVD of its m x m
  factor, not from ``F^T F`` (which squares the condition number);
* the likelihood gradient is one formula,
  ``sum (2 M X B) * dKxc - sum (B X^T M X B) * dKcc`` with
  ``M = Kinv - a a^T + r c^T + c r^T``, instead of a loop over the
  hyperparameters; its two contractions make one pass over each gradient
  (lowrank.hip on the GPU, through `LazyGradient.contract`);
* with a kernel that has ``device_cross_gram`` (the HIP marginalized graph
  kernel, `Normalization`, `Exponentiation`) on a GPU, every matrix stays in
  device memory and the algebra is float64 torch there; otherwise the same
  code runs on torch's CPU backend with any kernel of the protocol.
"""
import time
import warnings
import numpy as np
from scipy.optimize import minimize
from .gpr import GaussianProcessRegressor, _Dense, _torch


def _column_major(t):
    """`t` (N, M, n) with its memory as column-major planes."""
    return t.permute(2, 1, 0).contiguous().permute(2, 1, 0)


def _lazy(dK):
    from ...kernel.fix import LazyGradient
    if isinstance(dK, LazyGradient):
        return dK
    return LazyGradient(_column_major(dK))


class _LowRank:
    """``F F^T`` as ``U S^2 U^T``: U (N x r) orthonormal columns, S the
    singular values of F clamped at ``rcond * max(S)`` (the reference's
    ``lr.dot(F, rcond=beta, mode='clamp')``), from a thin QR of F and the SVD
    of the small factor."""

    def __init__(self, F, rcond):
        torch = _torch()
        Q, T = torch.linalg.qr(F)
        V, S, _ = torch.linalg.svd(T, full_matrices=False)
        self.U = Q @ V
        self.S = torch.clamp(S, min=rcond * S.max())

    def logdet(self):
        return 2.0 * self.S.log().sum()

    def inv(self, b):
        """``Kinv b`` with ``Kinv = U S^-2 U^T``."""
        Ub = self.U.T @ b
        return self.U @ (Ub / (self.S**2 if b.dim() == 1
                               else self.S[:, None]**2))

    def inv_diagonal(self):
        return ((self.U / self.S)**2).sum(1)


class LowRankApproximateGPR:
    """Gaussian process regression in the Nystrom low-rank approximation.

    Parameters
    ----------
    kernel: kernel instance (the protocol of `GaussianProcessRegressor`;
        ``device_cross_gram`` / ``device_gram`` / ``device_diag`` are used
        when present and the algebra runs on a GPU).
    alpha: float > 0
        Regularisation of the diagonal of the core matrix (and of the
        prior variance of predictions).
    beta: float > 0
        Relative cutoff of the singular values of the low-rank factor and
        of the eigenvalues of a core matrix that is not positive definite.
    optimizer: str, True, None or callable
        Method for ``scipy.optimize.minimize``; True means L-BFGS-B; None
        disables hyperparameter optimisation in ``fit``.
    normalize_y: bool
    regularization: '+', 'additive', '*' or 'multiplicative'
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation (these keep the
        evaluations on the host path).
    device: 'auto', 'cuda', 'cpu'
        Where the algebra runs.
    """

    def __init__(self, kernel, alpha=1e-7, beta=1e-7, optimizer=None,
                 normalize_y=False, regularization='+', kernel_options={},
                 device='auto'):
        self.kernel = kernel
        self.alpha = alpha
        self.beta = beta
        self.optimizer = 'L-BFGS-B' if optimizer is True else optimizer
        self.normalize_y = normalize_y
        self.regularization = regularization
        self.kernel_options = dict(kernel_options)
        self.device = device

    # -- data: as in GaussianProcessRegressor ----------------------------------
    X = GaussianProcessRegressor.X
    y = GaussianProcessRegressor.y
    mask = staticmethod(GaussianProcessRegressor.mask)
    _regularize = GaussianProcessRegressor._regularize

    @property
    def C(self):
        """The core samples that span the low-rank approximation."""
        try:
            return self._C
        except AttributeError:
            raise AttributeError(
                'Core samples do not exist. Please provide using fit().')

    @C.setter
    def C(self, C):
        self._C = C

    def _dense(self):
        if not isinstance(getattr(self, '_la', None), _Dense) \
                or self._la_device != self.device:
            self._la, self._la_device = _Dense(self.device), self.device
        return self._la

    # -- kernel evaluations: float64 tensors on the algebra's device ------------
    def _on_device(self, kernel, method):
        return (self._dense().device.type == 'cuda'
                and not self.kernel_options and hasattr(kernel, method))

    def _cross(self, kernel, X, Y, jac=False):
        """``kernel(X, Y)`` as a float64 tensor (and its gradient as a
        `LazyGradient` over the columns the kernel hands over)."""
        torch = _torch()
        la = self._dense()
        if self._on_device(kernel, 'device_cross_gram'):
            try:
                out = kernel.device_cross_gram(X, Y, eval_gradient=jac)
            except TypeError:        # not the HIP backend, or pair-sharded
                out = None
            if out is not None:
                K, dK = out if jac else (out, None)
                K = torch.as_tensor(K, device=la.device).to(torch.float64)
                if dK is not None:
                    from ...kernel.fix import LazyGradient
                    if not isinstance(dK, LazyGradient):
                        dK = LazyGradient(torch.as_tensor(dK,
                                                          device=la.device))
                return (K, dK) if jac else K
        if jac:
            K, dK = kernel(X, Y, eval_gradient=True, **self.kernel_options)
            return la.tensor(K), _lazy(la.tensor(dK))
        return la.tensor(kernel(X, Y, **self.kernel_options))

    def _core(self, kernel, C, jac=False):
        """The regularised core matrix ``kernel(C) (+ alpha)`` as a float64
        tensor of its own (and its gradient as a `LazyGradient`)."""
        torch = _torch()
        la = self._dense()
        out = None
        if self._on_device(kernel, 'device_gram'):
            try:
                out = kernel.device_gram(C, eval_gradient=jac)
            except TypeError:
                out = None
        if out is not None:
            K, dK = out if jac else (out, None)
            K = torch.as_tensor(K, device=la.device).to(torch.float64).clone()
            if dK is not None:
                # (the graph kernel's views of device_gram are only valid
                # until its next evaluation: the planes are copied, m x m x n)
                dK = _lazy(_column_major(torch.as_tensor(
                    dK, device=la.device)).clone())
            torch.cuda.current_stream(la.device).synchronize()
        elif jac:
            K, dK = kernel(C, eval_gradient=True, **self.kernel_options)
            K, dK = la.tensor(np.array(K, dtype=np.float64)), \
                _lazy(la.tensor(dK))
        else:
            K, dK = la.tensor(np.array(kernel(C, **self.kernel_options),
                                       dtype=np.float64)), None
        diag = torch.diagonal(K)
        diag.copy_(self._regularize(diag, self.alpha))
        return (K, dK) if jac else K

    def _prior_diag(self, Z):
        """``kernel.diag(Z)``, regularised, as a float64 tensor."""
        torch = _torch()
        la = self._dense()
        if self._on_device(self.kernel, 'device_diag'):
            try:
                d = self.kernel.device_diag(Z)
                return self._regularize(
                    torch.as_tensor(d, device=la.device).to(torch.float64),
                    self.alpha)
            except TypeError:
                pass
        return self._regularize(
            la.tensor(self.kernel.diag(Z, **self.kernel_options)), self.alpha)

    def _prior_gram(self, Z):
        torch = _torch()
        la = self._dense()
        if self._on_device(self.kernel, 'device_gram'):
            try:
                K = torch.as_tensor(self.kernel.device_gram(Z),
                                    device=la.device).to(torch.float64)
                K = K.clone()
                torch.cuda.current_stream(la.device).synchronize()
                diag = torch.diagonal(K)
                diag.copy_(self._regularize(diag, self.alpha))
                return K
            except TypeError:
                pass
        K = np.array(self.kernel(Z, **self.kernel_options), dtype=np.float64)
        K.flat[::len(K) + 1] = self._regularize(K.flat[::len(K) + 1],
                                                self.alpha)
        return la.tensor(K)

    # -- the low-rank algebra -----------------------------------------------------
    def _corespace(self, Kcc):
        """R with ``R R^T = Kcc^-1`` (``Q w^-1/2`` from ``eigh``); a core
        matrix that is not positive definite has its eigenvalues clamped at
        ``beta`` times the largest, with the reference's warning."""
        torch = _torch()
        w, Q = torch.linalg.eigh(Kcc)
        if not bool(torch.isfinite(w).all()):
            raise np.linalg.LinAlgError(
                'The core matrix is likely corrupted with NaNs and Infs '
                'because a pseudoinverse could not be computed.')
        if bool((w <= 0).any()):
            warnings.warn(
                'Core matrix singular, try to increase `alpha`.\n'
                'Now falling back to use a pseudoinverse.')
            w = torch.clamp(w, min=self.beta * float(w.max()))
            if bool((w <= 0).any()):
                raise np.linalg.LinAlgError(
                    'The core matrix is likely corrupted with NaNs and Infs '
                    'because a pseudoinverse could not be computed.')
        return Q * w.rsqrt(), (Q / w) @ Q.T

    # -- fitting ---------------------------------------------------------------------
    def fit(self, C, X, y, loss='likelihood', tol=1e-5, repeat=1,
            theta_jitter=1.0, verbose=False):
        """Train on (X, y) in the subspace spanned by the core set C:
        optionally optimise the hyperparameters against the likelihood
        first ('loocv' training is not available, as in the reference)."""
        self.C = C
        self.X = X
        self.y = y
        if self.optimizer:
            if loss == 'likelihood':
                objective = self.log_marginal_likelihood
            elif loss == 'loocv':
                raise NotImplementedError(
                    'LOOCV training is not available for the low-rank '
                    'regressor.')
            else:
                raise RuntimeError(f'Unknown loss function: {loss}.')
            x0 = np.array(self.kernel.theta, dtype=float)
            starts = [x0] + [x0 + theta_jitter * np.random.randn(len(x0))
                             for _ in range(repeat - 1)]
            best = None
            for x in starts:
                res = minimize(
                    fun=lambda t: objective(t, eval_gradient=True,
                                            clone_kernel=False,
                                            verbose=verbose),
                    method=self.optimizer, x0=x, bounds=self.kernel.bounds,
                    jac=True, tol=tol)
                if best is None or (res.success and res.fun < best.fun):
                    best = res
            if verbose:
                print(f'Optimization result:\n{best}')
            if not best.success:
                raise RuntimeError(
                    f'Training using the {loss} loss did not converge, got:\n'
                    f'{best}')
            self.kernel.theta = best.x
            #: the optimiser's report (scipy OptimizeResult: nit, nfev, fun)
            self.optimization_result = best
        la = self._dense()
        self.Kcc_rsqrt = self._corespace(self._core(self.kernel, self._C))[0]
        Kxc = self._cross(self.kernel, self._X, self._C)
        if not self._y_mask.all():
            Kxc = Kxc[_torch().as_tensor(self._y_mask, device=la.device)]
        self.Fxc = Kxc @ self.Kcc_rsqrt
        self._lr = _LowRank(self.Fxc, self.beta)
        self.Ky = self._lr.inv(la.tensor(self._y))
        return self

    # -- prediction --------------------------------------------------------------------
    def predict(self, Z, return_std=False, return_cov=False):
        """Mean (and standard deviation or covariance) of the predictive
        distribution at Z."""
        if not hasattr(self, 'Ky'):
            raise RuntimeError('Model not trained.')
        Fzc = self._cross(self.kernel, Z, self._C) @ self.Kcc_rsqrt
        ymean = Fzc @ (self.Fxc.T @ self.Ky)
        ymean = ymean.cpu().numpy() * self._ystd + self._ymean
        if return_std is True or return_cov is True:
            # diag / all of Kzx Kinv Kxz = (Fzc H)(Fzc H)^T
            H = self.Fxc.T @ (self._lr.U / self._lr.S)
            G = Fzc @ H
        if return_std is True:
            var = self._prior_diag(Z) - (G * G).sum(1)
            std = var.clamp(min=0).sqrt().cpu().numpy()
            return ymean, std * self._ystd
        if return_cov is True:
            cov = (self._prior_gram(Z) - G @ G.T).clamp(min=0)
            return ymean, cov.cpu().numpy() * self._ystd**2
        return ymean

    def predict_loocv(self, Z, z, return_std=False, method='auto'):
        """Leave-one-out predictions of the targets z at Z without one model
        per sample: 'ridge-like' (from the spectrum of ``Kzc^T Kzc + alpha``)
        or 'gpr-like' (from the low-rank inverse over Z); 'auto' takes the
        first when that spectrum stays above alpha."""
        assert len(Z) == len(z)
        torch = _torch()
        z = np.asarray(z, dtype=np.float64)
        if self.normalize_y is True:
            z_mean, z_std = np.mean(z), np.std(z)
            z = (z - z_mean) / z_std
        else:
            z_mean, z_std = 0, 1
        if not hasattr(self, 'Kcc_rsqrt'):
            raise RuntimeError('Model not trained.')
        la = self._dense()
        zt = la.tensor(z)
        Kzc = self._cross(self.kernel, Z, self._C)
        Cov = Kzc.T @ Kzc
        Cov.diagonal().add_(self.alpha)
        w, Q = torch.linalg.eigh(Cov)
        if bool((w <= 0).any()):
            raise np.linalg.LinAlgError(
                'Cannot raise a non-positive definite matrix to a power of '
                '-0.5.')
        if method == 'auto':
            method = 'ridge-like' if float(w.min()) > self.alpha \
                else 'gpr-like'
        if method == 'ridge-like':
            if return_std is True:
                raise NotImplementedError(
                    'LOOCV std using the ridge-like method is not ready yet.')
            P = Kzc @ (Q * w.rsqrt())
            Lz = P @ (P.T @ zt)
            zstar = zt - (zt - Lz) / (1 - (P * P).sum(1))
        elif method == 'gpr-like':
            lr = _LowRank(Kzc @ self.Kcc_rsqrt, self.beta)
            d = lr.inv_diagonal()
            zstar = zt - lr.inv(zt) / d
            if return_std is True:
                std = (1 / d.clamp(min=1e-14)).sqrt().cpu().numpy()
        else:
            raise RuntimeError(f'Unknown method {method} for predict_loocv.')
        zstar = zstar.cpu().numpy() * z_std + z_mean
        if return_std is True:
            return zstar, std * z_std
        return zstar

    # -- objective ----------------------------------------------------------------------
    def log_marginal_likelihood(self, theta=None, C=None, X=None, y=None,
                                eval_gradient=False, clone_kernel=True,
                                verbose=False):
        """``y^T K^-1 y + log|K|`` of the low-rank ``K = F F^T`` (the
        reference's convention: twice the negative log likelihood without the
        constant) at the log-scale hyperparameters `theta`, and its gradient
        w.r.t. `theta`."""
        torch = _torch()
        theta = np.array(theta if theta is not None else self.kernel.theta,
                         dtype=float)
        C = C if C is not None else self._C
        X = X if X is not None else self._X
        if y is not None:
            y_mask, y = self.mask(y)
        else:
            y, y_mask = self._y, self._y_mask
        if clone_kernel is True:
            kernel = self.kernel.clone_with_theta(theta)
        else:
            kernel = self.kernel
            kernel.theta = theta
        la = self._dense()

        t = time.perf_counter()
        out_x = self._cross(kernel, X, C, jac=eval_gradient)
        out_c = self._core(kernel, C, jac=eval_gradient)
        Kxc, dKxc = out_x if eval_gradient else (out_x, None)
        Kcc, dKcc = out_c if eval_gradient else (out_c, None)
        keep = None
        if not y_mask.all():
            keep = np.flatnonzero(y_mask)
            Kxc = Kxc.index_select(0, torch.as_tensor(keep, device=la.device))
        if la.device.type == 'cuda':
            torch.cuda.synchronize(la.device)
        t_kernel = time.perf_counter() - t

        t = time.perf_counter()
        yt = la.tensor(y)
        R, B = self._corespace(Kcc)
        lr = _LowRank(Kxc @ R, self.beta)
        Uy = lr.U.T @ yt
        S2 = lr.S**2
        parts = [(Uy * Uy / S2).sum().reshape(1), lr.logdet().reshape(1)]
        if eval_gradient is True:
            # gradient = sum (2 M X B) * dKxc - sum (B X^T M X B) * dKcc with
            # M = Kinv - a a^T + r c^T + c r^T, built
            # from N x m factors without M itself
            a = lr.U @ (Uy / S2)
            c = lr.U @ (Uy / S2**2)
            r = yt - lr.U @ Uy
            XB = Kxc @ B
            MXB = (lr.inv(XB) - torch.outer(a, a @ XB)
                   + torch.outer(c, r @ XB) + torch.outer(r, c @ XB))
            G1 = 2 * MXB
            G2 = XB.T @ MXB
            G2 = 0.5 * (G2 + G2.T)
            parts.append(dKxc.contract(G1, keep) - dKcc.contract(G2))
        packed = torch.cat(parts).cpu().numpy()      # the one download
        yKy, logdet = float(packed[0]), float(packed[1])
        value = yKy + logdet
        grad = None
        if eval_gradient is True:
            d = packed[2:]
            mask = np.asarray(getattr(kernel, 'active_theta_mask',
                                      np.ones(len(d), dtype=bool)))
            if len(d) == len(mask) and len(d) != len(theta):
                d = d[mask]
            grad = d * np.exp(theta)
        t_linalg = time.perf_counter() - t
        if verbose:
            print(f'logP {value:12.5g}  y^T.K.y {yKy:12.5g}  '
                  f'log|K| {logdet:12.5g}  '
                  f'Cond(K) {float((lr.S.max() / lr.S.min())**2):12.5g}  '
                  + (f'|dlogP| {np.linalg.norm(grad):12.5g}  '
                     if grad is not None else '')
                  + f't_kernel {t_kernel:8.2g} s  t_linalg {t_linalg:8.2g} s')
        self.last_timing = {'kernel': t_kernel, 'linalg': t_linalg}
        return (value, grad) if eval_gradient is True else value
