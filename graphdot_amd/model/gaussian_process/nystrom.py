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
from .._device_kernel import (device_call, on_device, as_float64,
                              active_planes)
from ._base import GaussianProcessRegressorBase
from .gpr import _torch


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


class LowRankApproximateGPR(GaussianProcessRegressorBase):
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
        super().__init__(kernel, beta, optimizer, normalize_y, regularization,
                         kernel_options, device)
        self.alpha = alpha

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

    # -- kernel evaluations: float64 tensors on the algebra's device ------------
    def _device(self, kernel, method, *args, **kwargs):
        """The result of the kernel's device method, or None where the
        model or the kernel has no device path."""
        if not on_device(self._dense(), self.kernel_options):
            return None
        return device_call(kernel, method, *args, **kwargs)

    def _cross(self, kernel, X, Y, jac=False):
        """``kernel(X, Y)`` as a float64 tensor (and its gradient as a
        `LazyGradient` over the columns the kernel hands over)."""
        torch = _torch()
        la = self._dense()
        out = self._device(kernel, 'device_cross_gram', X, Y,
                           eval_gradient=jac)
        if out is not None:
            K, dK = out if jac else (out, None)
            K = as_float64(K, la.device)
            if dK is not None:
                from ...kernel.fix import LazyGradient
                if not isinstance(dK, LazyGradient):
                    dK = LazyGradient(torch.as_tensor(dK, device=la.device))
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
        out = self._device(kernel, 'device_gram', C, eval_gradient=jac)
        if out is not None:
            K, dK = out if jac else (out, None)
            K = as_float64(K, la.device).clone()
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
        la = self._dense()
        d = self._device(self.kernel, 'device_diag', Z)
        if d is not None:
            return self._regularize(as_float64(d, la.device), self.alpha)
        return self._regularize(
            la.tensor(self.kernel.diag(Z, **self.kernel_options)), self.alpha)

    def _prior_gram(self, Z):
        torch = _torch()
        la = self._dense()
        K = self._device(self.kernel, 'device_gram', Z)
        if K is not None:
            K = as_float64(K, la.device).clone()
            torch.cuda.current_stream(la.device).synchronize()
            diag = torch.diagonal(K)
            diag.copy_(self._regularize(diag, self.alpha))
            return K
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
            self._optimize(objective, loss, tol, repeat, theta_jitter, verbose)
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
        theta, X, y, y_mask, kernel = self._prologue(theta, X, y,
                                                     clone_kernel)
        C = C if C is not None else self._C
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
            grad = d[active_planes(kernel, len(d))] * np.exp(theta)
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
