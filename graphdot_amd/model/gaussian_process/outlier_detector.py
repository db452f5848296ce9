"""Gaussian process regression with one learned noise level per training
sample: the behaviour of the reference's
``graphdot.model.gaussian_process.GPROutlierDetector``
(model/gaussian_process/outlier_detector.py) -- same constructor, ``fit /
predict / log_marginal_likelihood / y_uncertainty / save / load``, same
conventions:

* ``theta_ext`` is the log-scale kernel hyperparameters followed by
  ``log sigma`` per sample; the objective is ``y^T K^-1 y + log|K|`` with
  ``K = kernel(X) + diag(sigma^2)``; its gradient is
  ``(tr(K^-1 dK_k) - a^T dK_k a) exp(theta_k)`` for the kernel and
  ``(K^-1_ii - a_i^2) 2 sigma_i^2`` for the noise, ``a = K^-1 y``;
* ``K`` is inverted as the reference's ``pinvh(K, beta, mode='clamp')``:
  eigenvalues at or below ``beta lambda_max`` are raised to it;
* ``fit`` adds the L1 penalty ``w sum(sigma)``, draws its starts in the
  reference's order and keeps the best of `repeat` L-BFGS-B runs.

What is new: the clamp is decided without an eigendecomposition where it
would change nothing (`_Inverse`: a Cholesky inverse, then two sufficient
certificates, then `eigh`), and on the GPU, for a kernel with `device_gram`,
everything after the kernel is potrf.hip's factor-and-invert and the fused
epilogue of outlier.hip, with one host synchronisation per evaluation on the
common path.  Masked targets (None / NaN) drop their rows and columns, and
`fit` without an optimizer or `verbose` without a gradient raise or print
instead of crashing."""
import time
import numpy as np
from .._device_kernel import (device_call, on_device, as_float64,
                              active_planes)
from .._fit import multistart
from ._base import GaussianProcessRegressorBase
from .gpr import _torch


class _Inverse:
    """``pinvh(Ks, beta, mode='clamp')`` and its log-determinant, by the
    cheapest route that gives the same result:

    1. Cholesky inverse of Ks (not positive definite: go to 4);
    2. certificate A: ``||Ks||_inf ||Ks^-1||_inf < 1 / beta``;
    3. certificate B: ``Ks - beta ||Ks||_inf I`` is positive definite;
    4. otherwise `eigh`, eigenvalues ``<= beta max`` raised to ``beta max``.

    A and B each prove ``lambda_min > beta lambda_max``: the clamp would
    change nothing.  `path` is 'A', 'B' or 'eigh'."""

    @staticmethod
    def clamp(Ks, beta):
        torch = _torch()
        w, Q = torch.linalg.eigh(0.5 * (Ks + Ks.T))
        if not bool(torch.isfinite(w).all()):
            raise np.linalg.LinAlgError(
                'The kernel matrix is likely corrupted with NaNs and Infs '
                'because a pseudoinverse could not be computed.')
        cut = beta * w.max()
        w = torch.where(w > cut, w, cut)
        return ((Q / w) @ Q.T).contiguous(), float(torch.log(w).sum())

    @staticmethod
    def certified(normK, normKinv, beta):
        return bool(np.isfinite(normK) and np.isfinite(normKinv)
                    and normK * normKinv < 1.0 / beta)


class GPROutlierDetector(GaussianProcessRegressorBase):
    """Gaussian process regression with per-sample noise (outlier) learning.

    Parameters
    ----------
    kernel: kernel instance (the protocol of ``GaussianProcessRegressor``).
    sigma_bounds: (float, float)
        Bounds of every sample's noise level sigma (its square is added to
        the diagonal of the kernel matrix).
    beta: float > 0
        Relative eigenvalue cutoff of the clamped pseudo-inverse.
    optimizer: str, True or callable
        Method for ``scipy.optimize.minimize``; True means L-BFGS-B.  `fit`
        needs one: the noise levels are learned.
    normalize_y: bool
        Standardise the targets for fitting, undo for predictions.
    kernel_options: dict
        Extra keyword arguments for every kernel evaluation.
    device: 'auto', 'cuda', 'cpu'
        Where the dense algebra runs.
    """

    def __init__(self, kernel, sigma_bounds=(1e-4, np.inf), beta=1e-8,
                 optimizer=True, normalize_y=False, kernel_options={},
                 device='auto'):
        super().__init__(kernel, beta, optimizer, normalize_y, '+',
                         kernel_options, device)
        self.sigma_bounds = sigma_bounds

    @property
    def y_uncertainty(self):
        """The learned uncertainty magnitude of each (kept) training
        sample."""
        try:
            return self._sigma * self._ystd
        except AttributeError:
            raise AttributeError('Uncertainty must be learned via fit().')

    def _kept(self, X, mask):
        X = np.asarray(X)
        return X if mask.all() else X[mask]

    # -- the likelihood and the inverse ------------------------------------------------
    def _device_inputs(self, la, kernel, X, jac):
        """(Ks, planes, plane indices) as device tensors straight from the
        kernel's device buffers, or None where the kernel has no device path
        (the host path then runs the same algebra through torch)."""
        if not on_device(la, self.kernel_options):
            return None
        torch = _torch()
        out = device_call(kernel, 'device_gram', X, eval_gradient=jac)
        if out is None:
            return None
        Kd, dKd = out if jac else (out, None)
        Ks = as_float64(Kd, la.device).clone(
            memory_format=torch.contiguous_format)
        if dKd is None:
            return Ks, None, np.zeros(0, dtype=np.int64)
        # the planes as stored (float or double, the kernel's layout); a
        # graph kernel hands over all its columns, of which the active ones
        # are read
        P = torch.as_tensor(dKd, device=la.device)
        return Ks, P, active_planes(kernel, P.shape[2])

    def _evaluate(self, kernel, X, y, sigma2, jac):
        """(yKy, log|Ks|, d_theta (linear scale), d_alpha, Kinv, Ks) with
        ``Ks = kernel(X) + diag(sigma2)``; records the inverse's path in
        `self.last_timing`."""
        torch = _torch()
        la = self._dense()
        t = time.perf_counter()
        dev = self._device_inputs(la, kernel, X, jac)
        if dev is not None:
            Ks, P, planes = dev
            Ks.diagonal().add_(torch.as_tensor(sigma2, device=la.device))
        elif jac:
            K, dK = self._gramian(sigma2, X, kernel=kernel, jac=True)
            Ks, P = la.tensor(K), la.tensor(dK)
            planes = np.arange(P.shape[2])
        else:
            Ks, P = la.tensor(self._gramian(sigma2, X, kernel=kernel)), None
            planes = np.zeros(0, dtype=np.int64)
        t_kernel = time.perf_counter() - t
        t = time.perf_counter()
        yt = torch.as_tensor(y, dtype=torch.float64, device=la.device)
        s2 = torch.as_tensor(sigma2, dtype=torch.float64, device=la.device)
        fused = dev is not None and la.native(Ks)
        n, nt = len(y), len(planes)
        beta = self.beta
        timing = {}

        def tick(name, since):
            timing[name] = time.perf_counter() - since

        if fused:
            from . import _outlier, _potrf

            def epi(Kinv):
                return _outlier.epilogue(Kinv, Ks, yt, s2, P, planes)
            # potrf.hip's factor-and-invert, the epilogue behind it, then
            # ONE download: status, log-determinant shares and the packed
            # epilogue
            t0 = time.perf_counter()
            Kinv, head, nb = _potrf.factor_inverse(Ks)
            blob = torch.cat((_potrf.packed_head(head, nb),
                              epi(Kinv))).cpu().numpy()
            tick('factor', t0)
            logdet, out = _potrf.logdet(blob, nb)
            path = None
            if np.isfinite(logdet):
                if _Inverse.certified(out[1], out[2], beta):
                    path = 'A'
                else:
                    t0 = time.perf_counter()
                    B = Ks.clone()
                    B.diagonal().sub_(beta * float(out[1]))
                    L = _potrf.cholesky_(B)
                    if np.isfinite(_potrf.read_head(L._gd_head, nb)[1]):
                        path = 'B'
                    tick('certificate_B', t0)
            if path is None:
                t0 = time.perf_counter()
                Kinv, logdet = _Inverse.clamp(Ks, beta)
                out = epi(Kinv).cpu().numpy()
                path = 'eigh'
                tick('eigh', t0)
        else:
            from ._outlier import epilogue_torch

            def epi(Kinv):
                return epilogue_torch(Kinv, Ks, yt, s2, P, planes)
            path = None
            L, info = torch.linalg.cholesky_ex(Ks)
            if int(info) == 0:
                Kinv = torch.cholesky_inverse(L)
                logdet = 2.0 * float(torch.log(torch.diagonal(L)).sum())
                out = epi(Kinv).cpu().numpy()
                if _Inverse.certified(out[1], out[2], beta):
                    path = 'A'
                else:
                    B = Ks - beta * float(out[1]) * torch.eye(
                        n, dtype=Ks.dtype, device=Ks.device)
                    if int(torch.linalg.cholesky_ex(B)[1]) == 0:
                        path = 'B'
            if path is None:
                Kinv, logdet = _Inverse.clamp(Ks, beta)
                out = epi(Kinv).cpu().numpy()
                path = 'eigh'
        tick('linalg', t)
        timing.update(kernel=t_kernel, path=path)
        self.last_timing = timing
        yKy = float(out[0])
        return (yKy, logdet, out[3:3 + nt], out[3 + nt:3 + nt + n], Kinv,
                Ks)

    def log_marginal_likelihood(self, theta_ext, X=None, y=None,
                                eval_gradient=False, clone_kernel=True,
                                verbose=False):
        """``y^T K^-1 y + log|K|`` at the log-scale kernel hyperparameters
        followed by ``log sigma`` per (kept) sample, and its gradient
        w.r.t. them."""
        X, y, y_mask = self._targets(X, y)
        X = self._kept(X, y_mask)
        theta_ext = np.asarray(theta_ext, dtype=float)
        nt = len(self.kernel.theta)
        if len(theta_ext) != nt + len(y):
            raise ValueError(
                f'theta_ext: {nt} kernel hyperparameters and {len(y)} noise '
                f'levels expected, got {len(theta_ext)} values')
        theta, log_sigma = theta_ext[:nt], theta_ext[nt:]
        sigma = np.exp(log_sigma)
        kernel = self._kernel_at(theta, clone_kernel)
        yKy, logdet, d_theta, d_alpha, *_ = self._evaluate(
            kernel, X, y, sigma**2, eval_gradient is True)
        value = yKy + logdet
        grad = None
        if eval_gradient is True:
            grad = np.concatenate((d_theta * np.exp(theta), d_alpha))
        if verbose:
            t = self.last_timing
            print(f'logP {value:12.5g}  y^T.K.y {yKy:12.5g}  '
                  f'log|K| {logdet:12.5g}  '
                  + (f'|dlogP| {np.linalg.norm(grad):12.5g}  '
                     if grad is not None else '')
                  + f'inverse {t["path"]:>4}  t_kernel {t["kernel"]:8.2g} s  '
                  f't_linalg {t["linalg"]:8.2g} s')
        return (value, grad) if eval_gradient is True else value

    # -- fitting and prediction ------------------------------------------------
    def fit(self, X, y, w, udist=None, tol=1e-4, repeat=1, theta_jitter=1.0,
            verbose=False):
        """Learn the kernel hyperparameters and one noise level per (kept)
        sample by minimising the likelihood plus ``w sum(sigma)``, then
        invert the kernel matrix.  Random numbers are drawn in the
        reference's order: ``udist(N)`` for the first start, then
        ``randn(repeat - 1, n_theta)`` once, then ``udist(N)`` per start."""
        if not self.optimizer:
            raise RuntimeError(
                'GPROutlierDetector.fit learns the noise level of every '
                'sample and needs an optimizer (got optimizer='
                f'{self.optimizer!r})')
        self.X = X
        self.y = y
        N = len(self._y)
        if udist is None:
            def udist(n):
                return self._ystd * np.random.lognormal(-1.0, 1.0, n)
        assert callable(udist)

        def xgen(n):
            x0 = np.array(self.kernel.theta, dtype=float)
            yield x0
            yield from x0 + theta_jitter * np.random.randn(n - 1, len(x0))

        nt = len(self.kernel.theta)
        penalty = np.concatenate((np.zeros(nt), np.full(N, float(w))))

        def objective(x):
            val, jac = self.log_marginal_likelihood(
                x, eval_gradient=True, clone_kernel=False, verbose=verbose)
            exp_x = np.exp(x)
            return val + np.abs(penalty * exp_x).sum(), jac + penalty * exp_x

        bounds = np.vstack((np.asarray(self.kernel.bounds, dtype=float),
                            np.tile(np.log(self.sigma_bounds), (N, 1))))
        opt = multistart(
            objective,
            (np.concatenate((x, np.log(udist(N)))) for x in xgen(repeat)),
            self.optimizer, bounds, tol)
        if verbose:
            print(f'Optimization result:\n{opt}')
        if not opt.success:
            raise RuntimeError(f'Training did not converge, got:\n{opt}')
        self.kernel.theta = opt.x[:nt]
        self._sigma = np.exp(opt.x[nt:])
        #: the optimiser's report (scipy OptimizeResult: nit, nfev, fun)
        self.optimization_result = opt
        Xk = self._kept(self._X, self._y_mask)
        *_, Kinv, K = self._evaluate(self.kernel, Xk, self._y, self._sigma**2,
                                     False)
        self.K = K.cpu().numpy()
        self.Kinv = Kinv.cpu().numpy()
        self.Ky = self.Kinv @ self._y
        return self

    def predict(self, Z, return_std=False, return_cov=False):
        """Predictive mean (and standard deviation or covariance) at `Z`."""
        if not hasattr(self, 'Kinv'):
            raise RuntimeError('Model not trained.')
        Xk = self._kept(self._X, self._y_mask)
        Ks = np.asarray(self._gramian(None, Z, Xk), dtype=np.float64)
        ymean = (Ks @ self.Ky) * self._ystd + self._ymean
        if return_std is True:
            Kss = self._gramian(0, Z, diag=True)
            var = Kss - np.einsum('ij,jk,ik->i', Ks, self.Kinv, Ks)
            return ymean, np.sqrt(np.maximum(0, var)) * self._ystd
        if return_cov is True:
            Kss = self._gramian(0, Z)
            cov = np.maximum(0, Kss - Ks @ (self.Kinv @ Ks.T))
            return ymean, cov * self._ystd**2
        return ymean

