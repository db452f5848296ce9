"""Gaussian field regression (label propagation; Zhu, Ghahramani,
Lafferty, ICML 2003) with the behaviour of the reference's
``GaussianFieldRegressor``.  The gradient of either loss is two solves with
L and one rank-structured contraction per weight block, O(N_u N n); for
``RBFOverDistance(KernelInducedDistance(k))`` with the HIP graph kernel the
weights are recomputed from the kernel blocks by field.hip and never
stored.
"""
import warnings
import numpy as np
import scipy.linalg
from .._device_kernel import device_call, as_float64, active_planes
from .._fit import multistart

_NOT_PD = ('The Graph Laplacian is not positive definite. Some'
           'weights on edges may be invalid.')


def _torch():
    import torch
    return torch


def _fused_reason(weight):
    """Why `weight` cannot take the fused device path (None: it can)."""
    from .weight import RBFOverDistance
    from ...metric import KernelInducedDistance
    from ...kernel.fix import Normalization
    from ...kernel.marginalized import MarginalizedGraphKernel
    if not isinstance(weight, RBFOverDistance):
        return 'the weight is not an RBFOverDistance'
    if weight.mopts:
        return 'the weight passes options to its metric'
    metric = weight.metric
    if not isinstance(metric, KernelInducedDistance):
        return 'the metric is not a KernelInducedDistance'
    if metric.kernel_options:
        return 'the metric passes options to its kernel'
    kernel = metric.kernel
    inner = kernel.kernel if type(kernel) is Normalization else kernel
    if not isinstance(inner, MarginalizedGraphKernel):
        return ('the kernel is neither a MarginalizedGraphKernel nor '
                'Normalization of one')
    # (the kernel's own answer, without a launch: what its device methods
    # ask before they evaluate anything)
    if device_call(inner, '_device_backend', 'the fused path') is None:
        if getattr(inner.backend, 'shards_over_ranks', lambda: False)():
            return 'the graph kernel shards its pairs over ranks'
        return 'the graph kernel is not on the HIP backend'
    return None


class _HostSolver:
    """``L^-1 b`` by a Cholesky factor, or pinv(L) with the reference's
    warning if L is not positive definite."""

    def __init__(self, L):
        try:
            self.C = np.linalg.cholesky(L)
            self.pinv = None
        except np.linalg.LinAlgError:
            self.C = None
            self.pinv = np.linalg.pinv(L)
            warnings.warn(_NOT_PD)

    def __matmul__(self, b):
        if self.pinv is not None:
            return self.pinv @ b
        return scipy.linalg.solve_triangular(
            self.C, scipy.linalg.solve_triangular(
                self.C, b, lower=True, check_finite=False),
            trans='C', lower=True, check_finite=False)


class _DeviceSolver:
    """The same on the GPU by torch (one status word read back)."""

    def __init__(self, L):
        torch = _torch()
        C, info = torch.linalg.cholesky_ex(L)
        if int(info) == 0:
            self.C, self.pinv = C, None
        else:
            self.C, self.pinv = None, torch.linalg.pinv(L)
            warnings.warn(_NOT_PD)

    def __matmul__(self, b):
        torch = _torch()
        if self.pinv is not None:
            return self.pinv @ b
        if b.dim() == 1:
            return torch.cholesky_solve(b[:, None], self.C)[:, 0]
        return torch.cholesky_solve(b, self.C)


def _rank_contract(dW, alpha, beta, gamma):
    """``sum_{r, c} (alpha_r + beta_r gamma_c) dW[r, c, :]`` in O(Nr Nc n)."""
    return alpha @ dW.sum(axis=1) + beta @ np.einsum('rcj,c->rj', dW, gamma)


class GaussianFieldRegressor:
    """Predicts missing labels (None or NaN) from the labelled samples.

    weight: callable or 'precomputed' (X is then the weight matrix).
    optimizer: a method of ``scipy.optimize.minimize``, True (L-BFGS-B) or
    None (no hyperparameter training).  smoothing: added to every weight.
    device: 'auto' takes the fused device path where it applies
    (`_fused_reason`) and a GPU is visible, else the host path; 'cuda'
    raises TypeError where it does not apply; 'cpu' is the host path.
    """

    def __init__(self, weight, optimizer=None, smoothing=1e-3, device='auto'):
        assert smoothing >= 0, "Smoothing must be no less than 0."
        if device not in ('auto', 'cuda', 'cpu'):
            raise ValueError(f"device: 'auto', 'cuda' or 'cpu', got {device!r}")
        self.weight = weight
        self.optimizer = optimizer
        if optimizer is True:
            self.optimizer = 'L-BFGS-B'
        self.smoothing = smoothing
        self.device = device

    # -- the public interface (the reference's) --------------------------------
    def fit(self, X, y, loss='loocv2', tol=1e-5, repeat=1, theta_jitter=1.0,
            verbose=False):
        """Train the weight's hyperparameters by `loss`: 'ale' (or
        'average-label-entropy'), 'loocv1' or 'loocv2'; `repeat` runs from
        theta plus normal noise of scale `theta_jitter`.  Returns self."""
        assert len(X) == len(y)
        X = np.asarray(X)
        y = np.asarray(y, dtype=float)

        if hasattr(self.weight, 'theta') and self.optimizer:
            try:
                objective = {
                    'ale': self.average_label_entropy,
                    'average-label-entropy': self.average_label_entropy,
                    'loocv1': self.loocv_error_1,
                    'loocv2': self.loocv_error_2,
                }[loss]
            except KeyError:
                raise RuntimeError(f'Unknown loss function \'{loss}\'')

            def xgen(n):
                x0 = self.weight.theta.copy()
                yield x0
                yield from x0 + theta_jitter * np.random.randn(n - 1, len(x0))

            opt = multistart(
                lambda theta: objective(X, y, theta=theta, eval_gradient=True,
                                        verbose=verbose),
                xgen(repeat), self.optimizer, self.weight.bounds, tol)
            if verbose:
                print(f'Optimization result:\n{opt}')

            if opt.success:
                self.weight.theta = opt.x
            else:
                raise RuntimeError(f'Optimizer did not converge, got:\n'
                                   f'{opt}')
        return self

    def predict(self, X, y, return_influence=False):
        """The labels `y` with the missing ones (None or NaN) filled in and,
        with `return_influence`, the influence matrix: the contribution of
        each labelled sample to each prediction."""
        assert len(X) == len(y)
        X = np.asarray(X)
        y = np.asarray(y, dtype=float)
        z = y.copy()
        if return_influence is True:
            z[~np.isfinite(y)], influence = self._predict(
                X, y, return_influence=True)
            return z, influence
        z[~np.isfinite(y)] = self._predict(X, y, return_influence=False)
        return z

    def fit_predict(self, X, y, loss='average-label-entropy', tol=1e-5,
                    repeat=1, theta_jitter=1.0, return_influence=False,
                    verbose=False):
        """`fit` and then `predict`."""
        self.fit(X, y, loss=loss, tol=tol, repeat=repeat,
                 theta_jitter=theta_jitter, verbose=verbose)
        return self.predict(X, y, return_influence=return_influence)

    def average_label_entropy(self, X, y, theta=None, eval_gradient=False,
                              verbose=False):
        """The average label entropy of the predictions (labels 0/1) and,
        with `eval_gradient`, its gradient with respect to the weight's
        hyperparameters -- multiplied by ``exp(theta)``, as in the
        reference."""
        if theta is not None:
            self.weight.theta = theta
        X = np.asarray(X)
        y = np.asarray(y, dtype=float)
        kernel = self._fused()
        eps = 1e-7
        if kernel is not None:
            return self._device_ale(kernel, X, y, eval_gradient, eps,
                                    verbose)
        if eval_gradient is True:
            f_u, solve, blocks = self._host_field(X, y, jac=True)
        else:
            f_u = self._predict(X, y)
        z = np.minimum(1 - eps, np.maximum(eps, f_u))
        loss = -np.mean(z * np.log(z) + (1 - z) * np.log(1 - z))
        if eval_gradient is not True:
            return loss
        g = -(np.log(z) - np.log(1 - z)) / len(z)
        v = solve @ g
        grad = sum(_rank_contract(dW, -v * f_u, v, gamma)
                   for dW, gamma in blocks)
        grad = grad * np.exp(self.weight.theta)
        if verbose:
            self._report('Avg.Entropy', loss, grad)
        return loss, grad

    def loocv_error(self, X, y, p=2, theta=None, eval_gradient=False,
                    verbose=False):
        """The leave-one-out error of the labelled samples in the p-norm
        and, with `eval_gradient`, its gradient with respect to the weight's
        hyperparameters (the weight's own columns, as in the reference)."""
        if theta is not None:
            self.weight.theta = theta
        X = np.asarray(X)
        y = np.asarray(y, dtype=float)
        labeled = np.isfinite(y)
        y = y[labeled]
        n = len(y)
        kernel = self._fused()
        if kernel is not None:
            return self._device_loocv(kernel, X[labeled], y, p,
                                      eval_gradient, verbose)
        if eval_gradient is True:
            W, dW = self.weight(X[labeled], eval_gradient=True)
        elif self.weight == 'precomputed':
            W = X[labeled, :][:, labeled]
        else:
            W = self.weight(X[labeled])
        W = W + self.smoothing
        D = W.sum(axis=1)
        P = (1 / D)[:, None] * W
        e = y - P @ y
        loocv_error_p = np.mean(np.abs(e)**p)
        loocv_error = loocv_error_p**(1 / p)
        if eval_gradient is not True:
            return loocv_error
        derr_de = (loocv_error_p**(1 / p - 1) * np.abs(e)**(p - 1)
                   * np.sign(e) / n)
        grad = _rank_contract(dW, derr_de / D**2 * (W @ y), -derr_de / D, y)
        if verbose:
            self._report('LOOCV Err.', loocv_error, grad)
        return loocv_error, grad

    def loocv_error_1(self, X, y, **kwargs):
        """`loocv_error` with p = 1."""
        return self.loocv_error(X, y, p=1, **kwargs)

    def loocv_error_2(self, X, y, **kwargs):
        """`loocv_error` with p = 2."""
        return self.loocv_error(X, y, p=2, **kwargs)

    @staticmethod
    def _report(name, loss, grad):
        print(f'| {name} {loss:12.5g} | Gradient {np.linalg.norm(grad):12.5g} |')

    # -- which path ---------------------------------------------------------------
    def _fused(self):
        """The graph kernel of the fused device path, or None."""
        if self.device == 'cpu':
            return None
        reason = _fused_reason(self.weight)
        if reason is None and not _torch().cuda.is_available():
            reason = 'no GPU is visible to torch'
        if reason is None:
            return self.weight.metric.kernel
        if self.device == 'cuda':
            raise TypeError(f"device='cuda' needs the fused path, but {reason}")
        return None

    # -- the host path ---------------------------------------------------------------
    def _split(self, X, y):
        labeled = np.isfinite(y)
        f_l = y[labeled]
        if len(f_l) == len(y):
            raise RuntimeError(
                'All samples are labeled, no predictions will be made.')
        return labeled, f_l

    def _predict(self, X, y, return_influence=False):
        kernel = self._fused()
        if kernel is not None:
            return self._device_predict(kernel, X, y, return_influence)
        labeled, f_l = self._split(X, y)
        if self.weight == 'precomputed':
            W_uu = X[~labeled, :][:, ~labeled] + self.smoothing
            W_ul = X[~labeled, :][:, labeled] + self.smoothing
        else:
            W_uu = self.weight(X[~labeled]) + self.smoothing
            W_ul = self.weight(X[~labeled], X[labeled]) + self.smoothing
        D = W_uu.sum(axis=1) + W_ul.sum(axis=1)
        solve = _HostSolver(np.diag(D) - W_uu)
        if return_influence is True:
            influence = solve @ W_ul
            return influence @ f_l, influence
        return solve @ (W_ul @ f_l)

    def _host_field(self, X, y, jac):
        """f_u, the solver of L and the gradient blocks (dW, gamma)."""
        labeled, f_l = self._split(X, y)
        W_uu, dW_uu = self.weight(X[~labeled], eval_gradient=True)
        W_ul, dW_ul = self.weight(X[~labeled], X[labeled], eval_gradient=True)
        W_uu = W_uu + self.smoothing
        W_ul = W_ul + self.smoothing
        D = W_uu.sum(axis=1) + W_ul.sum(axis=1)
        solve = _HostSolver(np.diag(D) - W_uu)
        f_u = solve @ (W_ul @ f_l)
        return f_u, solve, ((dW_uu, f_u), (dW_ul, f_l))

    # -- the fused device path ---------------------------------------------------------
    def _self_block(self, kernel, X, jac):
        """X against itself by ``device_gram``; self-similarities from its
        diagonal, as in ``KernelInducedDistance(X)``."""
        torch = _torch()
        out = kernel.device_gram(list(X), eval_gradient=jac)
        K, dK = out if jac else (out, None)
        K = torch.as_tensor(K, device='cuda')
        kd = K.diagonal().to(torch.float64)
        b = dict(K=K, kr=kd, kc=kd, self_block=True)
        if jac:
            P = torch.as_tensor(dK, device='cuda')
            planes = active_planes(kernel, P.shape[2])
            idx = torch.as_tensor(planes, device='cuda')
            dkd = P.diagonal(dim1=0, dim2=1).T.index_select(1, idx).to(
                torch.float64)
            b.update(P=P, planes=planes, dkr=dkd, dkc=dkd)
        return b

    def _cross_block(self, kernel, X, Y, jac):
        """X against Y by ``device_cross_gram`` and ``device_diag``."""
        torch = _torch()
        from ...kernel.fix import LazyGradient
        X, Y = list(X), list(Y)
        out = kernel.device_cross_gram(X, Y, eval_gradient=jac)
        K, dK = out if jac else (out, None)
        dx = kernel.device_diag(X, eval_gradient=jac)
        dy = kernel.device_diag(Y, eval_gradient=jac)
        (kx, dkx), (ky, dky) = (dx, dy) if jac else ((dx, None), (dy, None))
        K = torch.as_tensor(K, device='cuda')
        b = dict(K=K, self_block=False,
                 kr=as_float64(kx, 'cuda'), kc=as_float64(ky, 'cuda'))
        if not jac:
            return b
        lazy = isinstance(dK, LazyGradient)
        P = dK.planes if lazy else torch.as_tensor(dK, device='cuda')
        planes = active_planes(kernel, P.shape[2])
        idx = torch.as_tensor(planes, device='cuda')

        def cols(a):
            return torch.as_tensor(a, device='cuda').index_select(
                1, idx).to(torch.float64)
        b.update(P=P, planes=planes, dkr=cols(dkx), dkc=cols(dky))
        if lazy:
            # Normalization: s_i t_c P + K (u_i + v_c)
            if dK.lead is not None or dK.scale is not None \
                    or len(dK.terms) > 1 or any(
                        L.data_ptr() != K.data_ptr() for L, _, _ in dK.terms):
                raise TypeError('a gradient form the field kernels do not '
                                'take')
            b.update(row=dK.row, col=dK.col)
            for _, u, v in dK.terms:
                b.update(u=cols(u), v=cols(v))
        return b

    def _rowsums(self, b, y=None, write=False):
        from . import _field
        return _field.rowsums(b['K'], b['kr'], b['kc'], self.weight.sigma,
                              self.smoothing, b['self_block'], y=y,
                              write=write)

    def _contract(self, b, alpha, beta, gamma):
        from . import _field
        return _field.contract(
            b['K'], b['kr'], b['kc'], b['dkr'], b['dkc'], self.weight.sigma,
            alpha, beta, gamma, b['P'], b['planes'], b['self_block'],
            row=b.get('row'), col=b.get('col'), u=b.get('u'), v=b.get('v'))

    def _device_field(self, kernel, X, y, jac, return_influence=False):
        """f_u, the solver of L, the blocks, f_l and the influence matrix
        on the GPU.  ``device_gram`` goes last: its views are valid until
        the next evaluation on the backend."""
        torch = _torch()
        labeled, f_l = self._split(X, y)
        f_l = torch.as_tensor(f_l, dtype=torch.float64, device='cuda')
        ul = self._cross_block(kernel, X[~labeled], X[labeled], jac)
        uu = self._self_block(kernel, X[~labeled], jac)
        s_ul, t_ul, W_ul = self._rowsums(ul, y=f_l, write=return_influence)
        s_uu, _, L = self._rowsums(uu, write=True)
        L.neg_()
        L.diagonal().add_(s_uu + s_ul)          # diag(D) - W_uu
        solve = _DeviceSolver(L)
        del L
        if return_influence:
            influence = solve @ W_ul
            return influence @ f_l, solve, uu, ul, f_l, influence
        return solve @ t_ul, solve, uu, ul, f_l, None

    def _device_predict(self, kernel, X, y, return_influence):
        f_u, _, _, _, _, influence = self._device_field(
            kernel, X, y, False, return_influence)
        if return_influence:
            return f_u.cpu().numpy(), influence.cpu().numpy()
        return f_u.cpu().numpy()

    def _device_ale(self, kernel, X, y, jac, eps, verbose):
        torch = _torch()
        f_u, solve, uu, ul, f_l, _ = self._device_field(kernel, X, y, jac)
        z = f_u.clamp(min=eps).clamp(max=1 - eps)
        loss = -(z * z.log() + (1 - z) * (1 - z).log()).mean()
        if jac is not True:
            return float(loss)
        g = -(z.log() - (1 - z).log()) / len(z)
        v = solve @ g
        alpha = -v * f_u
        grad = self._contract(uu, alpha, v, f_u) \
            + self._contract(ul, alpha, v, f_l)
        grad = grad * torch.as_tensor(np.exp(self.weight.theta),
                                      device=grad.device)
        out = torch.cat((loss[None], grad)).cpu().numpy()
        if verbose:
            self._report('Avg.Entropy', out[0], out[1:])
        return float(out[0]), out[1:]

    def _device_loocv(self, kernel, X_l, y, p, jac, verbose):
        torch = _torch()
        n = len(y)
        ll = self._self_block(kernel, X_l, jac)
        yt = torch.as_tensor(y, dtype=torch.float64, device='cuda')
        D, Wy, _ = self._rowsums(ll, y=yt)
        e = yt - Wy / D
        loocv_error_p = (e.abs()**p).mean()
        loocv_error = loocv_error_p**(1 / p)
        if jac is not True:
            return float(loocv_error)
        derr_de = (loocv_error_p**(1 / p - 1) * e.abs()**(p - 1) * e.sign()
                   / n)
        grad = self._contract(ll, derr_de / D**2 * Wy, -derr_de / D, yt)
        out = torch.cat((loocv_error[None], grad)).cpu().numpy()
        if verbose:
            self._report('LOOCV Err.', out[0], out[1:])
        return float(out[0]), out[1:]
