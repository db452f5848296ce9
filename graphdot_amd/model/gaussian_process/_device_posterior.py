"""The posterior of a fitted `GaussianProcessRegressor` kept on the device
for callers that predict a handful of candidates over and over (the tree
search of `graphdot_amd.model.tree_search`): the inverse of the training
matrix and ``Kinv y`` are uploaded once, the cross kernel stays where the
solver wrote it, and mean and standard deviation of the candidates come from
the fused kernels of posterior.hip, which stream the inverse once for all
candidates; one download of ``2 b`` numbers per call."""
import numpy as np

from .._device_kernel import device_call, on_device
from .gpr import GaussianProcessRegressor, _torch
from . import _posterior


class DevicePosterior:
    """``DevicePosterior(gpr).predict(Z, return_std, return_cov)`` returns
    what ``gpr.predict`` returns.

    `available` says whether the device path applies: the regressor's dense
    algebra is on a CUDA device, it has no `kernel_options`, and its kernel
    offers `device_cross_gram` and a `device_diag` that does not raise
    `NoDevicePath` (the HIP backend, not sharded over ranks).  Otherwise
    `predict` is `gpr.predict`.  After a refit of `gpr` the device copies are
    rebuilt on the next call."""

    def __init__(self, gpr):
        if not isinstance(gpr, GaussianProcessRegressor):
            raise TypeError('DevicePosterior wraps a GaussianProcessRegressor')
        if not hasattr(gpr, 'Kinv'):
            raise RuntimeError('Model not trained.')
        self.gpr = gpr
        self._refresh()

    def _refresh(self):
        gpr = self.gpr
        la = gpr._dense()
        self._fitted = gpr.Kinv         # identity: a refit makes a new array
        self.Kinv = la.tensor(np.ascontiguousarray(gpr.Kinv))
        self.Ky = la.tensor(gpr.Ky)
        #: the training samples with a usable target
        self.X = gpr._X[gpr._y_mask]
        self.available = self._probe(la)

    def _probe(self, la):
        kernel = self.gpr.kernel
        if not on_device(la, self.gpr.kernel_options) \
                or not hasattr(kernel, 'device_cross_gram'):
            return False
        # (one graph's self-similarity: a launch, the answer of the backend)
        return device_call(kernel, 'device_diag', self.X[:1]) is not None

    def _current(self):
        if self.gpr.Kinv is not self._fitted:
            self._refresh()

    # -- the algebra: tensors on any device ----------------------------------
    def _moments(self, Ks, kss, want_T=False):
        fused = _posterior.posterior if self.Kinv.is_cuda \
            else _posterior.posterior_torch
        return fused(self.Kinv, Ks, self.Ky, kss, self.gpr._ymean,
                     self.gpr._ystd, return_T=want_T)

    def _predict_from(self, Ks, kss=None, Kss=None):
        """`predict` from kernel matrices that are tensors on the algebra's
        device already: ``Ks = kernel(Z, X)`` (b, n) in float or double and,
        for the standard deviation, the unregularised ``kss = diag(Z)``, or,
        for the covariance, the unregularised ``Kss = kernel(Z)``."""
        torch = _torch()
        gpr = self.gpr
        b = Ks.shape[0]
        if kss is not None:
            kss = gpr._regularize(kss.to(torch.float64), gpr.alpha)
            out = self._moments(Ks, kss)[0].cpu().numpy()
            return out[:b], out[b:]
        if Kss is not None:
            Kss = Kss.to(torch.float64).clone()
            d = torch.diagonal(Kss)
            d.copy_(gpr._regularize(d, gpr.alpha))
            out, T = self._moments(Ks, d.contiguous(), want_T=True)
            cov = torch.clamp(Kss - Ks.to(torch.float64) @ T, min=0) \
                * float(gpr._ystd)**2
            host = torch.cat((out[:b], cov.reshape(-1))).cpu().numpy()
            return host[:b], host[b:].reshape(b, b)
        # (the mean alone does not touch the inverse: one b x n product)
        return ((Ks.to(torch.float64) @ self.Ky) * float(gpr._ystd)
                + float(gpr._ymean)).cpu().numpy()

    # -- prediction -------------------------------------------------------------
    def predict(self, Z, return_std=False, return_cov=False):
        self._current()
        if not self.available:
            return self.gpr.predict(Z, return_std=return_std,
                                    return_cov=return_cov)
        torch = _torch()
        kernel, dev = self.gpr.kernel, self.Kinv.device
        Ks = torch.as_tensor(kernel.device_cross_gram(Z, self.X), device=dev)
        if return_std is True:
            kss = torch.as_tensor(kernel.device_diag(Z), device=dev)
            return self._predict_from(Ks, kss=kss)
        if return_cov is True:
            if not hasattr(kernel, 'device_gram'):
                raise TypeError('return_cov needs the kernel\'s device_gram')
            Kss = torch.as_tensor(kernel.device_gram(Z), device=dev)
            return self._predict_from(Ks, Kss=Kss)
        return self._predict_from(Ks)
