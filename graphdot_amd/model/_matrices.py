"""The kernel matrices of the models that work on a whole Gram matrix where it
lies (`KernelPCA`, `KernelKMeans`, the neighbour models): a precomputed
matrix as it was handed in, or the kernel's own -- adopted from its device
path on a GPU, evaluated on the host otherwise."""
import numpy as np
from ._device_kernel import device_call, on_device


def _torch():
    import torch
    return torch


class KernelMatrices:
    """Expects `kernel`, `kernel_options` and `device` on the model, and,
    for `_cross`, the training set `X` and its size `_n`."""

    def _dense(self):
        from .gaussian_process.gpr import _Dense
        if getattr(self, '_la_device', None) != self.device \
                or not hasattr(self, '_la'):
            self._la, self._la_device = _Dense(self.device), self.device
        return self._la

    @property
    def _precomputed(self):
        return isinstance(self.kernel, str) and self.kernel == 'precomputed'

    def _given(self, M, shape, device=None):
        """A matrix handed in as it lies: a tensor stays on its device (or
        goes to `device`), an array goes to the algebra's."""
        torch = _torch()
        if torch.is_tensor(M):
            M = M.detach()
            if device is not None and M.device != device:
                M = M.to(device)
        else:
            M = np.asarray(M)
            if M.dtype not in (np.float32, np.float64):
                M = M.astype(np.float64)
            M = torch.from_numpy(np.ascontiguousarray(M)).to(
                device if device is not None else self._dense().device)
        if M.dtype not in (torch.float32, torch.float64):
            M = M.to(torch.float64)
        if M.dim() != 2 or any(s is not None and s != t
                               for s, t in zip(shape, M.shape)):
            raise ValueError(f'a matrix of shape {shape} expected, got '
                             f'{tuple(M.shape)}')
        return M

    def _gram(self, X):
        """(K as a tensor where the algebra runs, from the device path?)"""
        if self._precomputed:
            K = self._given(X, (None, None))
            if K.shape[0] != K.shape[1]:
                raise ValueError('precomputed: a square matrix expected, got '
                                 f'{tuple(K.shape)}')
            return K, False
        la = self._dense()
        if on_device(la, self.kernel_options):
            Kd = device_call(self.kernel, 'device_gram', X)
            if Kd is not None:
                # adopted where the solver wrote it, in its arithmetic and
                # layout; valid until the next evaluation on that backend
                return _torch().as_tensor(Kd, device=la.device), True
        return la.tensor(self.kernel(X, **self.kernel_options)), False

    def _cross(self, Z, device):
        return self._cross_from(Z, device)[0]

    def _cross_from(self, Z, device):
        """(the cross matrix of `Z` against the training set on `device`,
        from the device path?)"""
        if self._precomputed:
            return self._given(Z, (None, self._n), device), False
        la = self._dense()
        if on_device(la, self.kernel_options) and device.type == 'cuda':
            Ks = device_call(self.kernel, 'device_cross_gram', Z, self.X)
            if Ks is not None:
                return _torch().as_tensor(Ks, device=device), True
        Ks = np.asarray(self.kernel(Z, self.X, **self.kernel_options),
                        dtype=np.float64)
        return _torch().from_numpy(np.ascontiguousarray(Ks)).to(device), False

    def _self_similarity(self, Z, device):
        """(b,) float64 k(z, z) of the graphs `Z` on `device`: from the
        kernel's `device_diag` on a GPU, from `kernel.diag` otherwise."""
        la = self._dense()
        if on_device(la, self.kernel_options) and device.type == 'cuda':
            d = device_call(self.kernel, 'device_diag', Z)
            if d is not None:
                return _torch().as_tensor(d, device=device).to(
                    _torch().float64)
        d = np.asarray(self.kernel.diag(Z, **self.kernel_options),
                       dtype=np.float64)
        return _torch().from_numpy(np.ascontiguousarray(d)).to(device)
