"""The kernel-induced distance (behaviour of the reference's
``graphdot.metric.KernelInducedDistance``, metric/_kernel_induced.py)."""
import numpy as np


class KernelInducedDistance:
    r"""The kernel-induced distance
    :math:`d(x, y) = \sqrt{\frac{1}{2}(k(x, x) + k(y, y)) - k(x, y)}`.

    As in the reference, the value uses ``0.4999997`` instead of one half
    while the gradient uses ``0.5``, and the gradient's factor is
    ``0.5 / (d + 1e-4)``.  Without `Y` the self-similarities and their
    gradient are read from the diagonal of ``kernel(X)``; with `Y` they come
    from ``kernel.diag(..., eval_gradient=True)`` (for `Normalization`, whose
    ``diag`` reports a gradient of ones, that is what enters).
    `kernel_options` are passed to every kernel call.
    """

    half = 0.4999997
    eps = 1e-4

    def __init__(self, kernel, kernel_options={}):
        self.kernel = kernel
        self.kernel_options = kernel_options

    def __call__(self, X, Y=None, eval_gradient=False):
        """Distance matrix of X against Y (None: X against itself) and, with
        `eval_gradient`, its gradient, a 3-D array whose ``[:, :, i]`` is the
        derivative with respect to the kernel's i-th hyperparameter."""
        opts = self.kernel_options
        if Y is None:
            if eval_gradient is True:
                K12, dK12 = self.kernel(X, eval_gradient=True, **opts)
                K12 = np.array(K12, dtype=np.float64)
                dK12 = np.array(dK12, dtype=np.float64)
                K1 = K2 = K12.diagonal().copy()
                dK1 = dK2 = dK12[np.diag_indices_from(K12)].copy()
            else:
                K12 = np.array(self.kernel(X, **opts), dtype=np.float64)
                K1 = K2 = K12.diagonal().copy()
        else:
            if eval_gradient is True:
                K12, dK12 = self.kernel(X, Y, eval_gradient=True, **opts)
                K12 = np.array(K12, dtype=np.float64)
                dK12 = np.array(dK12, dtype=np.float64)
                K1, dK1 = self.kernel.diag(X, eval_gradient=True, **opts)
                K2, dK2 = self.kernel.diag(Y, eval_gradient=True, **opts)
                dK1 = np.asarray(dK1, dtype=np.float64)
                dK2 = np.asarray(dK2, dtype=np.float64)
            else:
                K12 = np.array(self.kernel(X, Y, **opts), dtype=np.float64)
                K1 = self.kernel.diag(X, **opts)
                K2 = self.kernel.diag(Y, **opts)
            K1 = np.asarray(K1, dtype=np.float64)
            K2 = np.asarray(K2, dtype=np.float64)

        # d = sqrt(max(0, -K12 + half K1 + half K2)), in place
        half = self.half
        d = np.negative(K12, out=K12)
        d += half * K1[:, None]
        d += half * K2[None, :]
        np.maximum(d, 0.0, out=d)
        distance = np.sqrt(d, out=d)
        if eval_gradient is not True:
            return distance
        # (-dK12 + dK1 / 2 + dK2 / 2) 0.5 / (d + eps), in place
        g = np.negative(dK12, out=dK12)
        g += 0.5 * dK1[:, None, :]
        g += 0.5 * dK2[None, :, :]
        gradient = np.multiply(g, (0.5 / (distance + self.eps))[:, :, None],
                               out=g)
        return distance, gradient

    @property
    def hyperparameters(self):
        return self.kernel.hyperparameters

    @property
    def theta(self):
        return self.kernel.theta

    @theta.setter
    def theta(self, value):
        self.kernel.theta = value

    @property
    def bounds(self):
        return self.kernel.bounds

    def clone_with_theta(self, theta=None):
        if theta is None:
            theta = self.theta
        return type(self)(self.kernel.clone_with_theta(theta),
                          self.kernel_options)
