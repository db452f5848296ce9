"""Weight functions of the Gaussian field regressor (behaviour of the
reference's ``graphdot.model.gaussian_field.weight``): distance matrices
turned into edge weights."""
from abc import ABC, abstractmethod
import copy
import numpy as np


class Weight(ABC):

    @abstractmethod
    def __call__(self, X, Y=None, eval_gradient=False):
        """The weight matrix between X and Y (None: X against itself) and,
        with `eval_gradient`, its gradient: a 3-D array whose ``[:, :, i]``
        is the derivative with respect to the i-th hyperparameter."""

    @property
    @abstractmethod
    def theta(self):
        """An ndarray of all the hyperparameters in log scale."""

    @theta.setter
    @abstractmethod
    def theta(self, values):
        """Set the hyperparameters from an array of log-scale values."""

    @property
    @abstractmethod
    def bounds(self):
        """The log-scale bounds of the hyperparameters as a 2D array."""

    def clone_with_theta(self, theta):
        clone = copy.deepcopy(self)
        clone.theta = theta
        return clone


class RBFOverDistance(Weight):
    """Weights ``exp(-d^2 / (2 sigma^2))`` of a `metric`'s distances (zero
    on the diagonal of X against itself); `mopts` go to the metric.  The
    gradient's first column is d/dsigma, ``d^2 w sigma^-3``, the others the
    metric's columns times ``-d w sigma^-2`` (as in the reference)."""

    def __init__(self, metric, sigma, sigma_bounds=(1e-3, 1e3), mopts={}):
        self.sigma = sigma
        self.sigma_bounds = sigma_bounds
        self.metric = metric
        self.mopts = mopts

    def __call__(self, X, Y=None, eval_gradient=False):
        Z = (X,) if Y is None else (X, Y)
        if eval_gradient is True:
            D, dD = self.metric(*Z, eval_gradient=True, **self.mopts)
        else:
            D = self.metric(*Z, **self.mopts)
        W = np.exp(-0.5 * D**2 * self.sigma**-2)
        if Y is None:
            W[np.diag_indices_from(W)] = 0
        if eval_gradient:
            dsigma = D**2 * W * self.sigma**-3
            dtheta = (-D * W * self.sigma**-2)[:, :, None] * dD
            dW = np.concatenate([dsigma.reshape(*dsigma.shape, 1), dtheta],
                                axis=2)
            return W, dW
        return W

    @property
    def theta(self):
        return np.concatenate((np.log([self.sigma]), self.metric.theta))

    @theta.setter
    def theta(self, values):
        self.sigma = np.exp(values[0])
        self.metric.theta = values[1:]

    @property
    def bounds(self):
        return np.vstack((np.log([self.sigma_bounds]), self.metric.bounds))


class RBFOverFixedDistance(Weight):
    """Weights ``exp(-d^2 / (2 sigma^2))`` over a fixed distance matrix `D`
    whose indices are the samples (`sticky_cache`: unused, as in the
    reference)."""

    def __init__(self, D, sigma, sigma_bounds=(1e-3, 1e3),
                 sticky_cache=False):
        self.sigma = sigma
        self.sigma_bounds = sigma_bounds
        self.D = D

    def __call__(self, X, Y=None, eval_gradient=False):
        d = self.D[X, :][:, X if Y is None else Y]
        w = np.exp(-0.5 * d**2 * self.sigma**-2)
        if Y is None:
            w[np.diag_indices_from(w)] = 0
        if eval_gradient:
            j = d**2 * w * self.sigma**-3
            return w, np.stack([j], axis=2)
        return w

    @property
    def theta(self):
        return np.log([self.sigma])

    @theta.setter
    def theta(self, values):
        self.sigma = np.exp(values)[0]

    @property
    def bounds(self):
        return np.log([self.sigma_bounds])
