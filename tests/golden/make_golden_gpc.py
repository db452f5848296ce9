#!/usr/bin/env python
"""Golden vectors of binary Gaussian process classification, recorded with
scikit-learn's ``GaussianProcessClassifier`` (the reference has no
classifier; runs only where scikit-learn is installed -- the package and the
tests never import it).  gpc.json holds two families:

(a) 40 points in 3 dimensions, two overlapping classes, under scikit-learn's
    ``ConstantKernel * RBF`` (`ConstantRBF` below is the same formula on the
    kernel protocol of this package): at three thetas the objective, its
    gradient w.r.t. log-theta and ``pi_``, `predict_proba` on 12 held-out
    points, and one `fit` from a fixed start (final theta and objective).
(b) 30 QM7-like graphs of tests/cases.py labelled "energy above the median":
    the normalised marginalized graph kernel's matrix, gradient planes,
    cross matrix and diagonal from the CPU oracle backend, fed to
    scikit-learn through the precomputed-kernel adaptor below at one theta
    (objective, gradient, probabilities), and stored for `Stored`, the
    stand-in kernel of the test that serves them.

    python tests/golden/make_golden_gpc.py     # rewrites gpc.json
"""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)

#: family (a): log([constant, length scale])
THETAS = [[0.0, 0.0], [1.2, -0.4], [-0.7, 0.9]]
FIT_START = [0.5, 0.3]
N_TRAIN, N_TEST = 40, 12
#: family (b)
N_GRAPHS, N_HELD_OUT = 30, 8


class ConstantRBF:
    """c exp(-|x - y|^2 / 2 l^2); theta = log([c, l]); gradient columns
    d/dc, d/dl in linear scale."""

    def __init__(self, c=1.0, l=1.0):
        self.c, self.l = c, l

    @property
    def theta(self):
        return np.log([self.c, self.l])

    @theta.setter
    def theta(self, t):
        self.c, self.l = np.exp(t)

    @property
    def bounds(self):
        return np.log([[1e-5, 1e5], [1e-5, 1e5]])

    def clone_with_theta(self, theta):
        k = ConstantRBF()
        k.theta = theta
        return k

    def __call__(self, X, Y=None, eval_gradient=False):
        X = np.asarray(X, float)
        Y = X if Y is None else np.asarray(Y, float)
        d2 = ((X[:, None, :] - Y[None, :, :])**2).sum(-1)
        K = self.c * np.exp(-0.5 * d2 / self.l**2)
        if not eval_gradient:
            return K
        return K, np.stack((K / self.c, K * d2 / self.l**3), axis=-1)

    def diag(self, X):
        return np.full(len(X), float(self.c))


class Stored:
    """Family (b)'s matrices on the kernel protocol: the samples are indices
    into `K_all`; the gradient planes cover the training block."""

    def __init__(self, K_all, dK, theta, bounds):
        self.K_all, self.dK = np.asarray(K_all), np.asarray(dK)
        self._theta, self.bounds = np.asarray(theta, float), bounds

    @property
    def theta(self):
        return self._theta

    @theta.setter
    def theta(self, t):
        assert np.allclose(t, self._theta), 'recorded at one theta only'

    def clone_with_theta(self, theta):
        self.theta = theta
        return self

    def __call__(self, X, Y=None, eval_gradient=False):
        i = np.asarray(X, dtype=int).ravel()
        j = i if Y is None else np.asarray(Y, dtype=int).ravel()
        K = self.K_all[np.ix_(i, j)]
        if not eval_gradient:
            return K
        assert Y is None
        return K, self.dK[np.ix_(i, i)]

    def diag(self, X):
        return self.K_all.diagonal()[np.asarray(X, dtype=int).ravel()]


def points():
    """(X, y, Z): two unit normal clouds one unit apart per coordinate."""
    rng = np.random.default_rng(2024)
    y = np.arange(N_TRAIN) % 2
    X = rng.normal(size=(N_TRAIN, 3)) + y[:, None]
    Z = rng.normal(size=(N_TEST, 3)) + (np.arange(N_TEST) % 2)[:, None]
    return X, y, Z


def graph_matrices():
    """(K_all, dK of the training block, labels, theta, bounds) from the
    oracle backend."""
    sys.path.insert(0, TESTS)
    sys.path.insert(0, os.path.dirname(TESTS))
    import cases
    from oracle_backend import OracleBackend
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    G = cases.config3_graphs(N_GRAPHS + N_HELD_OUT, seed=11)
    e = cases.synthetic_energies(G)[:N_GRAPHS]
    knode, kedge, q = cases.config3_fit_kernels()
    kernel = Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, backend=OracleBackend()))
    K_all = np.asarray(kernel(G), dtype=np.float64)
    _, dK = kernel(G[:N_GRAPHS], eval_gradient=True)
    return (K_all, np.asarray(dK, dtype=np.float64),
            (e > np.median(e)).astype(int), np.array(kernel.theta),
            np.asarray(kernel.bounds, dtype=float))


def sklearn_adaptor(stored):
    """`stored` as a scikit-learn kernel over sample indices (gradient
    w.r.t. log-theta, scikit-learn's convention)."""
    from sklearn.gaussian_process.kernels import Kernel

    class Precomputed(Kernel):
        def __init__(self, stored):
            self.stored = stored

        @property
        def theta(self):
            return self.stored.theta

        @theta.setter
        def theta(self, t):
            self.stored.theta = t

        @property
        def bounds(self):
            return self.stored.bounds

        def is_stationary(self):
            return False

        def diag(self, X):
            return self.stored.diag(X[:, 0])

        def __call__(self, X, Y=None, eval_gradient=False):
            out = self.stored(X[:, 0], None if Y is None else Y[:, 0],
                              eval_gradient)
            if not eval_gradient:
                return out
            return out[0], out[1] * np.exp(self.stored.theta)

    return Precomputed(stored)


def main():
    from sklearn.gaussian_process import GaussianProcessClassifier
    from sklearn.gaussian_process.kernels import ConstantKernel, RBF
    sys.path.insert(0, HERE)
    from make_golden import jsonable

    X, y, Z = points()
    out = {'points': {'X': X, 'y': y, 'Z': Z, 'at': []}}
    for theta in THETAS:
        c, l = np.exp(theta)
        gpc = GaussianProcessClassifier(ConstantKernel(c) * RBF(l),
                                        optimizer=None).fit(X, y)
        value, grad = gpc.log_marginal_likelihood(np.array(theta),
                                                  eval_gradient=True)
        assert np.allclose(ConstantRBF(c, l)(X), gpc.kernel_(X))
        out['points']['at'].append(dict(
            theta=theta, value=value, grad=grad,
            pi=gpc.base_estimator_.pi_, proba=gpc.predict_proba(Z)))
    c, l = np.exp(FIT_START)
    gpc = GaussianProcessClassifier(ConstantKernel(c) * RBF(l)).fit(X, y)
    out['points']['fit'] = dict(
        start=FIT_START, theta=gpc.kernel_.theta,
        value=gpc.log_marginal_likelihood_value_,
        proba=gpc.predict_proba(Z))

    K_all, dK, labels, theta, bounds = graph_matrices()
    stored = Stored(K_all, dK, theta, bounds)
    train = np.arange(N_GRAPHS, dtype=float)[:, None]
    held = N_GRAPHS + np.arange(N_HELD_OUT, dtype=float)[:, None]
    gpc = GaussianProcessClassifier(sklearn_adaptor(stored),
                                    optimizer=None).fit(train, labels)
    value, grad = gpc.log_marginal_likelihood(theta, eval_gradient=True)
    out['graphs'] = dict(
        K_all=K_all, dK=dK, labels=labels, theta=theta, bounds=bounds,
        value=value, grad=grad, pi=gpc.base_estimator_.pi_,
        proba=gpc.predict_proba(held))

    with open(os.path.join(HERE, 'gpc.json'), 'w') as f:
        json.dump(jsonable(out), f)
    print('gpc.json written: %d bytes' % os.path.getsize(
        os.path.join(HERE, 'gpc.json')))


if __name__ == '__main__':
    main()
