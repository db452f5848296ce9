#!/usr/bin/env python
"""Golden vectors of the reference's GPROutlierDetector, recorded under the
shim of make_golden.py (runs only where the reference checkout is present).
outlier_detector.json holds, for the reference test's 1-D RBF kernel (the
same as in tests/test_outlier_detector.py) on 12 points with two shifted
targets: `log_marginal_likelihood` value and gradient at several theta_ext,
with raw and normalised targets, some with the clamp of the pseudo-inverse
inactive and some with it active (asserted below); and seeded `fit` results
(repeat = 3, w = 0 and w > 0): theta, y_uncertainty, and `predict` mean,
std and cov.
"""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402


class RBFKernel:
    """v exp(-d^2 / 2 L^2); gradient columns d/dv, d/dL (the reference
    test's kernel)."""

    def __init__(self, v, L):
        self.v = v
        self.L = L

    def __call__(self, X, Y=None, eval_gradient=False):
        v, L = self.v, self.L
        d = np.subtract.outer(X, Y if Y is not None else X)
        f = v * np.exp(-0.5 * d**2 / L**2)
        if eval_gradient is False:
            return f
        j1 = np.exp(-0.5 * d**2 / L**2)
        j2 = v * np.exp(-0.5 * d**2 / L**2) * d**2 * L**-3
        return f, np.stack((j1, j2), axis=2)

    def diag(self, X):
        return np.ones_like(X)

    @property
    def theta(self):
        return np.log([self.v, self.L])

    @theta.setter
    def theta(self, t):
        self.v, self.L = np.exp(t)

    @property
    def bounds(self):
        return np.log([[1e-5, 1e5], [1e-2, 10]])

    def clone_with_theta(self, theta):
        k = RBFKernel(1.0, 1.0)
        k.theta = theta
        return k


def data():
    X = np.linspace(-1, 1, 12, endpoint=False)
    y = np.sin(X * np.pi)
    y[3] += 0.5
    y[7] -= 0.4
    Z = np.linspace(-1.2, 1.2, 7)
    return X, y, Z


#: (v, L, sigma per sample as (value, first sample's value), normalize_y)
LML_CASES = [
    (1.0, 1.0, 0.1, None, False),
    (2.0, 0.5, 0.01, 0.3, False),
    (0.5, 0.3, 0.05, None, True),
    (1.0, 1.0, 1e-3, None, False),
    (1.0, 1.0, 1e-4, None, False),       # clamp active
    (5.0, 2.0, 1e-4, 0.2, False),        # clamp active
    (1.0, 1.0, 1e-4, None, True),        # clamp active
]


def clamps(K, beta):
    a = np.linalg.eigvalsh(K)
    return bool((a <= beta * a.max()).any())


def main():
    mg.install_shims()
    sys.path.insert(0, mg.REF)
    from graphdot.model.gaussian_process import GPROutlierDetector
    X, y, Z = data()
    out = {'X': X, 'y': y, 'Z': Z, 'lml': [], 'fit': []}
    n_clamped = 0
    for v, L, s, s0, normalize in LML_CASES:
        gpr = GPROutlierDetector(RBFKernel(v, L), normalize_y=normalize)
        gpr.X, gpr.y = X, y
        sigma = np.full(len(X), s)
        if s0 is not None:
            sigma[0] = s0
        theta_ext = np.concatenate((np.log([v, L]), np.log(sigma)))
        val, grad = gpr.log_marginal_likelihood(theta_ext,
                                                eval_gradient=True)
        K = RBFKernel(v, L)(X) + np.diag(sigma**2)
        c = clamps(K, gpr.beta)
        n_clamped += c
        out['lml'].append(dict(v=v, L=L, normalize_y=normalize,
                               theta_ext=theta_ext, value=val, grad=grad,
                               clamped=c, cond=np.linalg.cond(K)))
    assert n_clamped >= 1, 'no case exercises the clamp'
    assert n_clamped < len(LML_CASES), 'no case without the clamp'

    for w, normalize in ((0.0, False), (0.05, False), (0.02, True)):
        gpr = GPROutlierDetector(RBFKernel(1.0, 1.0), normalize_y=normalize)
        np.random.seed(1)
        gpr.fit(X, y, w=w, repeat=3, theta_jitter=1.0)
        mean, std = gpr.predict(Z, return_std=True)
        _, cov = gpr.predict(Z, return_cov=True)
        out['fit'].append(dict(w=w, normalize_y=normalize, seed=1, repeat=3,
                               theta=gpr.kernel.theta,
                               y_uncertainty=gpr.y_uncertainty,
                               mean=mean, std=std, cov=cov))

    with open(os.path.join(HERE, 'outlier_detector.json'), 'w') as f:
        json.dump(mg.jsonable(out), f)
    print('outlier_detector.json written: %d of %d likelihood cases clamped'
          % (n_clamped, len(LML_CASES)))


if __name__ == '__main__':
    main()
