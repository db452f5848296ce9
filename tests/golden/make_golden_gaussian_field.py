#!/usr/bin/env python
"""Golden vectors of the reference's Gaussian field package and
kernel-induced distance, recorded under the shim of make_golden.py (runs
only where the reference checkout is present).  gaussian_field.json holds,
for fixed 2-D samples and the RBF kernel below (the same as in
tests/test_gaussian_field.py): distances and weights with gradients,
`predict` with and without influence for three smoothings, the pinv branch
of a Laplacian that is not positive definite, ALE and LOOCV (p = 1, 1.5, 2,
3) with gradients at theta != 0, and `fit` with 'loocv2' and 'ale'.
"""
import copy
import json
import os
import sys
import warnings
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402


class RBF:
    """s^2 exp(-|x - y|^2 / 2 l^2); gradient columns d/ds, d/dl."""

    def __init__(self, s=1.0, l=1.0):
        self.s, self.l = s, l

    @property
    def theta(self):
        return np.log([self.s, self.l])

    @theta.setter
    def theta(self, t):
        self.s, self.l = np.exp(t)

    @property
    def bounds(self):
        return np.log([[1e-1, 1e1], [1e-1, 1e1]])

    def clone_with_theta(self, theta):
        k = copy.deepcopy(self)
        k.theta = theta
        return k

    def __call__(self, X, Y=None, eval_gradient=False):
        X = np.asarray(X, float)
        Y = X if Y is None else np.asarray(Y, float)
        d2 = ((X[:, None, :] - Y[None, :, :])**2).sum(-1)
        K = self.s**2 * np.exp(-0.5 * d2 / self.l**2)
        if not eval_gradient:
            return K
        dK = np.stack((2 * K / self.s, K * d2 / self.l**3), axis=-1)
        return K, dK

    def diag(self, X, eval_gradient=False):
        k = np.full(len(X), self.s**2)
        if not eval_gradient:
            return k
        return k, np.column_stack((np.full(len(X), 2 * self.s),
                                   np.zeros(len(X))))


def data():
    rng = np.random.default_rng(23)
    X = rng.uniform(-1.5, 1.5, size=(16, 2))
    Y = rng.uniform(-1.5, 1.5, size=(4, 2))
    y = np.tanh(X[:, 0] - 0.5 * X[:, 1])
    b = (X[:, 0] + 0.3 * X[:, 1] > 0).astype(float)
    unl = rng.choice(len(X), 9, replace=False)
    y[unl] = np.nan
    b[unl] = np.nan
    return X, Y, y, b


#: (s, l, sigma) at theta != 0
PARAMS = (1.3, 0.8, 0.7)
NOT_PD = np.array([[0.0, 2.0, -3.0, 0.5],
                   [2.0, 0.0, 1.0, 0.0],
                   [-3.0, 1.0, 0.0, 1.0],
                   [0.5, 0.0, 1.0, 0.0]])


def main():
    mg.install_shims()
    sys.path.insert(0, mg.REF)
    from graphdot.metric import KernelInducedDistance
    from graphdot.model.gaussian_field import (
        GaussianFieldRegressor, RBFOverDistance, RBFOverFixedDistance)
    X, Y, y, b = data()
    s, l, sigma = PARAMS
    out = {'X': X, 'Y': Y, 'y': y, 'b': b, 'params': PARAMS}

    kid = KernelInducedDistance(RBF(s, l))
    out['kid_xx'], out['kid_xx_grad'] = kid(X, eval_gradient=True)
    out['kid_xy'], out['kid_xy_grad'] = kid(X, Y, eval_gradient=True)

    w = RBFOverDistance(KernelInducedDistance(RBF(s, l)), sigma)
    out['rbf_xx'], out['rbf_xx_grad'] = w(X, eval_gradient=True)
    out['rbf_xy'], out['rbf_xy_grad'] = w(X, Y, eval_gradient=True)
    Dfix = np.sqrt(((X[:, None, :] - X[None, :, :])**2).sum(-1))
    wf = RBFOverFixedDistance(Dfix, sigma)
    idx, jdx = np.arange(0, 16, 2), np.arange(1, 16, 3)
    out['fixed_idx'], out['fixed_jdx'] = idx, jdx
    out['fixed_xx'], out['fixed_xx_grad'] = wf(idx, eval_gradient=True)
    out['fixed_xy'] = wf(idx, jdx)

    def gfr(smoothing=1e-3, optimizer=None):
        return GaussianFieldRegressor(
            RBFOverDistance(KernelInducedDistance(RBF(s, l)), sigma),
            optimizer=optimizer, smoothing=smoothing)

    out['predict'] = []
    for smoothing in (0.0, 1e-3, 0.1):
        z = gfr(smoothing).predict(X, y)
        zi, infl = gfr(smoothing).predict(X, y, return_influence=True)
        out['predict'].append(dict(smoothing=smoothing, z=z, z_infl=zi,
                                   influence=infl))

    yn = np.array([1.0, np.nan, np.nan, 2.0])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        zn = GaussianFieldRegressor('precomputed', smoothing=0).predict(
            NOT_PD, yn)
    assert any('not positive definite' in str(c.message) for c in caught)
    out['not_pd'] = dict(W=NOT_PD, y=yn, z=zn)

    out['ale'] = []
    for smoothing in (1e-3, 0.1):
        loss, grad = gfr(smoothing).average_label_entropy(
            X, b, eval_gradient=True)
        out['ale'].append(dict(smoothing=smoothing, loss=loss, grad=grad))
    out['loocv'] = []
    for p in (1, 1.5, 2, 3):
        g = gfr()
        loss, grad = g.loocv_error(X, y, p=p, eval_gradient=True)
        out['loocv'].append(dict(p=p, loss=loss, grad=grad))

    out['fit'] = []
    for loss, labels in (('loocv2', y), ('ale', b)):
        g = gfr(optimizer=True)
        np.random.seed(0)
        g.fit(X, labels, loss=loss, repeat=1)
        theta = g.weight.theta
        f = (g.average_label_entropy if loss == 'ale'
             else g.loocv_error_2)(X, labels, theta=theta)
        out['fit'].append(dict(loss=loss, theta=theta, value=f))

    with open(os.path.join(HERE, 'gaussian_field.json'), 'w') as f:
        json.dump(mg.jsonable(out), f)
    print('gaussian_field.json written')


if __name__ == '__main__':
    main()
