#!/usr/bin/env python
"""Golden vectors of the reference's KernelOverMetric, recorded under the
shim of make_golden.py (runs only where the reference checkout is present;
sympy's ufuncify compiles the formulas with the C toolchain of that machine).

kernel_over_metric.json holds, for five formulas (Gaussian, the reference
test's rational quadratic, exp(-d / ell), Matern-3/2, a polynomial with
integer powers) over three distances -- the reference test's
PairwiseDistance stub (one theta) and a replay distance with 0 and with 3
gradient columns, whose seeded float32 matrices are stored here too
(symmetric with a zero diagonal over the whole pool) -- the X-only and X, Y
values and gradients with their dtypes, `diag`, `theta`, `bounds`,
`hyperparameters` and a clone at other theta.  (The reference's `bounds`
needs the np.vstack shim below on current numpy.)  tests/test_kernel_over_metric.py
defines the two stubs again, identically.
"""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402


class PairwiseDistance:
    """The reference test's distance |x - y| * scale, one theta."""

    def __init__(self, scale):
        self.scale = scale

    def __call__(self, X, Y=None, eval_gradient=False):
        distance = np.abs(np.subtract.outer(X, Y if Y is not None else X))
        if eval_gradient is True:
            return self.scale * distance, distance.reshape(*distance.shape, 1)
        else:
            return self.scale * distance

    @property
    def hyperparameters(self):
        return (self.scale,)

    @property
    def theta(self):
        return np.log([self.scale])

    @theta.setter
    def theta(self, value):
        self.scale = np.exp(value)[0]

    @property
    def bounds(self):
        return np.log([[1e-4, 1e4]])

    def clone_with_theta(self, theta=None):
        if theta is None:
            theta = self.theta
        clone = type(self)(scale=self.scale)
        clone.theta = theta
        return clone


class ReplayDistance:
    """Fixed float32 matrices over a pool of samples: X, Y are index arrays,
    the distance is D[X][:, Y] and its gradient dD[X][:, Y] (n_theta
    columns); theta only travels along."""

    def __init__(self, D, dD, theta):
        self.D = np.asarray(D, dtype=np.float32)
        self.dD = np.asarray(dD, dtype=np.float32).reshape(
            *self.D.shape, len(theta))
        self._theta = np.array(theta, dtype=float)

    def __call__(self, X, Y=None, eval_gradient=False):
        Y = X if Y is None else Y
        D = self.D[np.ix_(X, Y)]
        if eval_gradient is True:
            return D, self.dD[np.ix_(X, Y)]
        return D

    @property
    def hyperparameters(self):
        return tuple(np.exp(self._theta))

    @property
    def theta(self):
        return self._theta.copy()

    @theta.setter
    def theta(self, value):
        self._theta = np.array(value, dtype=float)

    @property
    def bounds(self):
        return np.log(np.tile([[1e-3, 1e3]], (len(self._theta), 1)))

    def clone_with_theta(self, theta=None):
        if theta is None:
            theta = self.theta
        return type(self)(self.D, self.dD, theta)


FORMULAS = [
    ('gauss', 'v * exp(-d^2 / ell^2)',
     dict(v=(1.0, (1e-2, 1e2)), ell=(1.3, (1e-2, 1e2)))),
    ('rq', 'v * (1 + d**2 / (2 * a * ell**2)) ** -a',
     dict(v=(1.2, (1e-5, 1e5)), a=(0.9, (1e-5, 1e5)),
          ell=(1.1, (1e-2, 1e2)))),
    ('exp', 'exp(-d/ell)', dict(ell=0.7)),
    ('matern32', 'v * (1 + sqrt(3) * d / ell) * exp(-sqrt(3) * d / ell)',
     dict(v=(1.0,), ell=(0.8, 1e-2, 1e2))),
    ('ipow', 'v * (1 - d / ell)**4 * (4 * d / ell + 1) + c * d**2',
     dict(v=(1.1, (1e-2, 1e2)), ell=(2.5, (0.1, 10.0)),
          c=(0.05, (1e-3, 1.0)))),
]


def replay_pool(n, n_theta, seed):
    """Seeded symmetric float32 distances with a zero diagonal and
    symmetric gradient planes (zero on the diagonal too)."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.05, 1.5, (n, n))
    D = np.triu(A, 1)
    D = (D + D.T).astype(np.float32)
    dD = rng.normal(size=(n, n, n_theta))
    dD = 0.5 * (dD + dD.transpose(1, 0, 2))
    dD[np.arange(n), np.arange(n), :] = 0
    return D, dD.astype(np.float32), rng.normal(size=n_theta) * 0.3


def distances():
    """(name, constructor spec, X, Y, theta for the clone's distance part)"""
    out = [('pairwise', dict(kind='pairwise', scale=1.5),
            np.linspace(-1, 2, 7), np.linspace(-0.5, 3, 5))]
    for n_theta, seed in ((0, 11), (3, 12)):
        D, dD, theta = replay_pool(9, n_theta, seed)
        out.append((f'replay{n_theta}',
                    dict(kind='replay', D=D, dD=dD, theta=theta),
                    np.array([0, 2, 3, 5, 8]), np.array([1, 4, 6, 7])))
    return out


def make_distance(spec):
    if spec['kind'] == 'pairwise':
        return PairwiseDistance(spec['scale'])
    return ReplayDistance(spec['D'], spec['dD'], spec['theta'])


def record(KernelOverMetric, expr, hypers, spec, X, Y):
    k = KernelOverMetric(make_distance(spec), expr, 'd', **hypers)
    rec = {}
    K, G = k(X, eval_gradient=True)
    rec['K_X'], rec['K_X_dtype'] = K, K.dtype.str
    rec['G_X'], rec['G_X_dtype'] = G, G.dtype.str
    rec['K_X_nograd'] = k(X)
    K, G = k(X, Y, eval_gradient=True)
    rec['K_XY'], rec['K_XY_dtype'] = K, K.dtype.str
    rec['G_XY'], rec['G_XY_dtype'] = G, G.dtype.str
    d = k.diag(X)
    rec['diag'], rec['diag_dtype'] = d, d.dtype.str
    rec['theta'] = k.theta
    rec['bounds'] = k.bounds
    hp = k.hyperparameters
    rec['hyperparameters'] = dict(typename=type(hp).__name__,
                                  fields=list(hp._fields),
                                  values=[list(v) if isinstance(v, tuple)
                                          else v for v in hp])
    theta2 = k.theta + 0.1 * np.arange(1, len(k.theta) + 1)
    c = k.clone_with_theta(theta2)
    rec['clone_theta_in'] = theta2
    rec['clone_theta'] = c.theta
    rec['clone_K_X'] = c(X)
    rec['original_theta_after_clone'] = k.theta
    return rec


def install_vstack_shim():
    """numpy >= 1.24 refuses a dict view in np.vstack, which the
    reference's `bounds` passes (another shim in the spirit of
    make_golden.install_shims)."""
    vstack = np.vstack

    def shimmed(tup, *args, **kwargs):
        if not isinstance(tup, (list, tuple, np.ndarray)):
            tup = list(tup)
        return vstack(tup, *args, **kwargs)
    np.vstack = shimmed


def main():
    mg.install_shims()
    install_vstack_shim()
    sys.path.insert(0, mg.REF)
    from graphdot.kernel import KernelOverMetric
    out = {'formulas': [], 'distances': {}, 'cases': []}
    for name, expr, hypers in FORMULAS:
        out['formulas'].append(dict(name=name, expr=expr, hypers=hypers))
    for dname, spec, X, Y in distances():
        out['distances'][dname] = dict(spec=spec, X=X, Y=Y)
        for name, expr, hypers in FORMULAS:
            rec = record(KernelOverMetric, expr, hypers, spec, X, Y)
            rec.update(formula=name, distance=dname)
            out['cases'].append(rec)
    with open(os.path.join(HERE, 'kernel_over_metric.json'), 'w') as f:
        json.dump(mg.jsonable(out), f)
    print('kernel_over_metric.json written: %d cases' % len(out['cases']))


if __name__ == '__main__':
    main()
