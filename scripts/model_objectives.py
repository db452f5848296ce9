#!/usr/bin/env python
"""One objective with its gradient of each model beside the exact regressor,
on the device path, written bit for bit (``float.hex``): what a refactor of
the models' host side must leave unchanged.  QM7-like graphs
(tests/cases.py configuration 3), the normalised float64 graph kernel:

* `LowRankApproximateGPR.log_marginal_likelihood` (a core set of 40);
* `GPROutlierDetector.log_marginal_likelihood`, and the inverse's path;
* `GaussianFieldRegressor.average_label_entropy` and `loocv_error`;
* `DevicePosterior.predict` with the standard deviation of a fitted
  `GaussianProcessRegressor`.

    python scripts/model_objectives.py [TREE] OUT.json

TREE (default: this tree) is the checkout whose `graphdot_amd` is imported:
run once per tree and compare the files (`--compare A.json B.json` exits
non-zero if any number differs).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(a):
    return [float(v).hex() for v in np.atleast_1d(np.asarray(a, float)).ravel()]


def objectives(n):
    import torch                                       # noqa: F401 (first)
    import cases
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.metric import KernelInducedDistance
    from graphdot_amd.model.gaussian_field import (GaussianFieldRegressor,
                                                   RBFOverDistance)
    from graphdot_amd.model.gaussian_process import (
        DevicePosterior, GaussianProcessRegressor, GPROutlierDetector,
        LowRankApproximateGPR)
    G = np.asarray(cases.config3_graphs(n), dtype=object)
    y = cases.synthetic_energies(list(G))
    y = (y - y.mean()) / y.std()
    knode, kedge, q = cases.config3_fit_kernels()
    k = Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, backend=HIPBackend(real=np.float64), ftol=1e-13))
    theta = np.array(k.theta)
    out = {}

    m = LowRankApproximateGPR(k, alpha=1e-4, device='cuda')
    v, g = m.log_marginal_likelihood(theta, C=G[:40], X=G, y=y,
                                     eval_gradient=True)
    out['nystrom'] = {'value': _hex(v), 'gradient': _hex(g)}

    m = GPROutlierDetector(k, device='cuda')
    ext = np.concatenate((theta, np.full(n, 0.5 * np.log(0.05))))
    v, g = m.log_marginal_likelihood(ext, X=G, y=y, eval_gradient=True)
    out['outlier'] = {'value': _hex(v), 'gradient': _hex(g),
                      'path': m.last_timing['path']}

    yy = y.copy()
    yy[::3] = np.nan
    b = (y > 0).astype(float)
    b[::3] = np.nan
    m = GaussianFieldRegressor(RBFOverDistance(KernelInducedDistance(k), 0.3),
                               smoothing=1e-3, device='cuda')
    v, g = m.average_label_entropy(G, b, eval_gradient=True)
    out['gfr_ale'] = {'value': _hex(v), 'gradient': _hex(g)}
    v, g = m.loocv_error(G, yy, eval_gradient=True)
    out['gfr_loocv'] = {'value': _hex(v), 'gradient': _hex(g)}

    m = GaussianProcessRegressor(k, alpha=1e-2, normalize_y=True,
                                 device='cuda')
    m.fit(G[:n - 20], y[:n - 20])
    post = DevicePosterior(m)
    mean, std = post.predict(G[n - 20:], return_std=True)
    out['posterior'] = {'available': bool(post.available),
                        'mean': _hex(mean), 'std': _hex(std)}
    return out


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == '--compare':
        with open(argv[1]) as fa, open(argv[2]) as fb:
            a, b = json.load(fa), json.load(fb)
        a.pop('tree', None), b.pop('tree', None)
        differ = [key for key in sorted(set(a) | set(b))
                  if a.get(key) != b.get(key)]
        print('equal to the last bit' if not differ
              else f'differ: {", ".join(differ)}')
        sys.exit(1 if differ else 0)
    tree = os.path.abspath(argv[0]) if len(argv) > 1 else ROOT
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, tree)
    res = {'tree': os.path.relpath(tree, ROOT), 'graphs': 200}
    res.update(objectives(200))
    os.makedirs(os.path.dirname(os.path.abspath(argv[-1])), exist_ok=True)
    with open(argv[-1], 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(f'{argv[-1]}: ' + ', '.join(k for k in res if k not in ('tree',
                                                                  'graphs')))


if __name__ == '__main__':
    main()
