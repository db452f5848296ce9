#!/usr/bin/env python
"""What the torch loops of graphdot_amd/model/svm/_smo.py must keep: recorded
ONCE on the CPU from the commit before `smo_torch` lost its own copy of the
loop, replayed bit for bit by tests/test_smo_loops.py on the current code.

smo_loops.json holds, per case, `alpha`, `G`, `info` and `slices` of

* `smo_torch(K, y, U)`,
* `smo_torch_from(K, 1, U, *one_class_start(K, nu, U))` and
* `smo2_torch(K, U, z, eps)`

with ``tol = 1e-3`` and ``max_iter = 500`` at (n, P) = (1, 1), (2, 2), (7, 3),
(65, 4), (130, 2), at (7, 3) with a NaN off the diagonal of K (status 1), and
at (65, 4) stopped by ``max_iter = 3``.  The inputs are not stored: `problem`
makes them from uniform draws of a seeded `default_rng` with additions,
multiplications and divisions alone, so they are the same bits wherever IEEE
doubles are.  Every problem has a sample with ``U = 0``; every `y` of two or
more samples holds both signs.

    python tests/golden/make_golden_smo_loops.py     # rewrites the fixture
"""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 2929
TOL = 1e-3
MAX_ITER = 500
#: name: (n, P, max_iter, a NaN in K?)
CASES = {
    'n1_p1': (1, 1, MAX_ITER, False),
    'n2_p2': (2, 2, MAX_ITER, False),
    'n7_p3': (7, 3, MAX_ITER, False),
    'n65_p4': (65, 4, MAX_ITER, False),
    'n130_p2': (130, 2, MAX_ITER, False),
    'n7_p3_nan': (7, 3, MAX_ITER, True),
    'n65_p4_max_iter_3': (65, 4, 3, False),
}
LOOPS = ('smo_torch', 'smo_torch_from', 'smo2_torch')


def problem(name):
    """(`batch` of a case, its `max_iter`)."""
    n, P, max_iter, nan = CASES[name]
    return batch(n, P, nan), max_iter


def batch(n, P, nan=False):
    """K (n, n), y (P, n) int8, U (P, n), nu (P,), z (P, n), eps (P,) as CPU
    tensors."""
    import torch
    rng = np.random.default_rng([SEED, n, P])
    X = rng.random((n, 3))
    d2 = np.zeros((n, n))
    for k in range(3):
        d = X[:, None, k] - X[None, :, k]
        d2 = d2 + d * d
    K = 1.0 / (1.0 + 4.0 * d2)      # (rational quadratic: positive definite)
    if nan:
        K[2, 4] = K[4, 2] = np.nan
    y = np.where(rng.random((P, n)) < 0.5, 1, -1).astype(np.int8)
    U = 0.5 + 1.5 * rng.random((P, n))
    z = 2.0 * rng.random((P, n)) - 1.0
    for p in range(P):
        out = (3 * p + 1) % n
        U[p, out] = 0.0
        if n > 1:
            y[p, p % n], y[p, (p + 1) % n] = 1, -1
    nu = 0.3 + 0.1 * np.arange(P)
    eps = 0.05 + 0.05 * np.arange(P)
    return (torch.from_numpy(K), torch.from_numpy(y), torch.from_numpy(U),
            torch.from_numpy(nu), torch.from_numpy(z), torch.from_numpy(eps))


def run(name):
    """{loop: Result} of a case on the `_smo` module that is importable."""
    import torch
    from graphdot_amd.model.svm import _smo
    (K, y, U, nu, z, eps), max_iter = problem(name)
    return {
        'smo_torch': _smo.smo_torch(K, y, U, TOL, max_iter),
        'smo_torch_from': _smo.smo_torch_from(
            K, torch.ones_like(y), U, *_smo.one_class_start(K, nu, U), TOL,
            max_iter),
        'smo2_torch': _smo.smo2_torch(K, U, z, eps, TOL, max_iter),
    }


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    out = {}
    for name in CASES:
        out[name] = {
            loop: {'alpha': r.alpha.tolist(), 'G': r.G.tolist(),
                   'info': r.info.tolist(), 'slices': r.slices}
            for loop, r in run(name).items()}
    # (what the cases are there for)
    for loop in LOOPS:
        status = [row[3] for row in out['n7_p3_nan'][loop]['info']]
        steps = [row[0] for row in out['n65_p4_max_iter_3'][loop]['info']]
        assert 1.0 in status, (loop, status)
        assert 3.0 in steps and max(steps) == 3.0, (loop, steps)
    # json writes a double with `repr` (and NaN, Infinity, -Infinity by name):
    # `json.load` gives the same bits back
    with open(os.path.join(HERE, 'smo_loops.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))
        f.write('\n')
    for name, loops in out.items():
        print(name, {k: (v['slices'], [row[3] for row in v['info']])
                     for k, v in loops.items()})


if __name__ == '__main__':
    main()
