#!/usr/bin/env python
"""Golden picks of the reference's active-learning selectors
(graphdot/model/active_learning: DeterminantMaximizer, VarianceMinimizer,
HierarchicalDrafter).  Needs a checkout of the reference (make_golden.REF);
the test-suite only reads active_learning.json.

The reference is imported under the shim of make_golden.py plus a stand-in
`numba` module (numba is not a dependency of this project) whose `jit` leaves the function as it is -- the
reference's own `forceobj=True` object-mode loop, run by Python.  Nothing of
the reference is copied: inputs and the indices it picks are recorded.

Problems: random 1-D and 3-D points under the RBF kernel
``exp(-|x - y|^2 / (2 l^2))``, N from 50 to 400, n from 5 to 40.  Only
problems whose best and second-best criterion differ at every step by at least
`MIN_GAP` (relative to the best criterion of the first step, the scale of
the problem's rounding errors; measured with a plain float64 restatement of
the criterion, recorded as `gap`) are kept, so that the float32 arithmetic of the
reference's DeterminantMaximizer and every other summation order pick the
same indices.  The drafter cases run the selectors with a callable RBF kernel
on the points and a fixed `random_state`.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402

MIN_GAP = {'determinant': 1e-4, 'variance': 1e-7}


def install_numba_stub():
    nb = types.ModuleType('numba')
    nb.__path__ = []
    nb.jit = lambda *args, **kwargs: (lambda f: f)
    core = types.ModuleType('numba.core')
    core.__path__ = []
    nbtypes = types.ModuleType('numba.core.types')

    class _T:
        def __getitem__(self, item):
            return self

        def __call__(self, *args):
            return self

    for name in ('intc', 'float32', 'float64', 'int32', 'int64'):
        setattr(nbtypes, name, _T())
    nb.core, core.types = core, nbtypes
    sys.modules.update({'numba': nb, 'numba.core': core,
                        'numba.core.types': nbtypes})


def rbf(X, length):
    X = np.asarray(X, dtype=np.float64)
    d2 = ((X[:, None, :] - X[None, :, :])**2).sum(-1)
    return np.exp(-0.5 * d2 / length**2)


def relative_gaps(K, picks, method, alpha=0.0):
    """Smallest gap between the best and the second-best criterion over the
    steps of the given picks, relative to the best criterion of the first
    step, by a plain float64 restatement."""
    gaps = []
    chosen = []
    N = len(K)
    Kr = K.copy()
    for s in range(len(picks)):
        rest = np.setdiff1d(np.arange(N), chosen)
        if method == 'determinant':
            crit = (Kr**2).sum(axis=1)[rest]
        else:
            A = K + alpha * np.eye(N)
            if chosen:
                P = A[np.ix_(rest, rest)] - A[np.ix_(rest, chosen)] @ \
                    np.linalg.solve(A[np.ix_(chosen, chosen)],
                                    A[np.ix_(chosen, rest)])
            else:
                P = A
            crit = P.sum(axis=1)
        top = np.sort(crit)[::-1]
        if s == 0:
            scale = abs(top[0])
        gaps.append((top[0] - top[1]) / scale if len(top) > 1 else np.inf)
        i = picks[s]
        if method == 'determinant':
            v = Kr[i] / np.linalg.norm(Kr[i])
            Kr = Kr - np.outer(Kr @ v, v)
        chosen.append(i)
    return float(min(gaps))


def main():
    mg.install_shims()
    install_numba_stub()
    sys.path.insert(0, mg.REF)
    from graphdot.model.active_learning import (
        DeterminantMaximizer, VarianceMinimizer, HierarchicalDrafter)

    rng = np.random.default_rng(20261015)
    problems = []
    want = {('determinant', 1): 4, ('determinant', 3): 4,
            ('variance', 1): 4, ('variance', 3): 4}
    tried = 0
    while any(v > 0 for v in want.values()) and tried < 4000:
        tried += 1
        method = ['determinant', 'variance'][tried % 2]
        dim = [1, 3][(tried // 2) % 2]
        if want[(method, dim)] == 0:
            continue
        N = int(rng.integers(50, 401))
        n = int(rng.integers(5, 41))
        X = rng.uniform(-1, 1, size=(N, dim))
        length = float(rng.choice([0.05, 0.1, 0.2, 0.3]))
        K = rbf(X, length)
        if method == 'determinant':
            picks = DeterminantMaximizer('precomputed')(K, n)
            alpha = 0.0
        else:
            alpha = 1e-6
            picks = VarianceMinimizer('precomputed', alpha=alpha)(K, n)
        picks = [int(i) for i in picks]
        if len(set(picks)) != n:
            continue
        gap = relative_gaps(K, picks, method, alpha)
        if gap < MIN_GAP[method]:
            continue
        want[(method, dim)] -= 1
        problems.append(dict(method=method, dim=dim, N=N, n=n, length=length,
                             alpha=alpha, X=X.tolist(), picks=picks, gap=gap))
        print(f'{method:12s} dim {dim} N {N:3d} n {n:2d} l {length}: '
              f'min gap {gap:.2e}')

    drafts = []
    for method, N, n, seed, dim, length in [
            ('determinant', 300, 24, 7, 3, 0.3),
            ('variance', 300, 24, 8, 3, 0.3),
            ('determinant', 200, 40, 9, 1, 0.05),
            ('variance', 257, 17, 10, 3, 0.2)]:
        X = np.random.default_rng(seed).uniform(-1, 1, size=(N, dim))

        def kernel(Y, length=length):
            return rbf(Y, length)
        sel = DeterminantMaximizer(kernel) if method == 'determinant' else \
            VarianceMinimizer(kernel)
        picks = HierarchicalDrafter(sel)(X, n, random_state=seed)
        drafts.append(dict(method=method, dim=dim, N=N, n=n, length=length,
                           seed=seed, X=X.tolist(),
                           picks=[int(i) for i in picks]))
        print(f'drafter {method:12s} N {N} n {n}: {len(picks)} picks')

    with open(os.path.join(HERE, 'active_learning.json'), 'w') as f:
        json.dump(dict(min_gap=MIN_GAP, problems=problems, drafts=drafts), f)


if __name__ == '__main__':
    main()
