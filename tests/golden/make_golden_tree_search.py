#!/usr/bin/env python
"""Golden search trees of the reference's MCTSGraphTransformer
(graphdot/model/tree_search).  Needs a checkout of the reference
(make_golden.REF); the test-suite only reads tree_search.json and imports the
problem definitions below (kernels, rewriters, data), which do not touch the
reference.

The reference is imported under the shim of make_golden.py plus two stand-ins
that leave its own text untouched: a `treelib` module whose `Tree` is `object`
(treelib is not a dependency of this project; the transformer does not use
it), and the node view's `__getattr__` wrapped so that the lookup of a
`__dunder__` name raises AttributeError (numpy 2 probes `__array_struct__` on
the views when the reference stores them in a column; the reference answers
KeyError).  Nothing of the reference is copied: inputs, seeds and the trees it
builds are recorded.

Problems
  scalar: 13 points of sin(x) + x / 3 on [-3, 3] under the RBF kernel of
      width 0.5 with the reference's host GPR (the shape of the reference's
      example/mcts.py), alpha = 1e-4; children are the parent plus normal
      steps, so that they stay off the training points; `precision` (the
      floor of the standard deviation in the likelihood) is 0.3, so that the
      likelihood of the target does not underflow and the scores of siblings
      differ by more than their exploration terms.
  graph: a pool of small labelled graphs (tests/cases.py) under the
      marginalized graph kernel evaluated by the oracle (oracle/mgk.py) with
      the reference's host GPR trained on the first graphs of the pool; a node
      holds the index of a graph, its children are indices drawn from the
      rest of the pool.

A case is kept only if the tree holds no NaN, no infinity and no zero
`tree_std`, and if the best and the second-best `score` differ at every
selection among siblings by at least `MIN_GAP`; rejected seeds are listed with
the reason.  `observed_disagreement` is the largest relative difference of any
float column between the reference's tree and this project's on the same
problem (float64, CPU), measured by this script: `MIN_GAP` lies orders of
magnitude above it, so both implementations select the same nodes.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

MIN_GAP = 1e-6
FLOAT_COLUMNS = ('self_mean', 'self_std', 'tree_mean', 'tree_std', 'score',
                 'likelihood')
ALPHA = 1e-4


# -- problem definitions (shared with tests/test_tree_search.py) -----------------
class RBF:
    """exp(-(x - y)^2 / (2 l^2)) on scalars."""

    def __init__(self, length):
        self.length = length

    def __call__(self, X, Y=None):
        X = np.asarray(X, dtype=np.float64)
        Y = X if Y is None else np.asarray(Y, dtype=np.float64)
        return np.exp(-0.5 * (X[:, None] - Y[None, :])**2 / self.length**2)

    def diag(self, X):
        return np.ones(len(X))


def scalar_problem():
    X = np.linspace(-3, 3, 13)
    return X, np.sin(X) + X / 3


class NormalSteps:
    """Children of a scalar: the parent plus `b` normal steps."""

    def __init__(self, b, width):
        self.b, self.width = b, width

    def __call__(self, node, rng):
        return list(float(node.g) + rng.normal(0.0, self.width, self.b))


SCALAR_CASES = [
    # (seed, g0, target, maxiter, b, step width, exploration bias)
    dict(seed=s, g0=g0, target=t, maxiter=15, b=4, width=w, bias=eb,
         precision=0.3)
    for s, g0, t, w, eb in [
        (0, 0.3, 1.2, 0.5, 1.0), (1, -1.1, 0.4, 0.5, 1.0),
        (2, 2.2, -0.9, 0.4, 0.5), (3, 0.0, 1.0, 0.6, 2.0),
        (4, -2.0, 0.0, 0.5, 1.0), (5, 1.4, 1.6, 0.3, 1.0),
        (6, -0.4, -1.3, 0.5, 1.5), (7, 0.8, 0.2, 0.5, 1.0)]]

N_POOL, N_TRAIN = 24, 10


def graph_pool():
    import cases
    return cases.config2_graphs(N_POOL, nmin=6, nmax=12, seed=11)


def graph_targets(pool):
    """A property known in closed form: node count plus mean degree."""
    return np.array([len(g.nodes) + 2.0 * len(g.edges) / len(g.nodes)
                     for g in pool])


class PoolKernel:
    """The marginalized graph kernel between graphs given by their index in
    the pool: the pool's Gram matrix by the oracle, normalised, looked up."""

    def __init__(self, pool):
        import cases
        from oracle import mgk
        knode, kedge, q = cases.config2a_kernels()
        K = mgk.gram(pool, knode, kedge, q=q)
        d = np.sqrt(np.diag(K))
        self.K = K / d[:, None] / d[None, :]

    def __call__(self, X, Y=None):
        i = np.asarray(X, dtype=int)
        j = i if Y is None else np.asarray(Y, dtype=int)
        return self.K[i][:, j]

    def diag(self, X):
        return self.K.diagonal()[np.asarray(X, dtype=int)]


class PoolDraws:
    """Children of a pool index: `b` distinct indices of graphs outside the
    training set, other than the parent."""

    def __init__(self, b):
        self.b = b

    def __call__(self, node, rng):
        rest = [i for i in range(N_TRAIN, N_POOL) if i != int(node.g)]
        return [int(i) for i in rng.choice(rest, size=self.b, replace=False)]


GRAPH_CASES = [
    dict(seed=s, g0=g0, target=t, maxiter=10, b=3, bias=eb, precision=1.0)
    for s, g0, t, eb in [(0, 12, 9.0, 1.0), (1, 15, 7.5, 1.0),
                         (2, 20, 10.5, 0.5), (3, 11, 8.0, 2.0)]]


def walk(transformer, tree, target, level=0):
    """Depth-first rows of a search tree, floats in full precision."""
    like = transformer._likelihood(target, tree)
    for i in range(len(tree)):
        row = dict(level=level, g=tree.g[i].item(), visits=int(tree.visits[i]),
                   likelihood=float(like[i]))
        for c in FLOAT_COLUMNS[:-1]:
            row[c] = float(tree[c][i])
        yield row
        if tree.children[i] is not None:
            yield from walk(transformer, tree.children[i], target, level + 1)


# -- the reference ---------------------------------------------------------------------
def install_stand_ins():
    tl = types.ModuleType('treelib')
    tl.Tree = object
    sys.modules['treelib'] = tl


def main():
    import make_golden as mg
    mg.install_shims()
    install_stand_ins()
    sys.path.insert(0, mg.REF)
    from graphdot.model.gaussian_process import GaussianProcessRegressor
    from graphdot.model.tree_search import MCTSGraphTransformer
    from graphdot.model.tree_search import graph_transformer as ref_gt
    from graphdot.model.tree_search._tree import Tree as RefTree
    import graphdot_amd.model.tree_search as ours
    from graphdot_amd.model.gaussian_process import \
        GaussianProcessRegressor as OurGPR

    inner = RefTree.NodeView.__getattr__

    def getattr_(self, key):
        if key.startswith('__') and key.endswith('__'):
            raise AttributeError(key)
        return inner(self, key)
    RefTree.NodeView.__getattr__ = getattr_

    gaps = []
    ref_argmax = ref_gt.argmax

    def recording_argmax(iterable, less):
        nodes = list(iterable)
        scores = sorted((float(n.score) for n in nodes), reverse=True)
        if len(scores) > 1:
            gaps.append(scores[0] - scores[1])
        return ref_argmax(nodes, less)
    ref_gt.argmax = recording_argmax

    def run(kind, case, kernel, X, y, rewriter):
        gaps.clear()
        ref = GaussianProcessRegressor(kernel, alpha=ALPHA)
        ref.fit(X, y)
        t = MCTSGraphTransformer(rewriter, ref, exploration_bias=case['bias'],
                                 precision=case['precision'])
        with np.errstate(all='ignore'):
            tree = t.seek(case['g0'], case['target'], maxiter=case['maxiter'],
                          return_tree=True, random_state=case['seed'])
        rows = list(walk(t, tree, case['target']))
        flat = np.array([[r[c] for c in FLOAT_COLUMNS] for r in rows])
        if not np.isfinite(flat).all():
            return None, 'NaN or infinity in the tree'
        if min(r['tree_std'] for r in rows) == 0:
            return None, 'zero tree_std'
        gap = min(gaps) if gaps else float('inf')
        if gap < MIN_GAP:
            return None, f'score gap {gap:.3g} below MIN_GAP'
        mine = OurGPR(kernel, alpha=ALPHA, device='cpu')
        mine.fit(X, y)
        t2 = ours.MCTSGraphTransformer(rewriter, mine, device='cpu',
                                       exploration_bias=case['bias'],
                                       precision=case['precision'])
        tree2 = t2.seek(case['g0'], case['target'], maxiter=case['maxiter'],
                        return_tree=True, random_state=case['seed'])
        rows2 = list(walk(t2, tree2, case['target']))
        same = len(rows) == len(rows2) and all(
            (a['level'], a['g'], a['visits']) == (b['level'], b['g'],
                                                  b['visits'])
            for a, b in zip(rows, rows2))
        if not same:
            raise SystemExit(f'{kind} seed {case["seed"]}: the two '
                             'implementations build different trees')
        flat2 = np.array([[r[c] for c in FLOAT_COLUMNS] for r in rows2])
        dis = float(np.max(np.abs(flat2 - flat)
                           / np.maximum(np.abs(flat), 1e-300)))
        return dict(case, kind=kind, rows=rows, min_gap=gap), dis

    out = {'MIN_GAP': MIN_GAP, 'alpha': ALPHA, 'cases': [], 'rejected': []}
    worst = 0.0
    X, y = scalar_problem()
    pool = graph_pool()
    pk = PoolKernel(pool)
    for kind, todo in (('scalar', SCALAR_CASES), ('graph', GRAPH_CASES)):
        for case in todo:
            if kind == 'scalar':
                res, info = run(kind, case, RBF(0.5), X, y,
                                NormalSteps(case['b'], case['width']))
            else:
                res, info = run(kind, case, pk, np.arange(N_TRAIN),
                                graph_targets(pool)[:N_TRAIN],
                                PoolDraws(case['b']))
            if res is None:
                out['rejected'].append(dict(kind=kind, seed=case['seed'],
                                            reason=info))
            else:
                out['cases'].append(res)
                worst = max(worst, info)
    out['observed_disagreement'] = worst
    kept = [c['kind'] for c in out['cases']]
    assert kept.count('scalar') >= 4 and kept.count('graph') >= 2, kept
    assert worst * 1e3 < MIN_GAP, worst
    with open(os.path.join(HERE, 'tree_search.json'), 'w') as f:
        json.dump(mg.jsonable(out), f)
    print('tree_search.json:', kept, 'rejected', out['rejected'],
          'disagreement %.2e' % worst)


if __name__ == '__main__':
    main()
