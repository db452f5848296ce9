"""Monte Carlo tree search towards a target value of a predicted property.

The interface and the numbers are those of the reference's
`MCTSGraphTransformer`; the formulation is this module's.  One iteration

1. walks from the root to a leaf, at every level to the sibling with the
   largest `score` (the first of equals), counting a visit on the way and
   remembering the path;
2. lets the rewriter derive the leaf's offspring and the surrogate predict
   mean and standard deviation of each;
3. walks the remembered path back up: every node on it takes the
   inverse-variance weighted mean of its children's `tree_mean` as its
   `tree_mean` and the equally weighted spread of those means around it as
   its `tree_std`, and its children are scored anew:

       score = N(target; tree_mean, max(tree_std, precision))
               + exploration_bias * sqrt(log(visits of the parent) / visits)

Nothing guards the weights: a node whose children all agree gets
`tree_std = 0` and with it an infinite weight one level up, as in the
reference.
"""
import math

import numpy as np

from ...util.iterable import argmax
from ._tree import Tree

#: `device='auto'`, from the measurements of DESIGN.md section 23 (MI355X,
#: 250 to 4000 training graphs, 1, 5 and 10 candidates): a prediction goes
#: through the `DevicePosterior` from `AUTO_MIN_TRAINING_SIZE` usable
#: training samples on whatever the number of candidates, and from
#: `AUTO_MIN_TRAINING_SIZE_MANY` on when there are at least
#: `AUTO_MANY_CANDIDATES` of them; a single candidate against fewer than 1000
#: graphs was no faster on the device, and nothing below 250 was measured
AUTO_MIN_TRAINING_SIZE = 1000
AUTO_MIN_TRAINING_SIZE_MANY = 250
AUTO_MANY_CANDIDATES = 5


class _BySize:
    """`predict` through the device posterior or the regressor itself,
    whichever the measurements favour for this many candidates."""

    def __init__(self, posterior):
        self.posterior = posterior

    def predict(self, Z, **kwargs):
        gpr = self.posterior.gpr
        n = len(gpr.Kinv)
        on_device = n >= AUTO_MIN_TRAINING_SIZE or (
            n >= AUTO_MIN_TRAINING_SIZE_MANY
            and len(Z) >= AUTO_MANY_CANDIDATES)
        return (self.posterior if on_device else gpr).predict(Z, **kwargs)

_SQRT_2PI = math.sqrt(2.0 * math.pi)


class MCTSGraphTransformer:
    """A variant of Monte Carlo tree search for optimisation and root-finding
    in a space of graphs.

    Parameters
    ----------
    rewriter: callable
        ``rewriter(node, rng)`` returns a list of graphs derived from
        ``node.g`` (`AbstractRewriter`).
    surrogate: object
        The predictor of the target property.  A regressor of this package
        is asked for ``predict(graphs, return_std=True)``, any other object
        for ``predict(graphs, return_cov=True)``.
    exploration_bias: float
        Weight of the exploration term of the score.
    precision: float
        Target precision of the outcome: the floor of the standard deviation
        in the likelihood of the target.
    device: 'auto', 'cuda' or 'cpu'
        Where a `GaussianProcessRegressor` predicts: 'cuda' keeps its
        posterior on the device (`DevicePosterior`) and raises if that is not
        possible, 'cpu' calls the regressor as it is, 'auto' takes the device
        where it is available and was measured to be no slower
        (`AUTO_MIN_TRAINING_SIZE` and its companions).
    """

    def __init__(self, rewriter, surrogate, exploration_bias=1.0,
                 precision=0.01, device='auto'):
        if device not in ('auto', 'cuda', 'cpu'):
            raise ValueError(f'device={device!r}: "auto", "cuda" or "cpu"')
        self.rewriter = rewriter
        self.surrogate = surrogate
        self.exploration_bias = exploration_bias
        self.precision = precision
        self.device = device
        self._posterior = None

    # -- the surrogate ----------------------------------------------------------
    def _device_posterior(self, gpr):
        from ..gaussian_process import DevicePosterior
        if self._posterior is None or self._posterior.gpr is not gpr:
            self._posterior = DevicePosterior(gpr)
        self._posterior._current()
        return self._posterior

    def _predictor(self):
        """(object to call `predict` on, whether it takes `return_std`)."""
        from ..gaussian_process import (
            GaussianProcessRegressor, LowRankApproximateGPR,
            GPROutlierDetector, DevicePosterior)
        model = self.surrogate
        if not isinstance(model, GaussianProcessRegressor):
            return model, isinstance(model, (
                DevicePosterior, LowRankApproximateGPR, GPROutlierDetector))
        if self.device == 'cuda':
            posterior = self._device_posterior(model)
            if not posterior.available:
                raise RuntimeError(
                    'device="cuda": the posterior of this regressor cannot '
                    'be kept on the device (CUDA algebra, no kernel_options '
                    'and a kernel with device_cross_gram and device_diag are '
                    'needed)')
            return posterior, True
        # 'auto': nothing is uploaded or probed for a training set below the
        # smallest size at which the device path pays
        if self.device == 'auto' and hasattr(model, 'Kinv') \
                and len(model.Kinv) >= AUTO_MIN_TRAINING_SIZE_MANY:
            posterior = self._device_posterior(model)
            if posterior.available:
                return _BySize(posterior), True
        return model, True

    def _evaluate(self, nodes):
        """Predict the siblings of `nodes` and count their first visit."""
        model, takes_std = getattr(self, '_predict', None) \
            or self._predictor()
        if takes_std:
            mean, std = model.predict(nodes.g, return_std=True)
        else:
            mean, cov = model.predict(nodes.g, return_cov=True)
            std = np.sqrt(np.diagonal(cov))
        for column, values in (('self_mean', mean), ('tree_mean', mean),
                               ('self_std', std), ('tree_std', std)):
            nodes[column] = np.array(values, dtype=float)
        nodes['score'] = np.zeros(len(nodes))
        nodes['visits'] = np.asarray(nodes.visits) + 1

    # -- scores -----------------------------------------------------------------------
    def _likelihood(self, target, nodes):
        """Density of `target` under each node's N(tree_mean, tree_std), the
        standard deviation floored at `precision`."""
        sigma = np.maximum(np.asarray(nodes.tree_std, dtype=float),
                           self.precision)
        z = (target - np.asarray(nodes.tree_mean, dtype=float)) / sigma
        return np.exp(-0.5 * z * z) / (sigma * _SQRT_2PI)

    def _score(self, target, nodes, parent_visits):
        explore = np.sqrt(math.log(parent_visits)
                          / np.asarray(nodes.visits, dtype=float))
        return self._likelihood(target, nodes) \
            + self.exploration_bias * explore

    @staticmethod
    def _best_child(children):
        """The sibling with the largest score; the first wins ties."""
        return argmax(children.iternodes(), lambda a, b: a.score < b.score)

    # -- the search ----------------------------------------------------------------------
    def _siblings(self, parent, graphs):
        n = len(graphs)
        return Tree(parent=[parent] * n, children=[None] * n, g=graphs,
                    visits=np.zeros(n, dtype=int))

    def _iterate(self, root, target, rng):
        # 1. down to a leaf
        node = next(root.iternodes())
        path = [node]
        while node.children is not None:
            node.visits += 1
            node = self._best_child(node.children)
            path.append(node)
        node.visits += 1
        # 2. offspring of the leaf
        node.children = self._siblings(node, self.rewriter(node, rng))
        self._evaluate(node.children)
        # 3. back up
        for node in reversed(path):
            kids = node.children
            means = np.asarray(kids.tree_mean, dtype=float)
            weights = 1.0 / np.square(np.asarray(kids.tree_std, dtype=float))
            total = weights.sum()
            centre = (means * weights).sum() / total
            node.tree_mean = centre
            node.tree_std = math.sqrt(
                (np.square(means - centre) * weights).sum() / total)
            kids['score'] = self._score(target, kids, node.visits)

    def seek(self, g0, target, maxiter=500, return_tree=False,
             random_state=None):
        """Search, from `g0`, for a graph whose predicted property is
        `target`.

        Parameters
        ----------
        g0: object
            The graph at the root of the search tree.
        target: float
            The wanted value of the property.
        maxiter: int
            Iterations, i.e. expanded nodes.
        return_tree: bool
            Return the `Tree` itself instead of a table of its nodes.
        random_state: int or np.random.Generator
            Seed of the generator handed to the rewriter, or the generator.

        Returns
        -------
        The `Tree` if `return_tree`; otherwise a pandas DataFrame with one
        row per node (`Tree.flat` plus a `likelihood` column), the most
        likely node first.
        """
        # (an int seeds PCG64, a Generator is passed through, None is entropy)
        rng = np.random.default_rng(random_state)
        self._predict = self._predictor()
        root = self._siblings(None, [g0])
        self._evaluate(root)
        for _ in range(maxiter):
            self._iterate(root, target, rng)
        if return_tree is True:
            return root
        table = root.flat
        table['likelihood'] = self._likelihood(target, table)
        return table.to_pandas().sort_values(
            by='likelihood', ascending=False)
