"""k-nearest-neighbour classification and regression of graphs under a kernel
(search.py has the distance and the order of the neighbours; DESIGN.md section
36): scikit-learn's `KNeighborsClassifier` and `KNeighborsRegressor` with
``metric='precomputed'`` on the feature-space distances.

A class probability is the weighted mean of the neighbours' one-hot labels, a
regression value the weighted mean of their targets, summed in rank order.
``weights='uniform'`` is 1, ``'distance'`` is 1 / d -- and where neighbours of
a sample lie at d == 0, exactly those get weight 1 and the rest 0
(scikit-learn's rule).  The predicted class is the first maximum of the
probabilities.

On the GPU the means are one more launch on the lists where the search left
them (`knn_average`), and the (b, m) means and the flag word are the one
download of a call."""
import numpy as np
from . import _knn
from .search import KernelNeighborsBase


def _torch():
    import torch
    return torch


class _KernelKNeighbors(KernelNeighborsBase):
    def __init__(self, kernel, n_neighbors=5, weights='uniform',
                 kernel_options=None, device='auto'):
        if weights not in _knn.WEIGHTS:
            raise ValueError(f'weights: one of {_knn.WEIGHTS} expected, got '
                             f'{weights!r}')
        self._init(kernel, n_neighbors, kernel_options, device)
        self.weights = weights

    def _fit_table(self, X, table):
        """Keep the (n, m) float64 table of what is averaged, where the
        matrix lies."""
        K, adopted, t_kernel = self._fit_matrix(X)
        if len(table) != self._n:
            raise ValueError(f'y: {self._n} rows expected, got {len(table)}')
        self._table = _torch().from_numpy(
            np.ascontiguousarray(table, dtype=np.float64)).to(K.device)
        self.last_timing = {
            'kernel': t_kernel, 'linalg': 0.0, 'adopted': adopted,
            'fused': _knn._declines(K, self.n_neighbors) is None}
        return self

    def _means(self, Z, diag):
        """(b, m) weighted means of the table over the neighbours of `Z` (of
        the training samples, each left out, for ``Z=None``)."""
        (d2, idx, flag), timing = self._lists(Z, diag)
        means, fused = _knn.mean(d2, idx, self._table, self.weights)
        timing['fused'] = timing['fused'] and fused
        return self._download(flag, means, timing=timing)[0]


class KernelKNeighborsClassifier(_KernelKNeighbors):
    """Classification of graphs by a vote of the k nearest training graphs
    under a kernel.

    Parameters
    ----------
    kernel, n_neighbors, kernel_options, device: as `KernelNearestNeighbors`
        (with a precomputed kernel the methods take the (b, n) cross matrix
        and ``diag=``, the (b,) self-similarities of the new samples).
    weights: 'uniform' or 'distance'.

    After `fit`: `classes_` (sorted), `last_timing`."""

    def fit(self, X, y):
        """`y`: one hashable label per sample."""
        y = y.tolist() if isinstance(y, np.ndarray) and y.ndim == 1 \
            else list(y)
        classes = sorted(set(y))
        code = {c: i for i, c in enumerate(classes)}
        self._codes = np.array([code[v] for v in y], dtype=np.int64)
        self.classes_ = np.empty(len(classes), dtype=object)
        self.classes_[:] = classes
        try:      # (plain numbers and strings: an array of their own type)
            plain = np.asarray(classes)
            if plain.ndim == 1 and plain.dtype != object:
                self.classes_ = plain
        except ValueError:
            pass
        onehot = np.zeros((len(y), len(classes)))
        onehot[np.arange(len(y)), self._codes] = 1.0
        return self._fit_table(X, onehot)

    def predict_proba(self, Z, diag=None):
        """(b, classes) probabilities of the graphs `Z`."""
        self._fitted('predict')
        return self._means(Z, diag)

    def predict(self, Z, diag=None):
        """(b,) the most probable class of each graph (the first on a
        tie)."""
        best = np.argmax(self.predict_proba(Z, diag), axis=1)
        return self.classes_[best]

    def score(self, Z, y, diag=None):
        """The accuracy of `predict(Z)` against the labels `y`."""
        got = self.predict(Z, diag)
        y = list(y)
        if len(y) != len(got):
            raise ValueError(f'y: {len(got)} labels expected, got {len(y)}')
        return float(np.mean([g == v for g, v in zip(got.tolist(), y)]))

    def loo_score(self):
        """The accuracy with every training sample predicted from the
        others."""
        got = np.argmax(self._means(None, None), axis=1)
        return float(np.mean(got == self._codes))


class KernelKNeighborsRegressor(_KernelKNeighbors):
    """Regression on graphs by the mean target of the k nearest training
    graphs under a kernel.

    Parameters: as `KernelKNeighborsClassifier`.  `y` is (n,) or (n, m), and
    the predictions have its shape."""

    def fit(self, X, y):
        y = np.asarray(y, dtype=np.float64)
        if y.ndim not in (1, 2):
            raise ValueError(f'y: (n,) or (n, m) expected, got {y.shape}')
        self._flat = y.ndim == 1
        self._y = y.reshape(len(y), -1)
        return self._fit_table(X, self._y)

    def _shaped(self, means):
        return means[:, 0] if self._flat else means

    def predict(self, Z, diag=None):
        """(b,) or (b, m) predictions for the graphs `Z`."""
        return self._shaped(self._means(Z, diag))

    @staticmethod
    def _r2(y, got):
        return float(1.0 - ((y - got) ** 2).sum()
                     / ((y - y.mean(0)) ** 2).sum())

    def score(self, Z, y, diag=None):
        """The coefficient of determination R^2 of `predict(Z)` against
        `y`."""
        got = self.predict(Z, diag)
        y = np.asarray(y, dtype=np.float64)
        if y.shape != got.shape:
            raise ValueError(f'y: {got.shape} expected, got {y.shape}')
        return self._r2(y, got)

    def loo_score(self):
        """R^2 with every training sample predicted from the others."""
        return self._r2(self._shaped(self._y),
                        self._shaped(self._means(None, None)))
