"""The local outlier factor of graphs under a kernel (Breunig, Kriegel, Ng and
Sander, "LOF: identifying density-based local outliers", SIGMOD 2000; search.py
has the distance and the order of the neighbours): the
density-based counterpart of `GPROutlierDetector` and `KernelOneClassSVM`,
meaning what scikit-learn's ``LocalOutlierFactor(novelty=True,
metric='precomputed')`` means on the feature-space distances.

With the lists of the k nearest training samples of sample i (itself left out
for a training sample), ``kdist[j]`` the k-th distance of training sample j,

    lrd[i] = 1 / (mean_r max(kdist[idx[i][r]], d[i][r]) + 1e-10)
    lof[i] = mean_r (lrd_train[idx[i][r]] / lrd[i])

and the scores are ``-lof``: near -1 for inliers, far below for outliers.

On the GPU `fit` is the search and two launches on its lists (`knn_lrd`,
`knn_ratio`) with one download of the n scores and the flag word; the k-th
distances and the densities stay on the device for `score_samples`."""
import time
import warnings
import numpy as np
from . import _knn
from .search import KernelNeighborsBase


def _torch():
    import torch
    return torch


class KernelLocalOutlierFactor(KernelNeighborsBase):
    """Outlier scores of graphs from the density of their neighbourhoods.

    Parameters
    ----------
    kernel, kernel_options, device: as `KernelNearestNeighbors` (with a
        precomputed kernel the methods take the (b, n) cross matrix and
        ``diag=``, the (b,) self-similarities of the new samples).
    n_neighbors: int; clipped to n - 1, with a warning.
    contamination: 'auto' (`offset_` = -1.5) or the share of outliers in the
        training set, in (0, 0.5]: `offset_` is that percentile of the
        training scores.

    After `fit`: `negative_outlier_factor_` (n,), `offset_`, `n_neighbors_`,
    `last_timing`.  `score_samples`, `decision_function` and `predict` are for
    new samples, not for members of the training set (whose scores are
    `negative_outlier_factor_`)."""

    def __init__(self, kernel, n_neighbors=20, contamination='auto',
                 kernel_options=None, device='auto'):
        if contamination != 'auto' and not 0.0 < contamination <= 0.5:
            raise ValueError("contamination: 'auto' or a number in (0, 0.5] "
                             f'expected, got {contamination!r}')
        self._init(kernel, n_neighbors, kernel_options, device)
        self.contamination = contamination

    def fit(self, X):
        """Score the graphs (or the samples of the precomputed kernel
        matrix) `X` against each other."""
        torch = _torch()
        K, adopted, t_kernel = self._fit_matrix(X)
        n = self._n
        if n < 2:
            raise ValueError(f'{self._name}: at least two samples expected')
        if self.n_neighbors > n - 1:
            warnings.warn(
                f'n_neighbors ({self.n_neighbors}) is greater than the '
                f'total number of samples ({n}); n_neighbors will be set to '
                f'(n_samples - 1) for estimation', UserWarning)
        self.n_neighbors_ = k = min(self.n_neighbors, n - 1)
        timing = {'kernel': t_kernel, 'adopted': adopted,
                  'start': time.perf_counter()}
        (d2, idx, flag), fused = self._own_lists(K, k)
        kdist = torch.sqrt(d2[:, k - 1]).contiguous()
        (lof, own), fused2 = _knn.factors(d2, idx, kdist)
        timing['fused'] = fused and fused2
        self._kdist, self._lrd = kdist, own
        self.negative_outlier_factor_ = -self._download(
            flag, lof, timing=timing)[0]
        self.offset_ = -1.5 if self.contamination == 'auto' else float(
            np.percentile(self.negative_outlier_factor_,
                          100.0 * self.contamination))
        return self

    def fit_predict(self, X):
        """(n,) +1 for the inliers of `X`, -1 for its outliers."""
        self.fit(X)
        return np.where(self.negative_outlier_factor_ < self.offset_, -1, 1)

    def score_samples(self, Z, diag=None):
        """(b,) the negated local outlier factors of the new graphs `Z`."""
        if not hasattr(self, '_lrd'):
            raise ValueError(f'{self._name}: score_samples before fit')
        if Z is None:
            raise ValueError(f'{self._name}: score_samples is for new '
                             'samples; see negative_outlier_factor_')
        (d2, idx, flag), timing = self._lists(Z, diag, self.n_neighbors_)
        (lof, _), fused = _knn.factors(d2, idx, self._kdist, self._lrd)
        timing['fused'] = timing['fused'] and fused
        return -self._download(flag, lof, timing=timing)[0]

    def decision_function(self, Z, diag=None):
        """`score_samples` shifted by `offset_`: negative for outliers."""
        return self.score_samples(Z, diag) - self.offset_

    def predict(self, Z, diag=None):
        """(b,) +1 for inliers among the new graphs `Z`, -1 for outliers."""
        return np.where(self.decision_function(Z, diag) < 0, -1, 1)
