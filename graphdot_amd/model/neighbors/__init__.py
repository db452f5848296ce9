"""Nearest neighbours in the feature space of a kernel, on the kernel
protocol: the search, the k-nearest-neighbour classifier and regressor and the
local outlier factor, selected on the kernel matrix where it lies (the
reference has the distance, `KernelInducedDistance`, and none of the
models)."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .search import KernelNearestNeighbors, device_lists
from .knn import KernelKNeighborsClassifier, KernelKNeighborsRegressor
from .lof import KernelLocalOutlierFactor

__all__ = ['KernelNearestNeighbors', 'KernelKNeighborsClassifier',
           'KernelKNeighborsRegressor', 'KernelLocalOutlierFactor',
           'device_lists']
