"""Gaussian process regression on the kernel protocol; mirrors
``graphdot.model.gaussian_process`` of the reference for the exact and the
Nystrom low-rank regressor and the outlier detector; the binary classifier
(Laplace approximation) follows scikit-learn, the reference has none."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .gpr import GaussianProcessRegressor
from .nystrom import LowRankApproximateGPR
from .outlier_detector import GPROutlierDetector
from ._device_posterior import DevicePosterior
from .gpc import GaussianProcessClassifier

__all__ = ['GaussianProcessRegressor', 'LowRankApproximateGPR',
           'GPROutlierDetector', 'DevicePosterior',
           'GaussianProcessClassifier']
