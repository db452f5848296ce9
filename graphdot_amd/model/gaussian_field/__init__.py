"""Gaussian field regression (semi-supervised label propagation); mirrors
``graphdot.model.gaussian_field`` of the reference."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .gfr import GaussianFieldRegressor
from .weight import Weight, RBFOverDistance, RBFOverFixedDistance

__all__ = ['GaussianFieldRegressor', 'Weight', 'RBFOverDistance',
           'RBFOverFixedDistance']
