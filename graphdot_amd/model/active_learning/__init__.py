"""Active learning: greedy choice of the samples to label next from the
kernel matrix of a candidate pool; mirrors ``graphdot.model.active_learning``
of the reference (``DeterminantMaximizer``, ``VarianceMinimizer``,
``HierarchicalDrafter``).  On the GPU the greedy loops run on the kernel
matrix where it lies (select.hip); see DESIGN.md section 17."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from ._greedy import SelectionError
from .determinant_maximizer import DeterminantMaximizer
from .variance_minimizer import VarianceMinimizer
from .hierarchical_drafter import HierarchicalDrafter

__all__ = ['DeterminantMaximizer', 'VarianceMinimizer', 'HierarchicalDrafter',
           'SelectionError']
