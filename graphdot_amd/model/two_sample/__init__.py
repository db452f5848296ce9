"""The kernel two-sample test on the kernel protocol: the maximum mean
discrepancy of two sets of graphs, its permutation null distribution and its
witness function, summed on the Gram matrix of the pooled sample where it lies
(the reference has none)."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .mmd import KernelTwoSampleTest

__all__ = ['KernelTwoSampleTest']
