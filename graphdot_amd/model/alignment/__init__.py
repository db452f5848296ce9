"""Centred kernel-target alignment on the kernel protocol: the alignment of a
kernel with labels or regression targets and its gradient, summed on the Gram
matrix and the gradient planes where they lie, and the hyperparameters that
maximise it (the reference has none)."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .kta import KernelTargetAlignment

__all__ = ['KernelTargetAlignment']
