"""Unsupervised decompositions on the kernel protocol: kernel principal
component analysis (the meaning of scikit-learn's ``KernelPCA``; the
reference has none)."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .kpca import KernelPCA

__all__ = ['KernelPCA']
