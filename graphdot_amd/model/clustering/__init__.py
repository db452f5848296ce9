"""Clustering on the kernel protocol: kernel k-means (Lloyd's iteration in
the feature space of the kernel; the reference has none)."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .kkmeans import KernelKMeans

__all__ = ['KernelKMeans']
