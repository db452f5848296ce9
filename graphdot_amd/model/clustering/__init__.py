"""Clustering on the kernel protocol: kernel k-means (Lloyd's iteration in
the feature space of the kernel) and HDBSCAN (density clustering on the
minimum spanning tree of the mutual-reachability graph); the reference has
neither."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .kkmeans import KernelKMeans
from .hdbscan import KernelHDBSCAN

__all__ = ['KernelKMeans', 'KernelHDBSCAN']
