"""Non-linear maps of graphs on the kernel protocol: exact t-SNE under the
kernel's feature-space distance, descended on the kernel matrix where it lies,
and Isomap on the geodesic distances of its neighbourhood graph (the reference
has neither model)."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .tsne import KernelTSNE
from .isomap import KernelIsomap

__all__ = ['KernelTSNE', 'KernelIsomap']
