"""Support vector machines on the kernel protocol: C-support vector
classification, epsilon-support vector regression and the one-class machine
by SMO on the Gram matrix where it lies (the reference has none)."""
try:      # torch's HIP runtime must be initialised before libgdhip's
    import torch as _torch   # (graphdot_amd.hip.runtime, _let_torch_initialise_first)
    _torch.cuda.is_available()
except ImportError:          # pragma: no cover
    pass
from .svc import KernelSVC
from .svr import KernelOneClassSVM, KernelSVR

__all__ = ['KernelSVC', 'KernelSVR', 'KernelOneClassSVM']
