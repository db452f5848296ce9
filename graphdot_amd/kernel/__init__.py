"""Graph kernels: the marginalized graph kernel (the hot path), the kernel
transformers of ``fix``, the ready-made molecular kernel and kernels over a
distance (`KernelOverMetric`)."""
# (the device-path protocol's exception: not one of the reference's names)
from ._device_path import NoDevicePath       # noqa: F401
from .molecular import Tang2019MolecularKernel
from ._kernel_over_metric import KernelOverMetric
from .marginalized import MarginalizedGraphKernel

__all__ = [
    'Tang2019MolecularKernel', 'KernelOverMetric', 'MarginalizedGraphKernel'
]
