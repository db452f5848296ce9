"""Graph distance metrics built on the marginalized graph kernel."""
from .maximin import MaxiMin
from ._kernel_induced import KernelInducedDistance

__all__ = ['MaxiMin', 'KernelInducedDistance']
