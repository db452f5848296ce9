"""Rules that turn interatomic distances into edge weights (reference:
``graphdot/graph/adjacency``): the distance shapes of ``euclidean`` and the
element-aware ``AtomicAdjacency`` that `Graph.from_ase` uses."""
from .atomic import AtomicAdjacency
from .euclidean import Gaussian, Tent, CompactBell

__all__ = [
    'Gaussian',
    'Tent',
    'CompactBell',
    'AtomicAdjacency',
]
