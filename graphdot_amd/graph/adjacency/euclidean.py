"""Convert spatial distances between nodes to edge adjacencies (reference:
``graphdot/graph/adjacency/euclidean.py``).

Every shape is a callable ``shape(d, length_scale)`` with a ``cutoff``.  On
scalars it is the reference's function: 0 beyond the cutoff.  On arrays (either
argument) it evaluates element-wise with the same operations in the same
order, so both paths give the same numbers -- `Graph.from_ase` uses the array
form on all candidate pairs at once.
"""
import math
import numpy as np

#: element-wise C-library pow: numpy's vectorised power of an array need not
#: round like the scalar pow the reference's shapes call (observed: 1 ulp)
_pow = np.frompyfunc(math.pow, 2, 1)


def _power(s, e):
    """s ** e element-wise with the rounding of the scalar s ** e."""
    if e in (1, 2):          # (exact either way)
        return s ** e
    return _pow(s, float(e)).astype(np.float64)


def _is_scalar(d, length_scale):
    return np.ndim(d) == 0 and np.ndim(length_scale) == 0


class Gaussian:
    def __call__(self, d, length_scale):
        return np.exp(-0.5 * d**2 / length_scale**2)

    def cutoff(self, length_scale):
        return np.inf


class Tent:
    def __init__(self, ord):
        assert ord >= 1
        self.ord = ord

    def __call__(self, d, length_scale):
        s = 1 - d / self.cutoff(length_scale)
        if _is_scalar(d, length_scale):
            return s ** self.ord if s >= 0 else 0
        s = np.asarray(s, dtype=np.float64)
        return np.where(s >= 0, _power(s, self.ord), 0.0)

    def cutoff(self, length_scale):
        return length_scale * 3


class CompactBell:
    def __init__(self, a, b):
        assert a > b and b >= 2
        self.a = a
        self.b = b

    def _bell(self, s, power=lambda s, e: s**e):
        return (-self.b * power(s, self.a) + self.a * power(s, self.b)) / (
            self.a - self.b)

    def __call__(self, d, length_scale):
        s = 1 - d / self.cutoff(length_scale)
        if _is_scalar(d, length_scale):
            return self._bell(s) if s >= 0 else 0
        s = np.asarray(s, dtype=np.float64)
        return np.where(s >= 0, self._bell(s, _power), 0.0)

    def cutoff(self, length_scale):
        return length_scale * 3
