"""Element-aware adjacency between atoms (reference:
``graphdot/graph/adjacency/atomic.py``).

The reference reads its length scales from a column of mendeleev's element
table.  That package is not a dependency here: the ``vdw_radius`` column is
shipped as `VDW_RADIUS_PM` below, and any other length scale is passed as a
number, a mapping ``{atomic number: Angstrom}`` or an array indexed by atomic
number.
"""
import re
import numpy as np
from .euclidean import Tent, Gaussian, CompactBell

#: Chemical symbols by atomic number (index 0 unused).
SYMBOLS = (
    'X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co '
    'Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te '
    'I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir '
    'Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No '
    'Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og'
).split()

#: Length of the reference's table: atomic numbers 0..118.
N_TABLE = 119

#: Van der Waals radii in pm of the main-group elements, the consistent set of
#: M. Mantina, A. C. Chamberlin, R. Valero, C. J. Cramer and D. G. Truhlar,
#: J. Phys. Chem. A 113, 5806-5812 (2009), Table 12 (Bondi's radii, with
#: H = 110 pm from Rowland and Taylor).  This is the set mendeleev documents
#: for its `vdw_radius` column.  Elements without an entry have no radius here
#: and raise when used (see `AtomicAdjacency`).
VDW_RADIUS_PM = {
    1: 110, 2: 140,
    3: 181, 4: 153, 5: 192, 6: 170, 7: 155, 8: 152, 9: 147, 10: 154,
    11: 227, 12: 173, 13: 184, 14: 210, 15: 180, 16: 180, 17: 175, 18: 188,
    19: 275, 20: 231, 31: 187, 32: 211, 33: 185, 34: 190, 35: 183, 36: 202,
    37: 303, 38: 249, 49: 193, 50: 217, 51: 206, 52: 206, 53: 198, 54: 216,
    55: 343, 56: 268, 81: 196, 82: 202, 83: 207, 84: 197, 85: 202, 86: 220,
    87: 348, 88: 283,
}


def _vdw_table():
    pm = np.full(N_TABLE, np.nan)
    for z, r in VDW_RADIUS_PM.items():
        pm[z] = r
    return pm * 0.01    # pm to A, as the reference converts


def _table_from(length_scale):
    if isinstance(length_scale, str):
        if length_scale != 'vdw_radius':
            raise ValueError(
                f'Length scale column {length_scale!r} is not available: '
                'only the vdw_radius table is shipped.  Pass a number, a '
                'mapping {atomic number: Angstrom} or an array indexed by '
                'atomic number instead.')
        return _vdw_table()
    if isinstance(length_scale, dict):
        table = np.full(N_TABLE, np.nan)
        for z, r in length_scale.items():
            table[int(z)] = float(r)
        return table
    if np.ndim(length_scale) == 0:
        return length_scale * np.ones(N_TABLE)
    table = np.array(length_scale, dtype=np.float64)
    if table.ndim != 1:
        raise ValueError('length_scale arrays are indexed by atomic number')
    return table


class AtomicAdjacency:
    r"""Converts interatomic distances into edge weights using the equation
    :math:`a(i, j) = w(\frac{\lVert\mathbf{r}_{ij}\rVert}{\sigma_{ij}})`,
    where :math:`w` is a weight function that generally decays with distance,
    and :math:`\sigma_{ij} = \sqrt{\sigma_i \sigma_j}` is a length scale
    between atoms :math:`i` and :math:`j`.

    Parameters
    ----------
    shape: str or callable
        ``tent[n]`` (:py:class:`Tent`), ``gaussian`` (:py:class:`Gaussian`)
        or ``compactbell[a,b]`` (:py:class:`CompactBell`), or a shape object.
    length_scale: 'vdw_radius', number, mapping or array
        Per-element length scales in Angstrom: the shipped van der Waals
        radii (default), one number for every element, a mapping
        ``{atomic number: Angstrom}``, or an array indexed by atomic number.
        Other mendeleev column names raise ValueError.
    zoom: float
        A factor multiplied with the length scales.
    """

    def __init__(self, shape='tent1', length_scale='vdw_radius', zoom=1.0):
        if isinstance(shape, str):
            self.shape = self._parse_shape(shape)
        else:
            self.shape = shape
        self.ltable = _table_from(length_scale)
        self.ltable *= zoom

    @staticmethod
    def _parse_shape(shape):
        if shape == 'gaussian':
            return Gaussian()

        m = re.match(r'tent(\d+)', shape)
        if m:
            return Tent(ord=int(m.group(1)))

        m = re.match(r'compactbell(\d+),(\d+)', shape)
        if m:
            return CompactBell(a=int(m.group(1)), b=int(m.group(2)))

        raise ValueError(f'Unrecognizable adjacency shape: {shape}')

    def length_scales(self, elements):
        """Length scales of the atomic numbers `elements` (scalar or array);
        ValueError if some element has none."""
        z = np.asarray(elements, dtype=np.int64)
        if np.any((z < 0) | (z >= len(self.ltable))):
            bad = int(z[(z < 0) | (z >= len(self.ltable))].ravel()[0])
            raise ValueError(f'No length scale for atomic number {bad}')
        ls = self.ltable[z]
        missing = np.isnan(ls)
        if np.any(missing):
            bad = int(np.asarray(z)[missing].ravel()[0])
            name = SYMBOLS[bad] if 0 < bad < len(SYMBOLS) else str(bad)
            raise ValueError(
                f'No length scale for element {name} (Z = {bad}) in the '
                'van der Waals radius table; pass length_scale as a number, '
                'a mapping {atomic number: Angstrom} or an array indexed by '
                'atomic number.')
        return ls

    def __call__(self, n1, n2, r):
        """Adjacency between atoms of atomic numbers n1, n2 at distance r: a
        non-negative weight.  Scalars give a scalar; arrays broadcast."""
        r1 = self.length_scales(n1)
        r2 = self.length_scales(n2)
        return self.shape(r, np.sqrt(r1 * r2))

    def cutoff(self, elements):
        max_length_scale = self.length_scales(elements).max()
        return self.shape.cutoff(max_length_scale)
