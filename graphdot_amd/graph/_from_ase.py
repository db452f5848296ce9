"""Molecular graphs from atoms in 3D (reference: ``graphdot/graph/_from_ase.py``).

The atoms object is duck-typed: only ``len()``, ``get_atomic_numbers()``,
``get_positions()``, ``pbc``, ``cell``, ``get_initial_charges()`` (with
`use_charge`) and, if present, ``get_chemical_formula()`` are read, so an ASE
``Atoms`` works and so does any object holding numbers and positions.

The neighbour search is vectorised: dense distances per periodic image for
small structures, ``scipy.spatial.cKDTree`` for large ones.  The selection is
the reference's: for every atom pair i < j the nearest image of j (among
{-1, 0, 1}^3 along the periodic axes) whose weight is positive becomes the
edge; the edges are listed in (i, j) order.
"""
from collections import Counter
from itertools import product
import uuid
import numpy as np
from ..minipandas import DataFrame
from .adjacency.atomic import AtomicAdjacency, SYMBOLS

#: atoms x images above which the neighbour search uses a k-d tree
_DENSE_LIMIT = 1 << 22


def hill_formula(numbers):
    """Chemical formula in Hill order (C, H, then alphabetical; all
    alphabetical without carbon), counts of one omitted."""
    count = Counter(SYMBOLS[int(z)] for z in numbers)
    if 'C' in count:
        head = ['C'] + (['H'] if 'H' in count else [])
    else:
        head = []
    order = head + sorted(s for s in count if s not in head)
    return ''.join(s + (str(count[s]) if count[s] > 1 else '') for s in order)


def _candidates(x, x_images, n, cutoff):
    """(i, image row, r) of every pair within `cutoff`."""
    if n * len(x_images) <= _DENSE_LIMIT:
        d = x[:, None, :] - x_images[None, :, :]
        r = np.sqrt((d * d).sum(axis=-1))
        i, k = np.nonzero(r <= cutoff)
        return i, k, r[i, k]
    from scipy.spatial import cKDTree
    nl = cKDTree(x).sparse_distance_matrix(cKDTree(x_images), cutoff,
                                           output_type='ndarray')
    return (nl['i'].astype(np.int64), nl['j'].astype(np.int64),
            nl['v'].astype(np.float64))


def _from_ase(cls, atoms, adjacency='default', use_charge=False, use_pbc=True):
    """Convert atoms in 3D space to a molecular graph: atoms become nodes
    (``element``, and ``charge`` with `use_charge`), short-range pairs edges
    (weight ``!w`` from `adjacency`, ``length``).  `use_pbc`: a boolean or
    three, and-ed with ``atoms.pbc``."""
    if isinstance(adjacency, str) and adjacency == 'default':
        adjacency = AtomicAdjacency()

    n = len(atoms)
    numbers = np.asarray(atoms.get_atomic_numbers())
    nodes = DataFrame({'!i': range(n)})
    nodes['element'] = numbers.astype(np.int8)
    if use_charge:
        nodes['charge'] = np.asarray(
            atoms.get_initial_charges()).astype(np.float32)

    pbc = np.logical_and(atoms.pbc, use_pbc)
    cell = np.asarray(atoms.cell)
    images = [(cell.T * image).sum(axis=1) for image in product(
        *tuple([-1, 0, 1] if p else [0] for p in np.broadcast_to(pbc, 3)))]
    x = np.asarray(atoms.get_positions(), dtype=np.float64)
    x_images = np.vstack([x + i for i in images])

    cutoff = adjacency.cutoff(numbers)
    i, k, r = _candidates(x, x_images, n, cutoff)
    j = k % n
    # (a pair at distance 0 is not a neighbour: the reference's sparse
    # distance matrix holds no zeros)
    keep = (j > i) & (r > 0)
    i, j, r = i[keep], j[keep], r[keep]
    w = np.asarray(adjacency(numbers[i], numbers[j], r), dtype=np.float64)
    keep = w > 0
    i, j, r, w = i[keep], j[keep], r[keep], w[keep]
    # the nearest image of each (i, j)
    order = np.lexsort((r, j, i))
    i, j, r, w = i[order], j[order], r[order], w[order]
    first = np.ones(len(i), dtype=bool)
    first[1:] = (i[1:] != i[:-1]) | (j[1:] != j[:-1])
    i, j, r, w = i[first], j[first], r[first], w[first]
    if len(i) == 0:
        raise ValueError('The atoms make no edges under this adjacency rule: '
                         'a molecular graph needs at least one.')

    edges = DataFrame({
        '!i': np.array(i, dtype=np.uint32),
        '!j': np.array(j, dtype=np.uint32),
        '!w': np.array(w, dtype=np.float32),
        'length': np.array(r, dtype=np.float32),
    })

    formula = atoms.get_chemical_formula() \
        if hasattr(atoms, 'get_chemical_formula') else hill_formula(numbers)
    return cls(nodes, edges, title='Molecule {formula} {id}'.format(
        formula=formula, id=uuid.uuid4().hex))
