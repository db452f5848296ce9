"""The Marginalized MiniMax (M3) metric between molecules (reference:
``graphdot/experimental/metric/m3.py``).

Both structures become graphs by `Graph.from_ase`; with the nodal
marginalized-kernel similarities ``k12(i1, i2)`` of the pair and the nodal
self-similarities ``k1``, ``k2`` of the two graphs,

    K = k12 / sqrt(k1 k2),   D = sqrt(max(2 - 2 K, 0)),
    M3 = max( max_i1 min_i2 D,  max_i2 min_i1 D ).

Arithmetic is double throughout.  On the HIP backend the pairs the
owner-computes solvers cover take one fused launch
(`HIPBackend.m3_distance`): the Hausdorff reduction runs in LDS in the
solver's epilogue and the nodal matrix never leaves the compute unit.
Elsewhere -- other backends, pairs sharded over ranks, graphs beyond the
owner-computes menu -- the nodal matrices are computed and reduced on the host
(`m3_from_nodal`).

A pair of one graph with itself takes ``k1 = k2`` from the diagonal of its own
nodal solution, on both paths: the reference computes ``k1`` by that very solve
(``_mlgk(g1, g1)``), and it makes ``M3(a, a)`` zero up to round-off rather than
up to the solver's tolerance.
"""
import numpy as np
from ...graph import Graph
from ...graph.adjacency.atomic import AtomicAdjacency
from ...microkernel import TensorProduct, KroneckerDelta, SquareExponential


def _segments(sizes):
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.concatenate(([0], np.cumsum(sizes)))


def m3_from_nodal(K, k1, k2, sx, sy, symmetric):
    """M3 distances of every graph pair from nodal similarities.

    K: (sx[-1], sy[-1]) nodal similarities of the X x Y graph pairs; k1, k2:
    nodal self-similarities of the graphs of X and Y; sx, sy: node offsets of
    the graphs (length len + 1).  `symmetric`: Y is X, so that the diagonal
    pairs are graphs with themselves and take their self-similarities from
    their own blocks of K.  Returns a (len X, len Y) float64 matrix."""
    K = np.asarray(K, dtype=np.float64)
    k1 = np.array(k1, dtype=np.float64)
    k2 = np.array(k2, dtype=np.float64)
    if symmetric:
        k1 = k2 = np.diagonal(K).copy()
    R1 = k1**-0.5
    R2 = k2**-0.5
    Kn = R1[:, None] * K * R2[None, :]
    D = np.sqrt(np.maximum(2 - 2 * Kn, 0))
    sx, sy = np.asarray(sx), np.asarray(sy)
    d12 = np.maximum.reduceat(
        np.minimum.reduceat(D, sy[:-1], axis=1), sx[:-1], axis=0)
    d21 = np.maximum.reduceat(
        np.minimum.reduceat(D, sx[:-1], axis=0), sy[:-1], axis=1)
    return np.maximum(d12, d21)


class M3:
    """The Marginalized MiniMax (M3) metric between molecules.

    Parameters
    ----------
    use_charge: bool
        Compare the atoms' initial charges as well as their elements.
    adjacency: 'default' or adjacency rule
        How `Graph.from_ase` makes edges; 'default' is
        ``AtomicAdjacency(shape='tent2', zoom=0.75)``.
    q: float
        Stopping probability of the random walk.
    element_delta, bond_eps, charge_eps: float
        Hyperparameters of the element, bond-length and charge microkernels.
    backend: 'auto' | 'hip' | Backend
        'auto' and 'hip' build a double-precision HIP backend.
    """

    def __init__(self, use_charge=False, adjacency='default', q=0.01,
                 element_delta=0.2, bond_eps=0.02, charge_eps=0.2,
                 backend='auto'):
        self.use_charge = use_charge
        if isinstance(adjacency, str) and adjacency == 'default':
            self.adjacency = AtomicAdjacency(shape='tent2', zoom=0.75)
        else:
            self.adjacency = adjacency
        self.q = q
        if use_charge:
            self.node_kernel = TensorProduct(
                element=KroneckerDelta(element_delta),
                charge=SquareExponential(charge_eps),
            )
        else:
            self.node_kernel = TensorProduct(
                element=KroneckerDelta(element_delta)
            )
        self.edge_kernel = TensorProduct(length=SquareExponential(bond_eps))
        self._backend = backend
        self._kernel = None

    @property
    def kernel(self):
        """The nodal marginalized graph kernel, double precision (built on
        first use: the HIP runtime is loaded only then)."""
        if self._kernel is None:
            from ...kernel.marginalized import MarginalizedGraphKernel
            backend = self._backend
            if isinstance(backend, str) and backend in ('auto', 'hip', 'cuda'):
                from ...kernel.marginalized._backend_hip import HIPBackend
                backend = HIPBackend(real=np.float64)
            self._kernel = MarginalizedGraphKernel(
                self.node_kernel, self.edge_kernel, q=self.q,
                dtype=np.float64, backend=backend)
        return self._kernel

    def graph(self, atoms):
        """The graph of `atoms` (a `Graph` is taken as it is)."""
        if isinstance(atoms, Graph):
            return atoms
        return Graph.from_ase(atoms, use_charge=self.use_charge,
                              adjacency=self.adjacency)

    def _graphs(self, X, Y):
        """Unified graphs of X and Y (each object converted once), and
        whether the call is symmetric (Y is None or holds X's objects)."""
        built = {}

        def convert(items):
            out = []
            for a in items:
                if id(a) not in built:
                    built[id(a)] = (a, self.graph(a))
                out.append(built[id(a)][1])
            return out

        X = list(X)
        symmetric = Y is None or (
            len(Y) == len(X) and all(a is b for a, b in zip(X, Y)))
        GX = convert(X)
        GY = [] if symmetric else convert(list(Y))
        G = Graph.unify_datatype(GX + GY)
        return G[:len(GX)], (None if symmetric else G[len(GX):]), symmetric

    def __call__(self, atoms1, atoms2):
        """M3 distance of two structures (atoms-like objects or graphs)."""
        if atoms1 is atoms2:
            return float(self.pairwise([atoms1])[0, 0])
        return float(self.pairwise([atoms1], [atoms2])[0, 0])

    def pairwise(self, X, Y=None):
        """(len X, len Y or len X) matrix of M3 distances in one evaluation.
        Items are atoms-like objects or `Graph`s made by `Graph.from_ase`."""
        GX, GY, symmetric = self._graphs(X, Y)
        D = self._fused(GX, GY)
        if D is None:
            D = self._composition(GX, GY)
        return D

    # -- the two evaluations ---------------------------------------------------------
    def _nodal(self, GX, GY):
        """Nodal similarities of the X x Y pairs and nodal self-similarities
        of both sides, float64."""
        mgk = self.kernel
        K = mgk(GX, GY, nodal=True)
        k1 = mgk.diag(GX, nodal=True)
        k2 = k1 if GY is None else mgk.diag(GY, nodal=True)
        return K, k1, k2

    def _composition(self, GX, GY):
        K, k1, k2 = self._nodal(GX, GY)
        sx = _segments([len(g.nodes) for g in GX])
        sy = sx if GY is None else _segments([len(g.nodes) for g in GY])
        return m3_from_nodal(K, k1, k2, sx, sy, GY is None)

    def _fused(self, GX, GY):
        """The fused device evaluation, or None where it does not apply."""
        mgk = self.kernel
        backend = mgk.backend
        if not hasattr(backend, 'm3_distance') or \
                getattr(backend, 'shards_over_ranks', lambda: False)():
            return None
        if np.dtype(backend.real) != np.float64:
            return None
        from ...kernel.marginalized._backend_hip import NotOwnerComputes
        graphs = list(GX) if GY is None else list(GX) + list(GY)
        nx = len(GX)
        ny = nx if GY is None else len(GY)
        if nx == 0 or ny == 0:
            return None
        if GY is None:
            i, j = np.triu_indices(nx)
        else:
            i, j = np.indices((nx, ny))
            j = j + nx
        job_t = np.dtype([('i', np.uint32), ('j', np.uint32)])
        jobs = np.column_stack((i.ravel(), j.ravel())).astype(
            np.uint32).ravel().view(job_t)
        traits = mgk.traits(symmetric=GY is None, nodal=False)
        try:
            d = backend.m3_distance(
                graphs, mgk.node_kernel, mgk.edge_kernel, mgk.p, mgk.q,
                mgk.eps, mgk.ftol, mgk.gtol, jobs, nx, ny, mgk.n_dims,
                traits)
        except NotOwnerComputes:
            return None
        return np.asarray(d, dtype=np.float64).reshape(nx, ny, order='F')
