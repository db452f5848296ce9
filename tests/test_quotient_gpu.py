"""Plain value calls on the twin-leaf quotient images (mgk_oc.h QUOT, DESIGN.md
section 4a) against the same backend on the full images: Gram matrices,
cross matrices and diagonals in both arithmetics and at two tolerances, the
iteration counts, and the calls that must not take the quotient path."""
import numpy as np
import pytest

import cases
from graphdot_amd.graph import Graph
from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
from oracle import mgk as oracle
from test_quotient import hand_built

pytestmark = pytest.mark.gpu

N_X = 13          # the cross calls: the first N_X graphs against the rest
#: Tolerance at which the iteration counts of the DEFAULT builds are compared.
#: The float build, and the double build with its float-rounded step lengths
#: (mgk_oc.h FSCAL), leave a residual of about eps * max(Dx) * sqrt(N) =
#: 6e-8 * 16 / (1 - q)^2 * sqrt(N) ~ 1e-6 sqrt(N) that no further iteration
#: of theirs removes in one step; the rule sqrt(rTr) < ftol N sits a factor
#: ten above it for every N >= 4 (two nodes by two) from ftol = 1e-5 on.
#: Below, both solvers stop where rounding lets them -- no property of the
#: system, least of all for the smallest pairs, whose CG terminates after
#: four steps in exact arithmetic.  Measured at 1e-8: float 17 of 780 pairs
#: apart, double 12 of 780, each with pairs 2 steps apart (methane x ethane);
#: mean iterations 14.135 / 14.147 (float), 14.141 / 14.147 (double).
#: At the issue's own tolerances, 1e-8 and 1e-13, the counts are compared on
#: the double build with DOUBLE scalars (-DGD_OC_FSCAL=0), whose iterates are
#: those of the formulation to double rounding.
ROUNDING_SAFE_FTOL = 1e-5
DOUBLE_SCALARS = 'double scalars'


@pytest.fixture(scope='module')
def graphs():
    hand = [Graph.from_networkx(g) for g, _, _ in hand_built().values()]
    return Graph.unify_datatype(hand + cases.config3_graphs(30))


@pytest.fixture(scope='module')
def results(graphs):
    """(real, ftol, quotient) -> dict of K, Kxy, diag and the iteration
    counts of the symmetric call; every backend is made once."""
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    knode, kedge, q = cases.config3_kernels()
    out = {}
    for real in (np.float32, np.float64, DOUBLE_SCALARS):
        for quotient in (True, False):
            be = HIPBackend(
                real=np.float64 if real is DOUBLE_SCALARS else real,
                quotient=quotient, record_iterations=True,
                **({'hipcc_extra': ['-DGD_OC_FSCAL=0']}
                   if real is DOUBLE_SCALARS else {}))
            for ftol in (1e-8, 1e-13) + (
                    () if real is DOUBLE_SCALARS else (ROUNDING_SAFE_FTOL,)):
                k = MarginalizedGraphKernel(knode, kedge, q=q, backend=be,
                                            ftol=ftol)
                r = {'K': k(graphs)}
                r['quotient'] = be.last_plan.quotient
                r['it'] = be.iterations(be.last_plan).astype(np.int64)
                out[(real, ftol, quotient)] = r
                if real is DOUBLE_SCALARS:
                    continue
                r['Kxy'] = k(graphs[:N_X], graphs[N_X:])
                r['quotient'] &= be.last_plan.quotient
                r['diag'] = k.diag(graphs)
                r['quotient'] &= be.last_plan.quotient
                r['kernels'] = {L['variant'].R for L in be.last_plan.launches}
                out[(real, ftol, quotient)] = r
    return out


def _rel(a, b):
    return float(np.max(np.abs(a / b - 1)))


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('ftol', [1e-8, 1e-13])
def test_quotient_values_are_those_of_the_full_images(results, graphs, real,
                                                      ftol):
    on, off = results[(real, ftol, True)], results[(real, ftol, False)]
    assert on['quotient'] and not off['quotient']
    figures = {name: _rel(on[name], off[name])
               for name in ('K', 'Kxy', 'diag')}
    print(real.__name__, ftol, figures)
    assert np.array_equal(on['K'], on['K'].T)
    if ftol == 1e-13:
        bound = 1e-5 if real is np.float32 else 1e-11
        assert max(figures.values()) <= bound, figures
    else:
        # both inside the parity tolerance of the C restatement of the
        # reference's PCG at this tolerance (tests/test_parity_gpu.py)
        knode, kedge, q = cases.config3_kernels()
        i, j = np.triu_indices(len(graphs))
        batch = oracle.TensorProductBatch(graphs, knode, kedge)
        ref, _ = batch.run(i, j, q=q, tol=ftol,
                           real='f32' if real is np.float32 else 'f64')
        rtol = 1e-5 if real is np.float32 else 2e-7
        for r in (on, off):
            assert np.allclose(r['K'][i, j], ref, rtol=rtol), \
                _rel(r['K'][i, j], ref)
            assert np.allclose(r['Kxy'], r['K'][:N_X, N_X:], rtol=rtol)
            assert np.allclose(r['diag'], np.diag(r['K']), rtol=rtol)


@pytest.mark.parametrize('real,ftol', [(np.float32, ROUNDING_SAFE_FTOL),
                                       (np.float64, ROUNDING_SAFE_FTOL),
                                       (DOUBLE_SCALARS, 1e-8),
                                       (DOUBLE_SCALARS, 1e-13)])
def test_quotient_iteration_counts_are_those_of_the_full_images(results, real,
                                                                ftol):
    """The rescaled quotient system has the inner products of the full one:
    the same alpha, beta and rTr, so the same iteration in which the residual
    passes sqrt(rTr) < ftol N (N of the FULL pair) -- except where rounding
    moves a residual across the threshold: at most 2 % of the pairs, by one
    step.  The default builds are compared at ROUNDING_SAFE_FTOL, the double
    build with double scalars at 1e-8 and 1e-13 (see ROUNDING_SAFE_FTOL)."""
    on, off = results[(real, ftol, True)], results[(real, ftol, False)]
    d = np.abs(on['it'] - off['it'])
    print(getattr(real, '__name__', real), ftol, 'pairs', len(d), 'differ', int((d > 0).sum()),
          'max', int(d.max()), 'mean iterations', on['it'].mean(),
          off['it'].mean())
    assert d.max() <= 1
    assert (d > 0).sum() <= 0.02 * len(d)


def test_quotient_pairs_have_fewer_row_batches(results):
    on, off = results[(np.float64, 1e-8, True)], \
        results[(np.float64, 1e-8, False)]
    assert max(on['kernels']) < max(off['kernels'])


@pytest.mark.parametrize('real', [np.float32, np.float64])
def test_gradient_and_nodal_calls_keep_the_full_images(graphs, real):
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    knode, kedge, q = cases.config3_kernels()
    sub = graphs[:16]
    got = []
    for quotient in (True, False):
        be = HIPBackend(real=real, quotient=quotient)
        k = MarginalizedGraphKernel(knode, kedge, q=q, backend=be)
        K, dK = k(sub, eval_gradient=True)
        assert not be.last_plan.quotient
        Kn = k(sub, nodal=True)
        assert not be.last_plan.quotient
        K1 = k(sub, lmin=1)
        assert not be.last_plan.quotient
        got.append((K, dK, Kn, K1))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
