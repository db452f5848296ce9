"""Every solver of the menu alone, on pairs at the edge of what it fits
(tests/menu_edges.py), against the oracle: one test per (variant, real)
under ``HIPBackend(variants=[v, GENERAL], quotient=False, min_launch=0)``.

The reference is `oracle.gram`, pair by pair: the dense solve
(``np.linalg.solve``) for every pair of at most `DENSE_ROWS` rows -- every
edge pair of the owner-computes slot solvers, whose largest capacity is
64 x 16 x 3 = 3072 rows -- and the oracle's double-precision conjugate
gradients to 1e-13 beyond (the pairs of the general solver that a set has
between its two largest graphs, and the edge pairs of the three largest
two-stage and on-the-fly entries): a dense solve of 16 384 rows takes a
minute and 2 GB.  That holds for values and nodal values.  The GRADIENT
reference of a pair above `DENSE_ROWS` rows is weaker: `oracle.solve_pair`
hands the two right-hand sides to `mgk_pcg_duo_f64`, which takes no tolerance
and stops at |r| < 1e-10 x 2 N -- the reference's fixed rule, the one the
device's value + gradient solve stops at too -- so for those pairs (the
4096-row full pair of OCVariant(16, 0, 4, 0), the full pairs of the
two-stage entries from 4095 rows on, the general solver's pairs) the gradient
check compares two double solves with one stopping rule, held to (2e-3, 2e-5)
or (1e-6, 1e-9); every gradient edge pair of up to 3072 rows, among them all
of the owner-computes slot solvers, has the dense reference.  An edge whose
pair needs a graph of several hundred nodes (3 x 683, 7 x 439) is taken as a
call k([a], [b]) of its own, not as part of the symmetric set: the set's
reference would have to solve that graph against itself.  The microkernels
of the reference are evaluated in float64 (`oracle.wide_rows`, as test_double_build_on_systems_of_a_few_rows does: in
the float32 of the attribute columns they are 6e-8 off, which a double build
held to 1e-9 shows).  References are made once per graph set and shared by
the arithmetics; most of a test's time is the oracle's Python loop over the
pairs of adjacency nonzeros, which is why `menu_edges.search` picks the sets
that are cheapest for it.

Bounds: those of test_rational_quadratic_dotproduct_and_power_microkernels
(value 1e-5 / 1e-9, gradient (2e-3, 2e-5) / (1e-6, 1e-9)) with ftol 1e-8 /
1e-13; the double value + gradient solve stops at the reference's fixed
rule, so its value is held to the 1e-8 of
test_double_build_on_systems_of_a_few_rows."""
import numpy as np
import pytest

import menu_edges as me
from graphdot_amd.kernel.marginalized._backend_hip import GENERAL
from oracle import mgk as oracle
from test_parity_gpu import elementwise_gradient_error

pytestmark = pytest.mark.gpu

DENSE_ROWS = 3072
FIXTURES = list(me.fixtures())
RNAME = {real: name for name, real in me.REALS.items()}
CASES = list({(v, RNAME[real]): None for v, real, _, _, _ in FIXTURES})
_REFERENCES = {}


def reference(recipes, graphs, k, what, cross=False):
    """`oracle.gram` of the set, pair by pair (see the module docstring);
    `what`: 'value', 'nodal' or 'gradient'.  `cross`: of the one pair
    (graphs[0], graphs[1]) alone, as a 1 x 1 matrix."""
    key = (tuple(map(tuple, recipes)), what, cross)
    if key in _REFERENCES:
        return _REFERENCES[key]
    if cross:
        a, c = graphs
        with oracle.wide_rows():
            r = oracle.gram([a], k.node_kernel, k.edge_kernel, Y=[c], q=k.q,
                            tol=1e-13, eval_gradient=what == 'gradient',
                            mode='dense' if len(a.nodes) * len(c.nodes)
                            <= DENSE_ROWS else 'pcg64')
        r = r[1] if what == 'gradient' else r
        r.flags.writeable = False
        _REFERENCES[key] = r
        return r
    n = len(graphs)
    sizes = [len(g.nodes) for g in graphs]
    s = np.concatenate(([0], np.cumsum(sizes))) if what == 'nodal' \
        else np.arange(n + 1)
    out = None
    for a in range(n):
        for c in range(a, n):
            mode = 'dense' if sizes[a] * sizes[c] <= DENSE_ROWS else 'pcg64'
            # (microkernels in float64 on the float32 attribute columns, as
            # test_double_build_on_systems_of_a_few_rows: evaluated in the
            # columns' own type they are 6e-8 off, oracle.WIDE_ROWS)
            with oracle.wide_rows():
                r = oracle.gram([graphs[a]], k.node_kernel, k.edge_kernel,
                                Y=[graphs[c]], q=k.q, tol=1e-13, mode=mode,
                                nodal=what == 'nodal',
                                eval_gradient=what == 'gradient')
            r = r[1] if what == 'gradient' else r
            if out is None:
                out = np.zeros((s[-1], s[-1]) + r.shape[2:])
            out[s[a]:s[a + 1], s[c]:s[c + 1]] = r
            out[s[c]:s[c + 1], s[a]:s[a + 1]] = np.swapaxes(r, 0, 1)
    out.flags.writeable = False
    _REFERENCES[key] = out
    return out


def variant_of_jobs(plan):
    """The variant that ran every job of the plan, in job order."""
    out = [None] * plan.n_jobs
    for L in plan.launches:
        for t in plan.order_host[L['offset']:L['offset'] + L['count']]:
            out[int(t)] = L['variant']
    return out


@pytest.mark.parametrize('v,rname', CASES,
                         ids=[f'{me.variant_id(v)}-{r}' for v, r in CASES])
def test_variant_alone_at_its_edges(v, rname):
    vid = me.variant_id(v)
    real = me.REALS[rname]
    f32 = real is np.float32
    vtol = 1e-5 if f32 else 1e-9
    gtol = (2e-3, 2e-5) if f32 else (1e-6, 1e-9)
    b = me.one_variant_backend(v, real, record_iterations=True)
    k = me.kernel_on(b, real)
    assert k.ftol == (1e-8 if f32 else 1e-13)
    by_c = {C: (G_, edges_) for v_, real_, C, G_, edges_ in FIXTURES
            if v_ == v and real_ is real}
    assert by_c

    def close(got, want, rtol):
        err = np.abs(np.asarray(got, dtype=np.float64) / want - 1).max()
        print(f'{vid} {rname}: max relative error {err:.3e} (bound {rtol})')
        return err <= rtol

    def launched(edge_jobs, n_jobs):
        """Launches: the edge pairs ran in v, nothing but v and GENERAL."""
        plan = b.last_plan
        ran = variant_of_jobs(plan)
        assert len(ran) == n_jobs and None not in ran
        assert set(ran) <= {v, GENERAL}, set(ran)
        for t in edge_jobs:
            assert ran[t] == v, (t, ran[t])
        return plan

    def iterated(it, N, label, C=1):
        """Iterations: the pair iterated, and ended below the solver's cap:
        N steps, 2 N + 16 in the double owner-computes solvers, whose step
        lengths are rounded to float (mgk_oc.h FSCAL, max_its).  A system of
        a few rows may take all of them, so 'below' is asked where the cap is
        above what conjugate gradients can need at all: with q = 0.05 the
        Jacobi-scaled system has a condition number under (1 + (1 - q)^2) /
        (1 - (1 - q)^2) = 19.5, which bounds the steps to 1e-13 by
        sqrt(19.5) / 2 x ln(2e13) = 68 whatever N is.  A batch whose rows
        never enter the residual ends at once or runs into the cap.
        C = 2: the double static layouts solve the two systems one after the
        other and count both (mgk_oc.h SEQ: twice the cap, twice the 68)."""
        cap = 2 * N + 16 if me.kind_of(v) != 'two-stage' and not f32 else N
        solves = 2 if C == 2 and me.kind_of(v) == 'static' and not f32 else 1
        cap *= solves
        print(f'{vid} {rname}: {label}, C = {C}, N = {N}, {int(it)} '
              f'iterations, cap {cap}')
        assert 1 <= it <= cap
        assert it < cap or cap <= 68 * solves

    if 1 in by_c:
        G, edges = by_c[1]
        jobs = me.triu_jobs(len(G))
        at = {(int(i), int(j)): t for t, (i, j) in enumerate(jobs.tolist())}
        edge_jobs = sorted({at[p] for p in edges.values()})
        K = k(G)
        plan = launched(edge_jobs, len(jobs))
        it = b.iterations(plan)
        sizes = np.array([len(g.nodes) for g in G])
        for t in edge_jobs:
            iterated(it[t], int(sizes[jobs['i'][t]] * sizes[jobs['j'][t]]),
                     f'job {t}')
        # Value
        ref = reference(edges.recipes, G, k, 'value')
        assert close(K, ref, vtol)
        assert np.array_equal(K, K.T)
        # Repeat
        assert np.array_equal(k(G), K)
        # Nodal
        if v in me.nodal_representatives():
            Kn = k(G, nodal=True)
            ran = set(variant_of_jobs(b.last_plan))
            assert v in ran and ran <= {v, GENERAL}, ran
            assert close(Kn, reference(edges.recipes, G, k, 'nodal'), vtol)
        # Roles: the even x odd pair in both orders
        if 'stride' in edges:
            i, j = edges['stride']
            assert sizes[i] % 2 == 0 and sizes[j] % 2 == 1
            Kxy = k([G[i]], [G[j]])
            launched([0], 1)
            Kyx = k([G[j]], [G[i]])
            launched([0], 1)
            assert close(Kxy, ref[i:i + 1, j:j + 1], vtol)
            assert close(Kyx, ref[j:j + 1, i:i + 1], vtol)
            assert close(Kxy, np.asarray(Kyx.T, dtype=np.float64), vtol)

        # the edges taken as a call of their own
        for name, (ga, gc) in edges.cross.items():
            Kac = k([ga], [gc])
            plan = launched([0], 1)
            iterated(b.iterations(plan)[0], len(ga.nodes) * len(gc.nodes),
                     f'cross {name}')
            assert close(Kac, reference(edges.cross_recipes[name], (ga, gc),
                                        k, 'value', cross=True), vtol)

    if 2 in by_c:
        G, edges = by_c[2]
        jobs = me.triu_jobs(len(G))
        at = {(int(i), int(j)): t for t, (i, j) in enumerate(jobs.tolist())}
        K2, dK = k(G, eval_gradient=True)
        edge_jobs = sorted({at[p] for p in edges.values()})
        plan = launched(edge_jobs, len(jobs))
        it = b.iterations(plan)
        sizes = np.array([len(g.nodes) for g in G])
        for t in edge_jobs:
            iterated(it[t], int(sizes[jobs['i'][t]] * sizes[jobs['j'][t]]),
                     f'job {t}', C=2)
        ref = reference(edges.recipes, G, k, 'value')
        assert close(K2, ref, vtol if f32 else 1e-8)
        dref = reference(edges.recipes, G, k, 'gradient')
        err = elementwise_gradient_error(
            dK, dref[:, :, k.active_theta_mask], *gtol)
        print(f'{vid} {rname}: gradient violation ratio {err:.3e}')
        assert err <= 1
        for name, (ga, gc) in edges.cross.items():
            K2, dK = k([ga], [gc], eval_gradient=True)
            plan = launched([0], 1)
            iterated(b.iterations(plan)[0], len(ga.nodes) * len(gc.nodes),
                     f'cross {name}', C=2)
            pair = edges.cross_recipes[name]
            assert close(K2, reference(pair, (ga, gc), k, 'value', cross=True),
                         vtol if f32 else 1e-8)
            dref = reference(pair, (ga, gc), k, 'gradient', cross=True)
            err = elementwise_gradient_error(
                dK, dref[:, :, k.active_theta_mask], *gtol)
            print(f'{vid} {rname}: cross {name}, gradient violation ratio '
                  f'{err:.3e}')
            assert err <= 1
