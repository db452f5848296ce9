#!/usr/bin/env python
"""The LDS figures of the solver menu, recorded ONCE from the commit before
the menu became `kernel/marginalized/_menu.py` and each LDS layout was stated
once; tests/test_menu_module.py replays them on the
current code.  Host only: no device, no compiler.

lds_bytes.json holds

* `lds_bytes`: `HIPBackend.lds_bytes(v, C, ntask, gbytes, tab_bytes, nodal)`
  of every variant of the default menu, in float and double, for C in (1, 2)
  and nodal in (False, True), the two-stage variants also with 4096 bytes of
  tables, at the `POINTS` (vector size, image bytes): the values around the
  multiples of 4, 16 and 64 that the caps of the regions round to.  `grids`
  holds the distinct rows of figures, `lds_bytes` the index of every case's
  row in it;
* `launches`: variant, `dynamic_lds`, `ucap`, `gcap` and `dense` of every
  launch of `_partition`, with the shape of the call, for the small calls of
  tests/golden/host_plans.json (`small_calls`).

    python tests/golden/make_golden_lds_bytes.py     # rewrites the fixture
"""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
VECTORS = (0, 1, 63, 64, 65, 380, 4095)
IMAGES = (0, 1, 15, 16, 17, 800, 20000)
#: the product of the two, thinned to keep the fixture small: every vector
#: size at one image size, every image size at one vector size (the figure is
#: a sum of a term in either), and two corners that a term in both would move
POINTS = tuple([(nt, 17) for nt in VECTORS]
               + [(65, gb) for gb in IMAGES if gb != 17]
               + [(0, 0), (4095, 20000)])
TABLES = (0, 4096)
REALS = (np.float32, np.float64)
job_t = np.dtype([('i', np.uint32), ('j', np.uint32)])


def menu(backend):
    """The solver variants of a backend's menu (not the sentinels)."""
    return [v for v in backend.variants if v.W > 0]


def is_oc(v):
    return hasattr(v, 'D')


def grid_key(real, v, C, nodal, tab_bytes):
    return '/'.join(['f%d' % (8 * np.dtype(real).itemsize), 'x'.join(
        'L' + '.'.join(map(str, f)) if isinstance(f, tuple) else str(f)
        for f in v if f is not None), f'C{C}n{int(nodal)}t{tab_bytes}'])


def grid_cases(backend):
    """(key, v, C, nodal, tab_bytes) of every recorded grid of a backend."""
    for v in menu(backend):
        for C in (1, 2):
            for nodal in (False, True):
                for tab in ((0,) if is_oc(v) else TABLES):
                    yield grid_key(backend.real, v, C, nodal, tab), v, C, \
                        nodal, tab


def small_calls():
    """(key, real, backend options, graphs, kernels, traits) of the calls of
    ``scripts/host_plan_digest.py --small``."""
    import cases
    from graphdot_amd.kernel.marginalized._backend_hip import VARIANTS
    c3, tang = cases.config3_kernels(), cases.tang2019_kernels()
    todo = [
        ('config3', cases.config3_graphs(24), c3,
         [dict(), dict(eval_gradient=True)]),
        ('config3_8', cases.config3_graphs(8), c3,
         [dict(nodal=True), dict(lmin=1), dict(diagonal=True)]),
        ('config1', cases.config1_graphs(), cases.config1_kernels(), [dict()]),
        ('config2', cases.config2_graphs(8, seed=0), cases.config2b_kernels(),
         [dict()]),
        ('large', cases.protein_like_graphs(4, nmin=150, nmax=420, seed=41),
         tang, [dict(), dict(nodal=True), dict(eval_gradient=True)]),
    ]
    for real in REALS:
        for name, graphs, kernels, calls in todo:
            for kw in calls:
                yield ('/'.join([name, np.dtype(real).name,
                                 ','.join(sorted(kw)) or 'value']),
                       real, {}, graphs, kernels, kw)
        yield ('two_stage_only/' + np.dtype(real).name, real,
               dict(variants=list(VARIANTS)), cases.config3_graphs(6), c3, {})


def host_plan_of(backend, graphs, kernels, traits_kw):
    """(jobs, first `HostPlan`) of a call, as host_plan_digest.py makes it."""
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    kn, ke, q = kernels
    k = MarginalizedGraphKernel(kn, ke, q=q, backend=backend)
    n = len(graphs)
    if traits_kw.get('diagonal'):
        i = j = np.arange(n)
    else:
        i, j = np.triu_indices(n)
    jobs = np.column_stack((i, j)).astype(np.uint32).ravel().view(job_t)
    traits = k.traits(symmetric=not traits_kw.get('diagonal'), **traits_kw)
    return jobs, next(backend._host_plans(graphs, kn, ke, jobs, traits))


def launch_record(L):
    v = L['variant']
    return dict(variant=[list(f) if isinstance(f, tuple) else f for f in v],
                dynamic_lds=int(L['dynamic_lds']), ucap=int(L['ucap']),
                gcap=int(L['gcap']), dense=bool(L.get('dense', False)))


def record():
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    grids, index = [], {}
    for real in REALS:
        b = HIPBackend(real=real)
        for key, v, C, nodal, tab in grid_cases(b):
            grid = [int(b.lds_bytes(v, C, nt, gb, tab, nodal))
                    for nt, gb in POINTS]
            if grid not in grids:      # (many cases share their figures)
                grids.append(grid)
            index[key] = grids.index(grid)
    launches = {}
    for key, real, options, graphs, kernels, kw in small_calls():
        b = HIPBackend(real=real, **options)
        _, plan = host_plan_of(b, graphs, kernels, kw)
        s = plan.shape
        launches[key] = dict(
            C=s.C, nodal=bool(s.nodal), tab_bytes=int(s.tab_bytes),
            launches=[launch_record(L) for L in plan.part[3]])
    return dict(points=[list(p) for p in POINTS],
                grids=grids, lds_bytes=index, launches=launches)


if __name__ == '__main__':
    for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
        if p not in sys.path:
            sys.path.insert(0, p)
    with open(os.path.join(HERE, 'lds_bytes.json'), 'w') as f:
        json.dump(record(), f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
