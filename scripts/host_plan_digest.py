"""Digest of the host plans of a fixed list of calls ("The host
plan of a call"): which images a call takes, its solver variants, launch
order and launch geometry, the JIT cache keys of its rendered sources, and
the shard plans of two and eight ranks.  Host only: no device, no compiler.

    python scripts/host_plan_digest.py [--small] [TREE] OUT.json

TREE (default: this tree) is where graphdot_amd and tests/cases.py are
imported from, in a child process with PYTHONPATH=TREE -- like
``isa_fingerprint.py --dense [TREE]``.  Two trees plan alike iff their digests
are equal: profiles/host_plans_parent.json (TREE = a checkout of the commit
before the host plan became one record) and profiles/host_plans.json are.
``--small``: the calls of tests/test_host_plans.py (tests/golden/host_plans.json).
"""
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def crc(a):
    import numpy as np
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def host_plan(b, graphs, kn, ke, p, jobs, traits):
    """(quotient taken?, used, launch order, launches, sources) of a call:
    the only tree-dependent part."""
    if hasattr(b, '_frontend'):       # before the record: precompile's tuple
        dgs, _, _, _, used, order, launches, sources = b._frontend(
            graphs, kn, ke, p, jobs, traits)
        quot = getattr(dgs[0], 'n_orig', None) is not None
        return quot, used, order, launches, sources
    plan = next(b._host_plans(graphs, kn, ke, jobs, traits))
    _, used, order, launches = plan.part
    return plan.shape.quot, used, order, launches, b._sources(
        used, kn, plan.edge_kernel, p, plan.dgraphs, plan.shape)


LAUNCH_KEYS = ('offset', 'count', 'ucap', 'gcap', 'dynamic_lds', 'grid',
               'threads', 'tab', 'dense')


def call_digest(b, graphs, kernels, traits_kw, shards=False):
    import numpy as np
    from graphdot_amd.hip import jit
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._sharded import measured_shard_plan
    kn, ke, q = kernels
    k = MarginalizedGraphKernel(kn, ke, q=q, backend=b)
    n = len(graphs)
    if traits_kw.get('diagonal'):
        i = j = np.arange(n)
    else:
        i, j = np.triu_indices(n)
    jobs = np.column_stack((i, j)).astype(np.uint32).ravel().view(
        np.dtype([('i', np.uint32), ('j', np.uint32)]))
    traits = k.traits(symmetric=not traits_kw.get('diagonal'), **traits_kw)
    quot, used, order, launches, sources = host_plan(
        b, graphs, kn, ke, k.p, jobs, traits)
    out = dict(
        quotient=bool(quot),
        variants=[str(b.variants[v]) for v in used],
        order_crc=crc(np.asarray(order, dtype=np.int64)),
        launches=[dict({key: L.get(key) for key in LAUNCH_KEYS},
                       variant=str(L['variant']),
                       costs_crc=crc(np.asarray(L['costs']))
                       if 'costs' in L else None) for L in launches],
        sources=sorted(jit.cache_key(s, b.hipcc_extra)
                       for s in sources.values()))
    if shards:
        out['shards'] = {}
        for world in (2, 8):
            sp = measured_shard_plan(b, graphs, kn, ke, jobs, n, n, traits,
                                     0, world)
            m = sp._model
            out['shards'][str(world)] = dict(
                merge_map=sorted([int(a), int(c)]
                                 for a, c in sp.merge_map.items()),
                quotient=None if sp.quotient is None else sorted(
                    [int(a), int(c)] for a, c in sp.quotient.items()),
                launch_order_crc=crc(m['launch_order']),
                group_crc=crc(np.asarray(m['group'], dtype=np.int64)),
                sizes=[len(s) for s in sp.shards])
    return out


def digest(small=False):
    import numpy as np
    import cases
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend, \
        VARIANTS
    c3, tang = cases.config3_kernels(), cases.tang2019_kernels()
    todo = [
        ('config3', cases.config3_graphs(24 if small else 1000), c3,
         [dict(), dict(eval_gradient=True)], True),
        ('config3_8', cases.config3_graphs(8), c3,
         [dict(nodal=True), dict(lmin=1), dict(diagonal=True)], False),
        ('config1', cases.config1_graphs(), cases.config1_kernels(),
         [dict()], True),
        ('config2', cases.config2_graphs(8 if small else 256, seed=0),
         cases.config2b_kernels(), [dict()], True),
    ]
    if not small:
        todo.append(('tang2019', cases.tang2019_graphs(256), tang,
                     [dict(), dict(eval_gradient=True)], True))
    todo.append(('large', cases.protein_like_graphs(4, nmin=150, nmax=420,
                                                    seed=41), tang,
                 [dict(), dict(nodal=True), dict(eval_gradient=True)], False))
    out = {}
    for real in (np.float32, np.float64):
        b = HIPBackend(real=real)
        for name, graphs, kernels, calls, shards in todo:
            for kw in calls:
                key = '/'.join([name, np.dtype(real).name,
                                ','.join(sorted(kw)) or 'value'])
                out[key] = call_digest(b, graphs, kernels, kw,
                                       shards and not kw)
        # a menu of two-stage variants only: quotient images exist, their
        # layout is refused (not owner-computes) -- the fallback arm
        b2 = HIPBackend(real=real, variants=list(VARIANTS))
        out['two_stage_only/' + np.dtype(real).name] = call_digest(
            b2, cases.config3_graphs(6), c3, {}, True)
    return out


def main(argv):
    if argv[:1] == ['--child']:
        small = '--small' in argv
        with open(argv[-1], 'w') as f:
            json.dump(digest(small), f, indent=1, sort_keys=True)
            f.write('\n')
        return
    small = ['--small'] if '--small' in argv else []
    argv = [a for a in argv if a != '--small']
    tree = os.path.abspath(argv[0]) if len(argv) > 1 else ROOT
    subprocess.run(
        [sys.executable, os.path.abspath(__file__), '--child', *small,
         os.path.abspath(argv[-1])], check=True,
        env=dict(os.environ, PYTHONPATH=os.pathsep.join(
            (tree, os.path.join(tree, 'tests')))))


if __name__ == '__main__':
    main(sys.argv[1:])
