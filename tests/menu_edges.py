"""Every solver of the menu alone, at the edge of what it fits: the graph
sets of tests/test_menu_edges.py (host rules, no device) and
tests/test_menu_edges_gpu.py (the kernels against the dense oracle).

A pair of graphs goes to the cheapest entry of the menu it fits
(``HIPBackend.classify``), so the workload-shaped sets of the parity tests
leave most entries far from the inequalities that admit a pair -- N = n1 n2
<= 64 W R, slot walk <= S, largest degree <= D, trips <= L[k] -- and a kernel
that mis-handles its last row batch at N == 64 W R would pass them.  Here
every entry ``v`` runs under ``HIPBackend(variants=[v, GENERAL],
quotient=False, min_launch=0)`` on a small set whose pairs sit ON those
inequalities.

The sets are synthetic and seeded: a graph is a recipe ``(generator, ...,
nodes[, seed])`` of `make_graph`, with the attributes of
`cases.config2_graphs`; the kernels are `cases.config2b_kernels`.  `FOUND`
is the result of `search()` -- ``python tests/menu_edges.py --search`` prints
it, and `UNREACHABLE`, `NOT_REACHED` and `SLOT_STEP`, which follow from it
-- committed as data, so that collection does not search;
tests/test_menu_edges.py recomputes every claimed equality from the public
host functions, so a set cannot drift off its edge when the menu changes.

Edges (`expected_edges`: name -> (i, j), a job of the symmetric call on the
set, i <= j):
  full        N == 64 W R; where no pair of the searched families reaches it
              (the row-stride rule NP = n1 (n2 | 1) <= 64 W R of the two-stage
              solvers, the LDS rule) the largest N given to v
  one_row     N == 64 W (R - 1) + 1: the last row batch holds one row
  no_last     N == 64 W (R - 1): the last row batch is absent
  slots_full  the slot walk uses all S slots
  max_degree  the largest degree of the pair == D
  trips_full  static: the trips equal L in every batch
  trips_first static: the trips equal L[0] in the first batch, no last batch
  grid        static: the two largest degrees == grid_of(L, D)
  stride      n_i even, n_j odd, and v takes the pair in both orders
  smallest    the smallest pair v takes
  dense       on-the-fly: a node of more than FLY_MIN_DEGREE neighbours and
              both adjacency matrices over 60 % full (the dense product)
`beyond`: name -> (recipe, recipe), the next pair up of a capacity edge (one
node more, one slot more), which v must NOT take.
`cross`: name -> (recipe, recipe), a row edge (`one_row`, `no_last`) taken as
a call k([a], [b]) of its own where no pair of graphs of at most 200 nodes
sits on it (2049 = 3 x 683): in the symmetric set the larger graph would
cost the reference its pair with itself.  Where the pool has no such pair
either, the sparsest pairs of every factorisation of the row count are tried
(`factor_pairs`); an edge is left to `NOT_REACHED` only when the variant takes
none of them.  A set is shared between the (real, C) of a variant only if it
sits on every edge; otherwise every build is searched by itself.
"""
import zlib

import numpy as np


# -- graphs -------------------------------------------------------------------
def make_nx(recipe):
    import networkx as nx
    kind = recipe[0]
    if kind == 'path':
        return nx.path_graph(recipe[1])
    if kind == 'ring':
        return nx.cycle_graph(recipe[1])
    if kind == 'star':                      # (n nodes, n - 1 leaves)
        return nx.star_graph(recipe[1] - 1)
    if kind == 'tree':                      # random tree, degrees <= 4
        _, n, seed = recipe
        rng = np.random.default_rng([n, seed])
        g = nx.Graph()
        g.add_node(0)
        for v in range(1, n):
            free = [u for u in range(v) if g.degree[u] < 4]
            g.add_edge(int(rng.choice(free)), v)
        return g
    if kind == 'deg':
        # caterpillar of n nodes with n4 nodes of degree 4, n3 of degree 3,
        # the other inner nodes of degree 2: the degree histogram -- all the
        # static layouts look at -- made to order
        _, n4, n3, n, _ = recipe
        n2 = n - 2 - 2 * n3 - 3 * n4
        spine = [4] * n4 + [3] * n3 + [2] * n2
        g = nx.path_graph(len(spine)) if spine else nx.Graph()
        nxt = len(spine)
        for u, d in enumerate(spine):
            for _ in range(d - (2 if 0 < u < len(spine) - 1 else 1)
                           + (len(spine) == 1)):
                g.add_edge(u, nxt)
                nxt += 1
        assert g.number_of_nodes() == n, (recipe, g.number_of_nodes())
        return g
    if kind == 'core':
        # n4 nodes of degree 4 and n3 of degree 3 joined among themselves
        # (Havel-Hakimi), the other n - n4 - n3 nodes pendant leaves dealt
        # round-robin onto them: unlike a tree, few leaves for many hubs
        _, n4, n3, n, _ = recipe
        g = nx.havel_hakimi_graph(_core_residual(n4, n3, n))
        nxt = n4 + n3
        for leaf in range(n - n4 - n3):
            g.add_edge(leaf % (n4 + n3), nxt)
            nxt += 1
        return g
    if kind == 'reg':
        _, d, n, seed = recipe
        return nx.random_regular_graph(d, n, seed=seed)
    if kind == 'nws':
        _, n, seed = recipe
        return nx.newman_watts_strogatz_graph(n, 5, 0.05, seed=seed)
    if kind == 'spoke':                     # a star of any size
        return nx.star_graph(recipe[1] - 1)
    if kind == 'hub':
        # a path whose first node has ten more neighbours (degree 11): the
        # sparsest graph the on-the-fly variants are for
        _, n, _ = recipe
        g = nx.path_graph(n)
        g.add_edges_from((0, u) for u in range(2, 12))
        return g
    if kind == 'dense':
        _, n, seed = recipe
        g = nx.gnp_random_graph(n, 0.9, seed=seed)
        for v in range(n):                  # (no isolated node)
            if g.degree[v] == 0:
                g.add_edge(v, (v + 1) % n)
        return g
    raise ValueError(recipe)


def _core_residual(n4, n3, n):
    """Degrees the hubs of a 'core' graph have among themselves."""
    m, leaves = n4 + n3, n - n4 - n3
    return [d - leaves // m - (u < leaves % m)
            for u, d in enumerate([4] * n4 + [3] * n3)]


def constructible(recipe):
    kind, n = recipe[0], recipe[-2] if len(recipe) > 2 else recipe[1]
    if kind == 'ring':
        return n >= 3
    if kind == 'star':
        return 3 <= n <= 5
    if kind == 'deg':
        n2 = n - 2 - 2 * recipe[2] - 3 * recipe[1]
        return n2 >= 0 and recipe[1] + recipe[2] + n2 >= 1
    if kind == 'core':
        import networkx as nx
        if recipe[1] + recipe[2] < 2 or n < recipe[1] + recipe[2]:
            return False
        res = _core_residual(recipe[1], recipe[2], n)
        return min(res) >= 1 and nx.is_graphical(res)
    if kind == 'reg':
        return recipe[1] < n and recipe[1] * n % 2 == 0
    if kind == 'nws':
        return n >= 8
    if kind == 'dense':
        return n >= 11
    if kind == 'hub':
        return n >= 12
    return n >= 2


def nodes_of(recipe):
    return recipe[1] if len(recipe) == 2 else recipe[-2]


def with_nodes(recipe, n):
    if len(recipe) == 2:
        return (recipe[0], n)
    return recipe[:-2] + (n, recipe[-1])


def make_graph(recipe):
    """The recipe's graph with the attributes of `cases.config2_graphs`."""
    from graphdot_amd.graph import Graph
    g = make_nx(tuple(recipe))
    rng = np.random.default_rng(zlib.crc32(repr(tuple(recipe)).encode()))
    for i in g.nodes:
        g.nodes[i]['radius'] = float(rng.choice([1.0, 1.5, 2.0]))
        g.nodes[i]['category'] = int(rng.choice([1, 2, 3]))
    for e in g.edges:
        g.edges[e]['w'] = float(rng.choice([0.5, 1.0, 2.0]))
        g.edges[e]['length'] = float(rng.uniform(0.5, 2.5))
    return Graph.from_networkx(g, weight='w')


def make_graphs(recipes):
    from graphdot_amd.graph import Graph
    return Graph.unify_datatype([make_graph(r) for r in recipes])


# -- the menu -------------------------------------------------------------------
REALS = {'f32': np.float32, 'f64': np.float64}
job_t = np.dtype([('i', np.uint32), ('j', np.uint32)])


def menu(real, C):
    """The entries under test for one arithmetic and C: the static layouts
    enabled on full images, the dynamic and on-the-fly owner-computes
    variants, the two-stage variants."""
    from graphdot_amd.kernel.marginalized._backend_hip import (
        HIPBackend, OC_VARIANTS, VARIANTS)
    b = HIPBackend(real=real)
    return [v for v in OC_VARIANTS + VARIANTS
            if not getattr(v, 'L', None) or b._static_enabled(v, C, quot=False)]


def kind_of(v):
    from graphdot_amd.kernel.marginalized._backend_hip import OCVariant
    if not isinstance(v, OCVariant):
        return 'two-stage'
    return 'static' if v.L else 'fly' if v.S == 0 else 'dynamic'


def variant_id(v):
    if kind_of(v) == 'two-stage':
        return 'W%dS%dR%d' % tuple(v)
    if v.L:
        return 'L' + 'x'.join(map(str, v.L))
    return 'oc%d_W%dS%dR%d' % (v.D, v.W, v.S, v.R)


def one_variant_backend(v, real, **kwargs):
    from graphdot_amd.kernel.marginalized._backend_hip import (
        HIPBackend, GENERAL)
    return HIPBackend(real=real, variants=[v, GENERAL], quotient=False,
                      min_launch=0, **kwargs)


def kernel_on(backend, real):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    kn, ke, q = cases.config2b_kernels()
    return MarginalizedGraphKernel(
        kn, ke, q=q, backend=backend,
        ftol=1e-8 if np.dtype(real) == np.float32 else 1e-13)


def triu_jobs(n):
    i, j = np.triu_indices(n)
    return np.column_stack((i, j)).astype(np.uint32).ravel().view(job_t)


def cross_jobs(pairs):
    return np.array(pairs, dtype=np.uint32).ravel().view(job_t)


def host_plan(backend, k, graphs, jobs, traits):
    return next(backend._host_plans(graphs, k.node_kernel, k.edge_kernel,
                                    jobs, traits))


def assignment(backend, k, graphs, jobs, traits):
    """Index into backend.variants of every job, as `prepare` decides it:
    the first host plan of the call (launch-wide LDS fit included)."""
    part = host_plan(backend, k, graphs, jobs, traits).part
    _, _, order, launches = part
    which = np.full(len(jobs), -1, dtype=np.int64)
    for L in launches:
        which[order[L['offset']:L['offset'] + L['count']]] = L['k']
    return which


def pair_metrics(backend, k, graphs, v, ii, jj, traits=None):
    """What the host rules look at for the jobs (ii, jj) of `graphs`, from
    the public host functions: N, padded rows NP, largest degrees, the slot
    walk (dynamic and two-stage variants) and the trips (static layouts)."""
    traits = traits or k.traits(symmetric=True)
    dg, _, _, _ = backend._graphs_and_kernels(
        graphs, k.node_kernel, k.edge_kernel, traits)
    from graphdot_amd.kernel.marginalized._devicegraph import graph_features
    f = graph_features(dg)
    ii, jj = np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)
    n, md = f['n_node'], f['max_degree']
    out = dict(n1=n[ii], n2=n[jj], N=n[ii] * n[jj],
               nnz1=f['n_nz'][ii], nnz2=f['n_nz'][jj],
               NP=n[ii] * (n[jj] | 1),
               deg_hi=np.maximum(md[ii], md[jj]),
               deg_lo=np.minimum(md[ii], md[jj]))
    what = kind_of(v)
    if what in ('dynamic', 'static'):
        ok = out['deg_hi'] <= v.D
        hist = np.zeros((len(dg), v.D + 1), dtype=np.int64)
        for g_, d_ in enumerate(dg):
            if md[g_] <= v.D:
                hist[g_] = np.bincount(d_.adjacency_count, minlength=v.D + 1)
        if what == 'dynamic':
            sl = np.full(len(ii), -1, dtype=np.int64)
            if ok.any():
                sl[ok] = backend.oc_slots_needed(hist[ii[ok]], hist[jj[ok]],
                                                 v.W, v.D)
            out['slots'] = sl
        else:
            tr = np.full((len(ii), backend.TRIP_BATCHES), -1, dtype=np.int64)
            if ok.any():
                tr[ok] = backend.oc_trips(hist[ii[ok]], hist[jj[ok]], v.D,
                                          backend.TRIP_BATCHES)
            out['trips'] = tr
    elif what == 'two-stage':
        deg_sorted = np.zeros((len(dg), int(n.max())), dtype=np.int64)
        for g_, d_ in enumerate(dg):
            deg_sorted[g_, :d_.n_node] = d_.adjacency_count
        out['slots'] = backend.slots_needed(f['n_nz'][ii], n[jj], jj,
                                            deg_sorted, v.W)
    return out


def edge_holds(name, v, m, t):
    """Does job t of the metrics `m` sit on edge `name` of variant v?"""
    from graphdot_amd.kernel.marginalized._backend_hip import (
        HIPBackend, FLY_MIN_DEGREE)
    W, R = v.W, v.R
    if name == 'full':
        return m['N'][t] <= 64 * W * R       # (== or the recorded largest)
    if name == 'one_row':
        return R > 1 and m['N'][t] == 64 * W * (R - 1) + 1
    if name == 'no_last':
        return R > 1 and m['N'][t] == 64 * W * (R - 1)
    if name == 'slots_full':
        return m['slots'][t] == v.S
    if name == 'max_degree':
        return m['deg_hi'][t] == v.D
    if name == 'trips_full':
        return tuple(m['trips'][t][:R]) == tuple(v.L) \
            and not m['trips'][t][R:].any()
    if name == 'trips_first':
        return R > 1 and m['trips'][t][0] == v.L[0] \
            and m['trips'][t][R - 1] == 0 and not m['trips'][t][R:].any()
    if name == 'grid':
        return (m['deg_hi'][t], m['deg_lo'][t]) == HIPBackend.grid_of(v.L, v.D)
    if name == 'stride':
        return m['n1'][t] % 2 == 0 and m['n2'][t] % 2 == 1
    if name == 'smallest':
        return True
    if name == 'dense':
        # both adjacency matrices more than ~60 % full: the rule of the dense
        # product (mgk_oc.h DENSE, `_classify_pairs`)
        return m['deg_hi'][t] > FLY_MIN_DEGREE and \
            23 * m['nnz1'][t] * m['nnz2'][t] > 9 * m['N'][t] ** 2
    raise KeyError(name)


def claimed(body):
    """The edges a fixture body sits on, in its set or as a cross call."""
    return set(body['edges']) | set(body.get('cross', {}))


def edges_of(v):
    """The edges a fixture of v may claim."""
    what = kind_of(v)
    out = ['full', 'stride', 'smallest']
    if v.R > 1:
        out += ['one_row', 'no_last']
    if what in ('dynamic', 'two-stage'):
        out += ['slots_full']
    if what in ('dynamic', 'static'):
        out += ['max_degree']
    if what == 'static':
        out += ['trips_full', 'grid'] + (['trips_first'] if v.R > 1 else [])
    if what == 'fly':
        out += ['dense']
    return out


# -- the search (not run at collection) -------------------------------------------
def _pool(v):
    """Candidate recipes for v, ascending in nodes."""
    what = kind_of(v)
    cap = 64 * v.W * v.R
    targets = {cap, cap - 64 * v.W, cap - 64 * v.W + 1}
    sizes = set(range(2, 41)) | set(range(44, 161, 4))
    for t in targets:
        if t > 1:
            sizes |= {d for d in range(2, 1200) if t % d == 0}
    # (the two-stage rule is on n1 (n2 | 1): odd partners just under the cap)
    if what == 'two-stage':
        for t in range(cap - 8, cap + 1):
            sizes |= {d for d in range(2, 400) if t % d == 0}
    sizes = sorted(s for s in sizes if 2 * s <= cap + 64)
    if what == 'fly' and cap <= 1024:
        # (no graph of more than 32 nodes in the launch: the kernels keep the
        # dense product of mgk_oc.h DENSE, `_dense_bytes`)
        sizes = [s for s in sizes if s <= 32]
    d4 = [('path',), ('ring',), ('star',), ('tree', 0), ('tree', 1),
          ('tree', 2), ('tree', 3), ('reg', 3, 0), ('reg', 4, 0)]
    d8 = [('nws', 0), ('reg', 5, 0), ('reg', 6, 0), ('reg', 7, 0),
          ('reg', 8, 0), ('path',)]
    if what == 'fly':
        fams = [('dense', 0), ('hub', 0), ('path',)]
    elif what == 'two-stage':
        fams = d4[:4] + [('reg', 4, 0)] + d8[:1] + [('reg', 8, 0)]
    else:
        fams = d4 if v.D == 4 else d8
    out = []
    for n in sizes:
        for fam in fams:
            if n > 160 and fam[0] not in ('path', 'ring', 'hub'):
                continue
            r = (fam[0],) + fam[1:-1] + (n, fam[-1]) if len(fam) > 1 \
                else (fam[0], n)
            if constructible(r):
                out.append(r)
    if what == 'two-stage':
        # a full slot walk in one batch: a hub of S neighbours (the walk does
        # not depend on N, and the LDS rule leaves some builds few rows)
        out.append(('spoke', v.S + 1, 0))
        out.sort(key=nodes_of)
    if what == 'static':
        # degree histograms made to order (the trips of every batch)
        for n4 in range(1, 9):
            for n3 in range(0, 4):
                for n2 in (0, 1, 2, 3, 5, 8, 13, 21, 34):
                    n = 3 * n4 + 2 * n3 + n2 + 2
                    if 2 * n <= cap + 64:
                        out.append(('deg', n4, n3, n, 0))
        for n4 in range(2, 9):
            for n3 in range(0, 5):
                for leaves in range(1, 21):
                    r = ('core', n4, n3, n4 + n3 + leaves, 0)
                    if constructible(r):
                        out.append(r)
        out.sort(key=nodes_of)
    return out


_GRAPH_CACHE = {}


def _graphs_cached(recipes):
    key = tuple(recipes)
    if key not in _GRAPH_CACHE:
        _GRAPH_CACHE[key] = make_graphs(recipes)
    return _GRAPH_CACHE[key]


def _classify(backend, k, graphs, ii, jj, C):
    """Variant index per pair by the rules of one pair (`classify`), under
    the call's own shape."""
    traits = k.traits(symmetric=True, eval_gradient=C == 2)
    dg, _, C_, fields = backend._graphs_and_kernels(
        graphs, k.node_kernel, k.edge_kernel, traits)
    arena = backend._host_arena(dg, fields)
    shape = backend._call_shape(arena, traits, C_, k.edge_kernel)
    return backend.classify(ii, jj, dg, C_, gtab=shape.gtab)[0]


def check_body(v, real, C, body):
    """Problems of a fixture body for (v, real, C): [] if every claimed edge
    holds, is given to v by the host plan of the symmetric call, the stride
    pair in both orders, and no pair beyond an edge is."""
    real = REALS.get(real, real)
    b = one_variant_backend(v, real)
    k = kernel_on(b, real)
    graphs = _graphs_cached(tuple(map(tuple, body['graphs'])))
    traits = k.traits(symmetric=True, eval_gradient=C == 2)
    jobs = triu_jobs(len(graphs))
    which = assignment(b, k, graphs, jobs, traits)
    m = pair_metrics(b, k, graphs, v, jobs['i'], jobs['j'], traits)
    at = {(int(a), int(c)): t for t, (a, c) in enumerate(jobs.tolist())}
    bad = []
    for name, (i, j) in body['edges'].items():
        t = at[(i, j)]
        if which[t] != 0:
            bad.append(f'{name}: pair {i, j} not given to the variant')
        if not edge_holds(name, v, m, t):
            bad.append(f'{name}: pair {i, j} is off the edge')
        if name == 'full' and (int(m['N'][t]) != body['N_full'] or int(
                m['N'][which == 0].max()) != body['N_full']):
            bad.append(f'full: N = {int(m["N"][t])}, recorded '
                       f'{body["N_full"]}')
        if name == 'stride':
            tr = k.traits(eval_gradient=C == 2)
            w2 = assignment(b, k, graphs, cross_jobs([(i, j), (j, i)]), tr)
            if w2.tolist() != [0, 0]:
                bad.append(f'stride: orders of {i, j} go to {w2.tolist()}')
    for name, (ra, rb) in body.get('beyond', {}).items():
        g2 = _graphs_cached((tuple(ra), tuple(rb)))
        w2 = assignment(b, k, g2, cross_jobs([(0, 1)]), traits)
        if w2[0] == 0:
            bad.append(f'beyond {name}: {ra} x {rb} is given to the variant')
    for name, (ra, rb) in body.get('cross', {}).items():
        if not cross_pair_taken(v, real, C, name, ra, rb):
            bad.append(f'cross {name}: {ra} x {rb} is off the edge or not '
                       'given to the variant')
    return bad


def cross_pair_taken(v, real, C, name, ra, rb):
    """Is the cross call k([a], [b]) the variant's, and on edge `name`?"""
    real = REALS.get(real, real)
    b = one_variant_backend(v, real)
    k = kernel_on(b, real)
    g2 = _graphs_cached((tuple(ra), tuple(rb)))
    tr = k.traits(eval_gradient=C == 2)
    w2 = assignment(b, k, g2, cross_jobs([(0, 1)]), tr)
    m2 = pair_metrics(b, k, g2, v, [0], [1], tr)
    return bool(w2[0] == 0 and edge_holds(name, v, m2, 0))


def row_target(v, name):
    """N of the edges `one_row` and `no_last`."""
    return 64 * v.W * (v.R - 1) + (name == 'one_row')


def factor_pairs(v, target):
    """The sparsest pairs of `target` rows: for every factorisation a b
    (a, b >= 2), in both orders, two paths -- for the on-the-fly variants a
    'hub' graph (a path with one node of degree 11, from 12 nodes on) and a
    path, or two hub graphs."""
    out = []
    for a in range(2, int(target ** 0.5) + 1):
        if target % a:
            continue
        for x, y in {(a, target // a), (target // a, a)}:
            if kind_of(v) == 'fly':
                # (a node of more than FLY_MIN_DEGREE neighbours in either)
                for ra, rb in ((('hub', x, 0), ('path', y)),
                               (('path', x), ('hub', y, 0)),
                               (('hub', x, 0), ('hub', y, 0))):
                    if constructible(ra) and constructible(rb):
                        out.append((ra, rb))
            else:
                out.append((('path', x), ('path', y)))
    return out


def next_pair_up(b, k, traits, a, c):
    """The pair (a, c) with one graph a node larger -- two where its
    generator has no graph of that size, a path of one node more where it
    has neither -- that the variant does not take, or None."""
    for ra, rc in ((a, with_nodes(c, nodes_of(c) + 1)),
                   (a, with_nodes(c, nodes_of(c) + 2)),
                   (with_nodes(a, nodes_of(a) + 1), c),
                   (with_nodes(a, nodes_of(a) + 2), c),
                   (a, ('path', nodes_of(c) + 1)),
                   (('path', nodes_of(a) + 1), c)):
        if constructible(ra) and constructible(rc):
            w2 = assignment(b, k, _graphs_cached((ra, rc)),
                            cross_jobs([(0, 1)]), traits)
            if w2[0] != 0:
                return (ra, rc)
    return None


def _largest_is_full(v, real, C, body):
    """`full` is the largest pair of the set that the variant gets: after
    the full pair has descended in N, a pair between two graphs chosen for
    other edges (a graph with itself) may be larger."""
    b = one_variant_backend(v, real)
    k = kernel_on(b, real)
    graphs = _graphs_cached(tuple(map(tuple, body['graphs'])))
    traits = k.traits(symmetric=True, eval_gradient=C == 2)
    jobs = triu_jobs(len(graphs))
    which = assignment(b, k, graphs, jobs, traits)
    m = pair_metrics(b, k, graphs, v, jobs['i'], jobs['j'], traits)
    N = np.where(which == 0, m['N'], -1)
    t = int(N.argmax())
    if N[t] > body['N_full'] or 'full' not in body['beyond']:
        i, j = int(jobs['i'][t]), int(jobs['j'][t])
        body['edges']['full'], body['N_full'] = (i, j), int(N[t])
        up = next_pair_up(b, k, traits, tuple(body['graphs'][i]),
                          tuple(body['graphs'][j]))
        body['beyond'].pop('full', None)
        if up:
            body['beyond']['full'] = up


def _search_one(v, real, C, log=None):
    """A fixture body for (v, real, C) or None if v takes no pair."""
    b = one_variant_backend(v, real)
    k = kernel_on(b, real)
    pool = _pool(v)
    graphs = _graphs_cached(tuple(pool))
    n = np.array([nodes_of(r) for r in pool])
    cap = 64 * v.W * v.R
    ii, jj = np.triu_indices(len(pool))
    keep = n[ii] * n[jj] <= cap + 320
    ii, jj = ii[keep], jj[keep]
    ch = _classify(b, k, graphs, ii, jj, C)
    m = pair_metrics(b, k, graphs, v, ii, jj)
    N = m['N']
    nnz = np.array([2 * g.number_of_edges() for g in map(make_nx, pool)],
                   dtype=np.float64)
    traits = k.traits(symmetric=True, eval_gradient=C == 2)
    # what the whole set refused (the launch sizes its LDS regions for the
    # largest vector and the largest image among its pairs): pairs, by edge;
    # an edge refused twelve times is not claimed; the full pair descends in N
    banned, fails, n_top = set(), {}, cap
    for _ in range(160):
        mine = np.array([t for t in np.flatnonzero(ch == 0) if N[t] <= n_top],
                        dtype=np.int64)
        if not len(mine):
            return None
        chosen, edges, beyond = [], {}, {}

        def cost(t):
            # what the pair adds to the reference of the whole set: every
            # pair between its new graphs and the set's costs the oracle a
            # Python loop over nnz x nnz and, up to 3072 rows, a dense solve
            new = {int(ii[t]), int(jj[t])} - set(chosen)
            old = list(chosen)
            total = 0.0
            for g in sorted(new):
                for h in old + [g]:
                    rows = float(n[g] * n[h])
                    total += 5e-6 * nnz[g] * nnz[h] + (
                        1e-10 * rows ** 3 if rows <= 3072 else 1e-5 * rows)
                old.append(g)
            return (total, int(n[ii[t]] + n[jj[t]]))

        def take(name, cand):
            cand = [t for t in cand if (name, int(t)) not in banned
                    and fails.get(name, 0) < 12 and edge_holds(name, v, m, t)]
            if not cand:
                return None
            if name == 'dense':
                # the largest dense pair that adds little to the reference
                # of the set (the estimate of `cost`, about seconds)
                small_ = [t for t in cand if cost(t)[0] <= 0.6]
                t = max(small_ or cand, key=lambda t: (
                    int(N[t]) if small_ else -int(N[t]), -cost(t)[0]))
            else:
                t = min(cand, key=cost)
            for g in (int(ii[t]), int(jj[t])):
                if g not in chosen:
                    chosen.append(g)
            edges[name] = (int(ii[t]), int(jj[t]), int(t))
            return t

        # the large pairs first: later edges re-use their graphs
        top = int(N[mine].max())
        t_full = take('full', [t for t in mine if N[t] == top])
        for name in edges_of(v):
            if name in ('one_row', 'no_last'):
                # (a graph of several hundred nodes costs the reference of
                # the symmetric set its pair with itself: a cross call below)
                take(name, [t for t in mine if n[jj[t]] <= 200])
            elif name not in ('full', 'smallest', 'stride'):
                take(name, mine)
        # stride: both orders must be the variant's
        cand = [t for t in mine if edge_holds('stride', v, m, t)]
        if cand:
            rev = _classify(b, k, graphs, jj[cand], ii[cand], C)
            take('stride', [t for t, r in zip(cand, rev) if r == 0])
        small = int(N[mine].min())
        take('smallest', [t for t in mine if N[t] == small])
        # the next pair up: one node more in either graph
        up = next_pair_up(b, k, traits, pool[int(ii[t_full])],
                          pool[int(jj[t_full])])
        if up:
            beyond['full'] = up
        if 'slots_full' in edges:
            over = [t for t in range(len(ii))
                    if m['slots'][t] > v.S and N[t] <= cap and ch[t] != 0
                    and (kind_of(v) == 'two-stage' or m['deg_hi'][t] <= v.D)]
            if over:
                t = min(over, key=lambda t: (int(m['slots'][t]), int(N[t]),
                                             int(n[ii[t]] + n[jj[t]])))
                beyond['slots_full'] = (pool[int(ii[t])], pool[int(jj[t])])
        # the row edges the set does not sit on: as a cross call k([a], [b]),
        # from the pool or from the sparsest pairs of every factorisation
        cross = {}
        # (and a full slot walk that the launch of the set refuses: its
        # graphs' images and the full pair's vector do not fit one launch)
        for name in ('one_row', 'no_last', 'slots_full'):
            if name not in edges_of(v) or name in edges:
                continue
            cand = [(pool[int(ii[t])], pool[int(jj[t])]) for t in mine
                    if edge_holds(name, v, m, t)]
            cand.sort(key=lambda p: nodes_of(p[0]) + nodes_of(p[1]))
            more = factor_pairs(v, row_target(v, name)) \
                if name != 'slots_full' else []
            for ra, rb in cand[:4] + more:
                if cross_pair_taken(v, real, C, name, ra, rb):
                    cross[name] = (ra, rb)
                    break
        order = sorted(chosen)             # (ascending in nodes: i <= j kept)
        pos = {g: p for p, g in enumerate(order)}
        body = dict(graphs=[pool[g] for g in order],
                    edges={name: (pos[a_], pos[c_])
                           for name, (a_, c_, _) in edges.items()},
                    N_full=top, beyond=beyond, cross=cross)
        _largest_is_full(v, real, C, body)
        bad = check_body(v, real, C, body)
        if not bad:
            return body
        if log:
            log(f'  retry {variant_id(v)} {real.__name__} C{C}: {bad}')
        for line in bad:
            name = line.split(':')[0]
            if name.startswith(('beyond', 'cross')):
                raise AssertionError(line)
            banned.add((name, edges[name][2]))
            if name == 'full':
                n_top = top - 1
            else:
                fails[name] = fails.get(name, 0) + 1
    return None


def search(log=print, only=None):
    """FOUND: {variant id: (bodies, {'f32/1': index into bodies or None})}.
    `only`: the kinds of variants to search for."""
    found = {}
    seen = []
    for rname, real in REALS.items():
        for C in (2, 1):
            for v in menu(real, C):
                if v not in seen:
                    seen.append(v)
    for v in seen:
        if only and kind_of(v) not in only and variant_id(v) not in only:
            continue
        bodies, where = [], {}
        for rname, real in (('f64', np.float64), ('f32', np.float32)):
            for C in (2, 1):
                if v not in menu(real, C):
                    continue
                key = f'{rname}/{C}'
                # a set is shared between builds only where it sits on
                # every edge; otherwise this build is searched by itself
                hit = None
                for n_, body in enumerate(bodies):
                    if claimed(body) == set(edges_of(v)) \
                            and not check_body(v, real, C, body):
                        hit = n_
                        break
                if hit is None:
                    body = _search_one(v, real, C, log)
                    if body is not None and body in bodies:
                        hit = bodies.index(body)
                    elif body is not None:
                        bodies.append(body)
                        hit = len(bodies) - 1
                where[key] = hit
        found[variant_id(v)] = (bodies, where)
        log(f'{variant_id(v)}: {len(bodies)} sets, {where}, edges ' + '; '.join(
            ','.join(sorted(claimed(b_))) + f' N={b_["N_full"]}'
            for b_ in bodies))
    return found


#: the search's result (see the module docstring)
FOUND = {'L16': ([{'graphs': [('path', 2), ('star', 5), ('path', 8)],
           'edges': {'full': (2, 2),
                     'max_degree': (1, 1),
                     'trips_full': (1, 1),
                     'grid': (1, 1),
                     'stride': (0, 1),
                     'smallest': (0, 0)},
           'N_full': 64,
           'beyond': {'full': (('path', 8), ('path', 9))},
           'cross': {}}],
         {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4': ([{'graphs': [('path', 2), ('path', 5), ('reg', 4, 5, 0),
                        ('path', 8), ('path', 13), ('core', 2, 3, 16, 0)],
             'edges': {'full': (3, 5),
                       'one_row': (1, 4),
                       'no_last': (3, 3),
                       'max_degree': (1, 5),
                       'trips_full': (2, 5),
                       'grid': (2, 2),
                       'trips_first': (2, 2),
                       'stride': (3, 4),
                       'smallest': (0, 0)},
             'N_full': 128,
             'beyond': {'full': (('path', 9), ('core', 2, 3, 16, 0))},
             'cross': {}}],
           {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x1': ([{'graphs': [('path', 2), ('path', 3), ('path', 8),
                          ('core', 3, 2, 9, 0), ('tree', 12, 0),
                          ('core', 2, 3, 16, 0), ('path', 43)],
               'edges': {'full': (4, 5),
                         'one_row': (1, 6),
                         'no_last': (2, 5),
                         'max_degree': (1, 4),
                         'trips_full': (3, 5),
                         'grid': (3, 3),
                         'trips_first': (3, 3),
                         'stride': (2, 3),
                         'smallest': (0, 0)},
               'N_full': 192,
               'beyond': {'full': (('tree', 13, 0), ('core', 2, 3, 16, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x4': ([{'graphs': [('path', 2), ('path', 3), ('star', 5), ('path', 8),
                          ('reg', 4, 9, 0), ('path', 12),
                          ('core', 2, 3, 16, 0), ('path', 43)],
               'edges': {'full': (5, 6),
                         'one_row': (1, 7),
                         'no_last': (3, 6),
                         'max_degree': (1, 6),
                         'trips_full': (4, 6),
                         'grid': (4, 6),
                         'trips_first': (2, 2),
                         'stride': (3, 4),
                         'smallest': (0, 0)},
               'N_full': 192,
               'beyond': {'full': (('path', 13), ('core', 2, 3, 16, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x4x1': ([{'graphs': [('path', 2), ('star', 5), ('path', 12),
                            ('core', 6, 0, 14, 0), ('core', 2, 3, 16, 0)],
                 'edges': {'full': (4, 4),
                           'no_last': (2, 4),
                           'max_degree': (2, 4),
                           'trips_full': (3, 3),
                           'grid': (3, 3),
                           'trips_first': (1, 1),
                           'stride': (0, 1),
                           'smallest': (0, 0)},
                 'N_full': 256,
                 'beyond': {'full': (('core', 2, 3, 16, 0), ('path', 17))},
                 'cross': {}}],
               {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x4x1x1': ([{'graphs': [('path', 2), ('path', 3), ('core', 6, 0, 14, 0),
                              ('core', 2, 3, 16, 0), ('core', 2, 4, 20, 0)],
                   'edges': {'full': (3, 4),
                             'no_last': (3, 3),
                             'max_degree': (3, 3),
                             'trips_full': (2, 4),
                             'grid': (2, 2),
                             'trips_first': (2, 2),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 320,
                   'beyond': {'full': (('core', 2, 3, 16, 0), ('path', 21))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x4x3x1': ([{'graphs': [('path', 2), ('core', 5, 4, 13, 0),
                              ('core', 2, 3, 16, 0), ('core', 2, 4, 20, 0)],
                   'edges': {'full': (2, 3),
                             'no_last': (2, 2),
                             'max_degree': (2, 2),
                             'trips_full': (1, 3),
                             'grid': (1, 2),
                             'trips_first': (1, 2),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 320,
                   'beyond': {'full': (('core', 2, 3, 16, 0), ('path', 21))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x4x3x1x1': ([{'graphs': [('path', 2), ('path', 3), ('tree', 10, 0),
                                ('core', 3, 1, 11, 0), ('core', 2, 3, 16, 0),
                                ('core', 4, 3, 24, 0), ('tree', 32, 1),
                                ('tree', 107, 0)],
                     'edges': {'full': (4, 5),
                               'one_row': (1, 7),
                               'no_last': (2, 6),
                               'max_degree': (1, 2),
                               'trips_full': (3, 6),
                               'grid': (2, 2),
                               'trips_first': (2, 2),
                               'stride': (2, 3),
                               'smallest': (0, 0)},
                     'N_full': 384,
                     'beyond': {'full': (('core', 2, 3, 16, 0), ('path', 25))},
                     'cross': {}}],
                   {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x4x4x1x1x1': ([{'graphs': [('path', 2), ('deg', 1, 3, 11, 0),
                                  ('core', 6, 0, 14, 0), ('core', 2, 3, 16, 0),
                                  ('core', 4, 3, 24, 0), ('core', 4, 4, 28, 0),
                                  ('deg', 8, 2, 35, 0)],
                       'edges': {'full': (3, 5),
                                 'one_row': (1, 6),
                                 'no_last': (3, 4),
                                 'max_degree': (1, 1),
                                 'trips_full': (2, 5),
                                 'grid': (1, 1),
                                 'trips_first': (1, 1),
                                 'stride': (0, 1),
                                 'smallest': (0, 0)},
                       'N_full': 448,
                       'beyond': {'full': (('core', 2, 3, 16, 0),
                                           ('path', 29))},
                       'cross': {}}],
                     {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x4x4x3x1x1x1': ([{'graphs': [('path', 2), ('core', 2, 2, 14, 0),
                                    ('deg', 3, 2, 15, 0),
                                    ('core', 2, 3, 16, 0),
                                    ('deg', 8, 2, 32, 0)],
                         'edges': {'full': (3, 4),
                                   'no_last': (1, 4),
                                   'max_degree': (1, 1),
                                   'trips_full': (2, 4),
                                   'grid': (1, 1),
                                   'trips_first': (1, 1),
                                   'stride': (1, 2),
                                   'smallest': (0, 0)},
                         'N_full': 512,
                         'beyond': {'full': (('core', 2, 3, 16, 0),
                                             ('deg', 8, 2, 33, 0))},
                         'cross': {}}],
                       {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'L16x4x4x4x4x1x1x1x1': ([{'graphs': [('path', 2), ('core', 2, 3, 16, 0),
                                      ('core', 3, 3, 19, 0),
                                      ('core', 8, 0, 20, 0),
                                      ('core', 4, 3, 24, 0),
                                      ('core', 5, 3, 27, 0),
                                      ('deg', 8, 2, 32, 0)],
                           'edges': {'full': (4, 4),
                                     'one_row': (2, 5),
                                     'no_last': (1, 6),
                                     'max_degree': (1, 1),
                                     'trips_full': (3, 5),
                                     'grid': (1, 1),
                                     'trips_first': (1, 1),
                                     'stride': (1, 2),
                                     'smallest': (0, 0)},
                           'N_full': 576,
                           'beyond': {'full': (('core', 4, 3, 24, 0),
                                               ('path', 25))},
                           'cross': {}}],
                         {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S12R2': ([{'graphs': [('path', 2), ('star', 4), ('path', 5),
                              ('star', 5), ('path', 8), ('path', 13),
                              ('path', 16)],
                   'edges': {'full': (4, 6),
                             'one_row': (2, 5),
                             'no_last': (4, 4),
                             'slots_full': (1, 3),
                             'max_degree': (1, 3),
                             'stride': (1, 2),
                             'smallest': (0, 0)},
                   'N_full': 128,
                   'beyond': {'full': (('path', 8), ('path', 17)),
                              'slots_full': (('star', 5), ('tree', 13, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S16R3': ([{'graphs': [('path', 2), ('path', 3), ('star', 5),
                              ('path', 8), ('path', 12), ('path', 16),
                              ('path', 43)],
                   'edges': {'full': (4, 5),
                             'one_row': (1, 6),
                             'no_last': (3, 5),
                             'slots_full': (2, 2),
                             'max_degree': (1, 2),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 192,
                   'beyond': {'full': (('path', 12), ('path', 17)),
                              'slots_full': (('star', 5), ('tree', 13, 1))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S20R3': ([{'graphs': [('path', 2), ('path', 3), ('path', 8),
                              ('path', 12), ('tree', 12, 0), ('path', 16),
                              ('path', 43)],
                   'edges': {'full': (3, 5),
                             'one_row': (1, 6),
                             'no_last': (2, 5),
                             'slots_full': (4, 4),
                             'max_degree': (1, 4),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 192,
                   'beyond': {'full': (('path', 12), ('path', 17)),
                              'slots_full': (('reg', 3, 10, 0),
                                             ('tree', 13, 1))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S20R4': ([{'graphs': [('path', 2), ('path', 3), ('path', 12),
                              ('tree', 12, 0), ('path', 16)],
                   'edges': {'full': (4, 4),
                             'no_last': (2, 4),
                             'slots_full': (3, 3),
                             'max_degree': (2, 3),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 256,
                   'beyond': {'full': (('path', 16), ('path', 17)),
                              'slots_full': (('reg', 3, 10, 0),
                                             ('tree', 13, 1))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S24R4': ([{'graphs': [('path', 2), ('path', 3), ('path', 12),
                              ('path', 16), ('tree', 16, 1)],
                   'edges': {'full': (3, 3),
                             'no_last': (2, 3),
                             'slots_full': (4, 4),
                             'max_degree': (2, 4),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 256,
                   'beyond': {'full': (('path', 16), ('path', 17)),
                              'slots_full': (('tree', 13, 1),
                                             ('tree', 19, 1))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S28R5': ([{'graphs': [('path', 2), ('path', 3), ('reg', 4, 10, 0),
                              ('path', 16), ('path', 20)],
                   'edges': {'full': (3, 4),
                             'no_last': (3, 3),
                             'slots_full': (2, 4),
                             'max_degree': (2, 3),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 320,
                   'beyond': {'full': (('path', 16), ('path', 21)),
                              'slots_full': (('reg', 3, 10, 0),
                                             ('tree', 24, 1))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S28R6': ([{'graphs': [('path', 2), ('path', 3), ('path', 10),
                              ('reg', 4, 13, 0), ('path', 16), ('path', 24),
                              ('path', 32), ('path', 107)],
                   'edges': {'full': (4, 5),
                             'one_row': (1, 7),
                             'no_last': (2, 6),
                             'slots_full': (3, 4),
                             'max_degree': (1, 3),
                             'stride': (2, 3),
                             'smallest': (0, 0)},
                   'N_full': 384,
                   'beyond': {'full': (('path', 16), ('path', 25)),
                              'slots_full': (('tree', 14, 1),
                                             ('tree', 23, 2))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S32R7': ([{'graphs': [('path', 2), ('reg', 4, 6, 0), ('path', 11),
                              ('path', 16), ('path', 24), ('path', 28),
                              ('path', 35)],
                   'edges': {'full': (3, 5),
                             'one_row': (2, 6),
                             'no_last': (3, 4),
                             'slots_full': (1, 6),
                             'max_degree': (1, 1),
                             'stride': (1, 2),
                             'smallest': (0, 0)},
                   'N_full': 448,
                   'beyond': {'full': (('path', 16), ('path', 29)),
                              'slots_full': (('reg', 3, 10, 0),
                                             ('tree', 26, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc4_W1S36R9': ([{'graphs': [('path', 2), ('star', 5), ('reg', 3, 12, 0),
                              ('path', 16), ('path', 19), ('path', 24),
                              ('path', 27), ('path', 32)],
                   'edges': {'full': (5, 5),
                             'one_row': (4, 6),
                             'no_last': (3, 7),
                             'slots_full': (2, 7),
                             'max_degree': (1, 1),
                             'stride': (2, 4),
                             'smallest': (0, 0)},
                   'N_full': 576,
                   'beyond': {'full': (('path', 24), ('path', 25)),
                              'slots_full': (('tree', 12, 1),
                                             ('tree', 36, 1))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W1S32R3': ([{'graphs': [('path', 2), ('path', 3), ('path', 8),
                              ('nws', 9, 0), ('reg', 8, 9, 0), ('path', 12),
                              ('path', 16), ('path', 43)],
                   'edges': {'full': (5, 6),
                             'one_row': (1, 7),
                             'no_last': (2, 6),
                             'slots_full': (3, 3),
                             'max_degree': (1, 4),
                             'stride': (2, 3),
                             'smallest': (0, 0)},
                   'N_full': 192,
                   'beyond': {'full': (('path', 12), ('path', 17)),
                              'slots_full': (('reg', 5, 6, 0),
                                             ('reg', 7, 8, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W1S48R5': ([{'graphs': [('path', 2), ('reg', 8, 9, 0), ('nws', 12, 0),
                              ('path', 16), ('path', 20)],
                   'edges': {'full': (3, 4),
                             'no_last': (3, 3),
                             'slots_full': (2, 2),
                             'max_degree': (1, 3),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 320,
                   'beyond': {'full': (('path', 16), ('path', 21)),
                              'slots_full': (('reg', 7, 8, 0),
                                             ('reg', 7, 8, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W1S64R9': ([{'graphs': [('path', 2), ('reg', 8, 9, 0), ('nws', 14, 0),
                              ('path', 16), ('path', 19), ('path', 24),
                              ('path', 27), ('path', 32)],
                   'edges': {'full': (5, 5),
                             'one_row': (4, 6),
                             'no_last': (3, 7),
                             'slots_full': (2, 2),
                             'max_degree': (1, 2),
                             'stride': (2, 4),
                             'smallest': (0, 0)},
                   'N_full': 576,
                   'beyond': {'full': (('path', 24), ('path', 25)),
                              'slots_full': (('reg', 5, 6, 0),
                                             ('nws', 22, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W4S32R3': ([{'graphs': [('path', 2), ('nws', 8, 0), ('path', 8),
                              ('reg', 8, 9, 0), ('path', 9), ('path', 12),
                              ('path', 57), ('path', 64)],
                   'edges': {'full': (5, 7),
                             'one_row': (4, 6),
                             'no_last': (2, 7),
                             'slots_full': (1, 3),
                             'max_degree': (1, 3),
                             'stride': (1, 3),
                             'smallest': (0, 0)},
                   'N_full': 768,
                   'beyond': {'full': (('path', 12), ('path', 65)),
                              'slots_full': (('reg', 5, 6, 0),
                                             ('reg', 7, 8, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W4S40R2': ([{'graphs': [('path', 2), ('path', 4), ('reg', 5, 6, 0),
                              ('path', 8), ('reg', 8, 9, 0), ('path', 64)],
                   'edges': {'full': (3, 5),
                             'no_last': (1, 5),
                             'slots_full': (2, 4),
                             'max_degree': (1, 4),
                             'stride': (1, 4),
                             'smallest': (0, 0)},
                   'N_full': 512,
                   'beyond': {'full': (('path', 8), ('path', 65)),
                              'slots_full': (('nws', 18, 0), ('nws', 25, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W4S48R4': ([{'graphs': [('path', 2), ('reg', 6, 7, 0), ('reg', 8, 9, 0),
                              ('path', 24), ('path', 32)],
                   'edges': {'full': (4, 4),
                             'no_last': (3, 4),
                             'slots_full': (1, 2),
                             'max_degree': (1, 2),
                             'stride': (0, 1),
                             'smallest': (0, 0)},
                   'N_full': 1024,
                   'beyond': {'full': (('path', 32), ('path', 33)),
                              'slots_full': (('reg', 7, 8, 0),
                                             ('reg', 7, 8, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W4S64R5': ([{'graphs': [('path', 2), ('reg', 8, 9, 0), ('path', 16),
                              ('path', 20), ('path', 25), ('path', 41),
                              ('path', 64)],
                   'edges': {'full': (3, 6),
                             'one_row': (4, 5),
                             'no_last': (2, 6),
                             'slots_full': (1, 1),
                             'max_degree': (1, 1),
                             'stride': (2, 4),
                             'smallest': (0, 0)},
                   'N_full': 1280,
                   'beyond': {'full': (('path', 20), ('path', 65)),
                              'slots_full': (('nws', 20, 0),
                                             ('reg', 5, 26, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W8S40R2': ([{'graphs': [('path', 2), ('reg', 5, 6, 0), ('reg', 8, 9, 0),
                              ('path', 16), ('path', 19), ('path', 27),
                              ('path', 32)],
                   'edges': {'full': (6, 6),
                             'one_row': (4, 5),
                             'no_last': (3, 6),
                             'slots_full': (1, 2),
                             'max_degree': (1, 2),
                             'stride': (1, 2),
                             'smallest': (0, 0)},
                   'N_full': 1024,
                   'beyond': {'full': (('path', 32), ('path', 33)),
                              'slots_full': (('nws', 31, 0), ('nws', 31, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W8S48R3': ([{'graphs': [('path', 2), ('reg', 6, 7, 0), ('reg', 8, 9, 0),
                              ('path', 16), ('path', 24), ('path', 25),
                              ('path', 41), ('path', 64)],
                   'edges': {'full': (4, 7),
                             'one_row': (5, 6),
                             'no_last': (3, 7),
                             'slots_full': (1, 2),
                             'max_degree': (1, 2),
                             'stride': (3, 5),
                             'smallest': (0, 0)},
                   'N_full': 1536,
                   'beyond': {'full': (('path', 24), ('path', 65)),
                              'slots_full': (('reg', 7, 8, 0),
                                             ('reg', 7, 8, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W8S64R4': ([{'graphs': [('path', 2), ('reg', 8, 9, 0), ('path', 24),
                              ('path', 29), ('path', 32), ('path', 53),
                              ('path', 64)],
                   'edges': {'full': (4, 6),
                             'one_row': (3, 5),
                             'no_last': (2, 6),
                             'slots_full': (1, 1),
                             'max_degree': (1, 1),
                             'stride': (2, 3),
                             'smallest': (0, 0)},
                   'N_full': 2048,
                   'beyond': {'full': (('path', 32), ('path', 65)),
                              'slots_full': (('nws', 27, 0),
                                             ('reg', 5, 38, 0))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W16S32R2': ([{'graphs': [('path', 2), ('nws', 8, 0), ('reg', 8, 9, 0),
                               ('path', 25), ('path', 32), ('path', 41),
                               ('path', 64)],
                    'edges': {'full': (4, 6),
                              'one_row': (3, 5),
                              'no_last': (4, 4),
                              'slots_full': (1, 2),
                              'max_degree': (1, 2),
                              'stride': (1, 2),
                              'smallest': (0, 0)},
                    'N_full': 2048,
                    'beyond': {'full': (('path', 32), ('path', 65)),
                               'slots_full': (('reg', 5, 6, 0),
                                              ('reg', 7, 8, 0))},
                    'cross': {}}],
                  {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W16S40R2': ([{'graphs': [('path', 2), ('reg', 5, 6, 0), ('reg', 8, 9, 0),
                               ('path', 25), ('path', 32), ('path', 41),
                               ('path', 64)],
                    'edges': {'full': (4, 6),
                              'one_row': (3, 5),
                              'no_last': (4, 4),
                              'slots_full': (1, 2),
                              'max_degree': (1, 2),
                              'stride': (1, 2),
                              'smallest': (0, 0)},
                    'N_full': 2048,
                    'beyond': {'full': (('path', 32), ('path', 65)),
                               'slots_full': (('nws', 28, 0), ('nws', 72, 0))},
                    'cross': {}}],
                  {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc8_W16S48R3': ([{'graphs': [('path', 2), ('reg', 6, 7, 0), ('reg', 8, 9, 0),
                               ('path', 32), ('path', 64), ('path', 96)],
                    'edges': {'full': (3, 5),
                              'no_last': (3, 4),
                              'slots_full': (1, 2),
                              'max_degree': (1, 2),
                              'stride': (0, 1),
                              'smallest': (0, 0)},
                    'N_full': 3072,
                    'beyond': {'full': (('path', 32), ('path', 97)),
                               'slots_full': (('reg', 7, 8, 0),
                                              ('reg', 7, 8, 0))},
                    'cross': {}},
                   {'graphs': [('path', 2), ('reg', 6, 7, 0), ('reg', 8, 9, 0),
                               ('path', 32), ('path', 64), ('path', 96)],
                    'edges': {'full': (3, 5),
                              'no_last': (3, 4),
                              'slots_full': (1, 2),
                              'max_degree': (1, 2),
                              'stride': (0, 1),
                              'smallest': (0, 0)},
                    'N_full': 3072,
                    'beyond': {'full': (('path', 32), ('path', 97)),
                               'slots_full': (('reg', 7, 8, 0),
                                              ('reg', 7, 8, 0))},
                    'cross': {'one_row': (('path', 3), ('path', 683))}}],
                  {'f64/2': 0, 'f64/1': 1, 'f32/2': 1, 'f32/1': 1}),
 'oc8_W16S64R3': ([{'graphs': [('path', 2), ('reg', 8, 9, 0), ('path', 32),
                               ('path', 64), ('path', 96)],
                    'edges': {'full': (2, 4),
                              'no_last': (2, 3),
                              'slots_full': (1, 1),
                              'max_degree': (1, 1),
                              'stride': (0, 1),
                              'smallest': (0, 0)},
                    'N_full': 3072,
                    'beyond': {'full': (('path', 32), ('path', 97)),
                               'slots_full': (('nws', 27, 0),
                                              ('reg', 5, 76, 0))},
                    'cross': {}},
                   {'graphs': [('path', 2), ('reg', 8, 9, 0), ('path', 32),
                               ('path', 64), ('path', 96)],
                    'edges': {'full': (2, 4),
                              'no_last': (2, 3),
                              'slots_full': (1, 1),
                              'max_degree': (1, 1),
                              'stride': (0, 1),
                              'smallest': (0, 0)},
                    'N_full': 3072,
                    'beyond': {'full': (('path', 32), ('path', 97)),
                               'slots_full': (('nws', 27, 0),
                                              ('reg', 5, 76, 0))},
                    'cross': {'one_row': (('path', 3), ('path', 683))}}],
                  {'f64/2': 0, 'f64/1': 0, 'f32/2': 1, 'f32/1': 1}),
 'oc0_W4S0R1': ([{'graphs': [('path', 2), ('dense', 11, 0), ('hub', 13, 0),
                             ('dense', 16, 0), ('hub', 16, 0)],
                  'edges': {'full': (4, 4),
                            'dense': (3, 3),
                            'stride': (0, 2),
                            'smallest': (0, 1)},
                  'N_full': 256,
                  'beyond': {'full': (('hub', 16, 0), ('hub', 17, 0))},
                  'cross': {}}],
                {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc0_W4S0R2': ([{'graphs': [('path', 2), ('dense', 11, 0), ('hub', 16, 0),
                             ('path', 17), ('dense', 18, 0), ('path', 32)],
                  'edges': {'full': (2, 5),
                            'no_last': (2, 2),
                            'dense': (4, 4),
                            'stride': (2, 3),
                            'smallest': (0, 1)},
                  'N_full': 512,
                  'beyond': {'full': (('hub', 16, 0), ('path', 33))},
                  'cross': {}}],
                {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc0_W4S0R3': ([{'graphs': [('path', 2), ('dense', 11, 0), ('dense', 16, 0),
                             ('hub', 16, 0), ('hub', 19, 0), ('hub', 24, 0),
                             ('path', 27), ('path', 32)],
                  'edges': {'full': (5, 7),
                            'one_row': (4, 6),
                            'no_last': (3, 7),
                            'dense': (2, 2),
                            'stride': (2, 4),
                            'smallest': (0, 1)},
                  'N_full': 768,
                  'beyond': {'full': (('hub', 24, 0), ('path', 33))},
                  'cross': {}}],
                {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc0_W8S0R2': ([{'graphs': [('path', 2), ('dense', 11, 0), ('path', 16),
                             ('dense', 17, 0), ('hub', 19, 0), ('path', 27),
                             ('hub', 32, 0)],
                  'edges': {'full': (6, 6),
                            'one_row': (4, 5),
                            'no_last': (2, 6),
                            'dense': (3, 3),
                            'stride': (2, 3),
                            'smallest': (0, 1)},
                  'N_full': 1024,
                  'beyond': {'full': (('hub', 32, 0), ('hub', 33, 0))},
                  'cross': {}}],
                {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc0_W16S0R2': ([{'graphs': [('path', 2), ('dense', 11, 0), ('dense', 14, 0),
                              ('hub', 25, 0), ('hub', 32, 0), ('path', 41),
                              ('path', 64)],
                   'edges': {'full': (4, 6),
                             'one_row': (3, 5),
                             'no_last': (4, 4),
                             'dense': (2, 2),
                             'stride': (2, 3),
                             'smallest': (0, 1)},
                   'N_full': 2048,
                   'beyond': {'full': (('hub', 32, 0), ('path', 65))},
                   'cross': {}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'oc0_W16S0R4': ([{'graphs': [('path', 2), ('dense', 11, 0), ('hub', 24, 0),
                              ('hub', 64, 0), ('path', 128)],
                   'edges': {'full': (3, 3),
                             'no_last': (2, 4),
                             'dense': (1, 1),
                             'stride': (0, 1),
                             'smallest': (0, 1)},
                   'N_full': 4096,
                   'beyond': {'full': (('hub', 64, 0), ('hub', 65, 0))},
                   'cross': {'one_row': (('path', 7), ('hub', 439, 0))}}],
                 {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S8R2': ([{'graphs': [('path', 2), ('path', 5), ('path', 6), ('path', 8),
                         ('path', 13), ('path', 21)],
              'edges': {'full': (2, 5),
                        'one_row': (1, 4),
                        'no_last': (3, 3),
                        'slots_full': (2, 5),
                        'stride': (2, 4),
                        'smallest': (0, 0)},
              'N_full': 126,
              'beyond': {'full': (('path', 6), ('path', 22)),
                         'slots_full': (('path', 2), ('nws', 22, 0))},
              'cross': {}}],
            {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S12R3': ([{'graphs': [('path', 2), ('path', 3), ('path', 8), ('path', 10),
                          ('path', 16), ('path', 19), ('path', 43)],
               'edges': {'full': (3, 5),
                         'one_row': (1, 6),
                         'no_last': (2, 4),
                         'slots_full': (3, 5),
                         'stride': (2, 5),
                         'smallest': (0, 0)},
               'N_full': 190,
               'beyond': {'full': (('path', 10), ('path', 20)),
                          'slots_full': (('ring', 3), ('nws', 19, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S16R4': ([{'graphs': [('path', 2), ('reg', 4, 7, 0), ('path', 12),
                          ('path', 15), ('path', 16), ('path', 17)],
               'edges': {'full': (3, 5),
                         'no_last': (2, 4),
                         'slots_full': (1, 1),
                         'stride': (2, 3),
                         'smallest': (0, 0)},
               'N_full': 255,
               'beyond': {'full': (('path', 15), ('path', 18)),
                          'slots_full': (('ring', 3), ('nws', 28, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S20R5': ([{'graphs': [('path', 2), ('reg', 4, 8, 0), ('path', 11),
                          ('path', 16), ('path', 29)],
               'edges': {'full': (2, 4),
                         'no_last': (3, 3),
                         'slots_full': (1, 1),
                         'stride': (1, 2),
                         'smallest': (0, 0)},
               'N_full': 319,
               'beyond': {'full': (('path', 11), ('path', 30)),
                          'slots_full': (('ring', 4), ('nws', 29, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S24R6': ([{'graphs': [('path', 2), ('path', 3), ('ring', 3), ('path', 5),
                          ('path', 64), ('path', 107), ('path', 191)],
               'edges': {'full': (0, 6),
                         'one_row': (1, 5),
                         'no_last': (3, 4),
                         'slots_full': (2, 5),
                         'stride': (0, 1),
                         'smallest': (0, 0)},
               'N_full': 382,
               'beyond': {'full': (('path', 2), ('path', 192)),
                          'slots_full': (('reg', 4, 5, 0), ('nws', 18, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S28R7': ([{'graphs': [('path', 2), ('path', 3), ('path', 5), ('path', 6),
                          ('reg', 4, 10, 0), ('path', 64), ('path', 77),
                          ('path', 149)],
               'edges': {'full': (1, 7),
                         'one_row': (2, 6),
                         'no_last': (3, 5),
                         'slots_full': (4, 4),
                         'stride': (0, 1),
                         'smallest': (0, 0)},
               'N_full': 447,
               'beyond': {'full': (('path', 3), ('path', 150)),
                          'slots_full': (('reg', 4, 5, 0), ('nws', 19, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S32R9': ([{'graphs': [('path', 2), ('reg', 4, 11, 0), ('path', 16),
                          ('path', 19), ('path', 27), ('path', 32),
                          ('path', 287)],
               'edges': {'full': (0, 6),
                         'one_row': (3, 4),
                         'no_last': (2, 5),
                         'slots_full': (1, 1),
                         'stride': (0, 1),
                         'smallest': (0, 0)},
               'N_full': 574,
               'beyond': {'full': (('path', 2), ('path', 288)),
                          'slots_full': (('reg', 4, 6, 0), ('nws', 18, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S48R9': ([{'graphs': [('path', 2), ('reg', 4, 12, 0), ('path', 16),
                          ('path', 19), ('path', 23), ('path', 25),
                          ('path', 27), ('path', 32)],
               'edges': {'full': (4, 5),
                         'one_row': (3, 6),
                         'no_last': (2, 7),
                         'slots_full': (1, 7),
                         'stride': (1, 3),
                         'smallest': (0, 0)},
               'N_full': 575,
               'beyond': {'full': (('path', 23), ('path', 26)),
                          'slots_full': (('reg', 4, 5, 0), ('nws', 34, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W1S64R16': ([{'graphs': [('path', 2), ('path', 8), ('ring', 8), ('path', 31),
                           ('path', 33), ('path', 120)],
                'edges': {'full': (3, 4),
                          'one_row': (3, 3),
                          'no_last': (1, 5),
                          'slots_full': (2, 5),
                          'stride': (1, 3),
                          'smallest': (0, 0)},
                'N_full': 1023,
                'beyond': {'full': (('path', 31), ('path', 34)),
                           'slots_full': (('reg', 4, 7, 0), ('nws', 34, 0))},
                'cross': {}}],
              {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W4S16R4': ([{'graphs': [('path', 2), ('path', 24), ('path', 31),
                          ('path', 32), ('path', 33)],
               'edges': {'full': (2, 4),
                         'no_last': (1, 3),
                         'slots_full': (2, 3),
                         'stride': (1, 2),
                         'smallest': (0, 0)},
               'N_full': 1023,
               'beyond': {'full': (('path', 31), ('path', 34)),
                          'slots_full': (('reg', 4, 6, 0), ('nws', 31, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W4S32R8': ([{'graphs': [('path', 2), ('path', 11), ('path', 23),
                          ('path', 28), ('path', 64), ('path', 89),
                          ('path', 163)],
               'edges': {'full': (2, 5),
                         'one_row': (1, 6),
                         'no_last': (3, 4),
                         'slots_full': (2, 5),
                         'stride': (0, 1),
                         'smallest': (0, 0)},
               'N_full': 2047,
               'beyond': {'full': (('path', 23), ('path', 90)),
                          'slots_full': (('reg', 8, 9, 0), ('nws', 25, 0))},
               'cross': {}}],
             {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W4S64R16': ([{'graphs': [('path', 2), ('reg', 8, 15, 0), ('path', 45),
                           ('path', 62)],
                'edges': {'full': (2, 3),
                          'slots_full': (1, 1),
                          'stride': (0, 1),
                          'smallest': (0, 0)},
                'N_full': 2790,
                'beyond': {'full': (('path', 45), ('path', 63)),
                           'slots_full': (('reg', 8, 14, 0), ('nws', 34, 0))},
                'cross': {}},
               {'graphs': [('path', 2), ('reg', 4, 12, 0), ('path', 23),
                           ('path', 60), ('path', 63), ('path', 64),
                           ('path', 65), ('path', 167)],
                'edges': {'full': (4, 6),
                          'one_row': (2, 7),
                          'no_last': (3, 5),
                          'slots_full': (1, 7),
                          'stride': (1, 2),
                          'smallest': (0, 0)},
                'N_full': 4095,
                'beyond': {'full': (('path', 63), ('path', 66)),
                           'slots_full': (('reg', 8, 14, 0), ('nws', 34, 0))},
                'cross': {}}],
              {'f64/2': 0, 'f64/1': 1, 'f32/2': 1, 'f32/1': 1}),
 'W16S16R2': ([{'graphs': [('path', 2), ('reg', 8, 12, 0), ('path', 23),
                           ('path', 25), ('path', 32), ('path', 41),
                           ('path', 89)],
                'edges': {'full': (2, 6),
                          'one_row': (3, 5),
                          'no_last': (4, 4),
                          'slots_full': (1, 1),
                          'stride': (1, 2),
                          'smallest': (0, 0)},
                'N_full': 2047,
                'beyond': {'full': (('path', 23), ('path', 90)),
                           'slots_full': (('reg', 8, 16, 0), ('nws', 24, 0))},
                'cross': {}}],
              {'f64/2': 0, 'f64/1': 0, 'f32/2': 0, 'f32/1': 0}),
 'W16S32R4': ([{'graphs': [('path', 2), ('reg', 8, 20, 0), ('path', 45),
                           ('path', 62)],
                'edges': {'full': (2, 3),
                          'slots_full': (1, 1),
                          'stride': (0, 2),
                          'smallest': (0, 0)},
                'N_full': 2790,
                'beyond': {'full': (('path', 45), ('path', 63)),
                           'slots_full': (('reg', 8, 19, 0), ('nws', 47, 0))},
                'cross': {}},
               {'graphs': [('path', 2), ('path', 24), ('path', 63),
                           ('reg', 4, 63, 0), ('path', 65), ('path', 128)],
                'edges': {'full': (2, 4),
                          'no_last': (1, 5),
                          'slots_full': (2, 3),
                          'stride': (1, 2),
                          'smallest': (0, 0)},
                'N_full': 4095,
                'beyond': {'full': (('path', 63), ('path', 66)),
                           'slots_full': (('reg', 8, 19, 0), ('nws', 47, 0))},
                'cross': {'one_row': (('path', 7), ('path', 439))}}],
              {'f64/2': 0, 'f64/1': 1, 'f32/2': 1, 'f32/1': 1}),
 'W16S64R8': ([{'graphs': [('path', 2), ('path', 29), ('path', 30)],
                'edges': {'full': (1, 2),
                          'stride': (0, 1),
                          'smallest': (0, 0)},
                'N_full': 870,
                'beyond': {'full': (('path', 29), ('path', 31))},
                'cross': {'slots_full': (('path', 2), ('spoke', 65, 0))}},
               {'graphs': [('path', 2), ('spoke', 65, 0), ('path', 72),
                           ('path', 76)],
                'edges': {'full': (2, 3),
                          'slots_full': (0, 1),
                          'stride': (0, 1),
                          'smallest': (0, 0)},
                'N_full': 5472,
                'beyond': {'full': (('path', 72), ('path', 77)),
                           'slots_full': (('reg', 4, 5, 0), ('spoke', 65, 0))},
                'cross': {}},
               {'graphs': [('path', 2), ('path', 63), ('spoke', 65, 0),
                           ('path', 90)],
                'edges': {'full': (1, 3),
                          'slots_full': (0, 2),
                          'stride': (0, 1),
                          'smallest': (0, 0)},
                'N_full': 5670,
                'beyond': {'full': (('path', 63), ('path', 91)),
                           'slots_full': (('reg', 4, 5, 0), ('spoke', 65, 0))},
                'cross': {}},
               {'graphs': [('path', 2), ('path', 64), ('spoke', 65, 0),
                           ('path', 67), ('path', 90), ('path', 91),
                           ('path', 107), ('path', 112)],
                'edges': {'full': (4, 5),
                          'one_row': (3, 6),
                          'no_last': (1, 7),
                          'slots_full': (0, 2),
                          'stride': (0, 2),
                          'smallest': (0, 0)},
                'N_full': 8190,
                'beyond': {'full': (('path', 90), ('path', 92)),
                           'slots_full': (('reg', 4, 5, 0), ('spoke', 65, 0))},
                'cross': {}}],
              {'f64/2': 0, 'f64/1': 1, 'f32/2': 2, 'f32/1': 3}),
 'W16S128R16': ([{'graphs': [('path', 2), ('path', 3), ('path', 40),
                             ('path', 42)],
                  'edges': {'full': (2, 3),
                            'stride': (0, 1),
                            'smallest': (0, 0)},
                  'N_full': 1680,
                  'beyond': {'full': (('path', 40), ('path', 43))},
                  'cross': {'slots_full': (('path', 2), ('spoke', 129, 0))}},
                 {'graphs': [('path', 2), ('path', 42), ('path', 43)],
                  'edges': {'full': (1, 2),
                            'stride': (1, 2),
                            'smallest': (0, 0)},
                  'N_full': 1806,
                  'beyond': {'full': (('path', 42), ('path', 44))},
                  'cross': {'slots_full': (('path', 2), ('spoke', 129, 0))}},
                 {'graphs': [('path', 2), ('reg', 8, 44, 0), ('path', 104),
                             ('path', 105)],
                  'edges': {'full': (3, 3),
                            'slots_full': (1, 1),
                            'stride': (2, 3),
                            'smallest': (0, 0)},
                  'N_full': 11025,
                  'beyond': {'slots_full': (('ring', 4), ('spoke', 129, 0)),
                             'full': (('path', 105), ('path', 107))},
                  'cross': {}}],
                {'f64/2': None, 'f64/1': 0, 'f32/2': 1, 'f32/1': 2})}

#: entries no pair can reach, by (variant, real, C): the rule that excludes them
#: (tests/test_menu_edges.py checks it).  lds: `lds_bytes` of a workgroup of the
#: variant exceeds LDS_LIMIT before any pair is in it
UNREACHABLE = {('W16S128R16', 'f64', 2): 'lds'}

#: edges of `edges_of(v)` no fixture sits on.  one_row, no_last: the variant
#: takes none of `factor_pairs`, the sparsest pairs of every factorisation of
#: that row count (tests/test_menu_edges.py evaluates it); other edges: no
#: pair of the searched pool sits on them while the variant takes it
NOT_REACHED = {('L16x4x4x1', 'f32', 1): ('one_row',),
 ('L16x4x4x1', 'f32', 2): ('one_row',),
 ('L16x4x4x1', 'f64', 1): ('one_row',),
 ('L16x4x4x1', 'f64', 2): ('one_row',),
 ('L16x4x4x1x1', 'f32', 1): ('one_row',),
 ('L16x4x4x1x1', 'f32', 2): ('one_row',),
 ('L16x4x4x1x1', 'f64', 1): ('one_row',),
 ('L16x4x4x1x1', 'f64', 2): ('one_row',),
 ('L16x4x4x3x1', 'f32', 1): ('one_row',),
 ('L16x4x4x3x1', 'f32', 2): ('one_row',),
 ('L16x4x4x3x1', 'f64', 1): ('one_row',),
 ('L16x4x4x3x1', 'f64', 2): ('one_row',),
 ('L16x4x4x4x3x1x1x1', 'f32', 1): ('one_row',),
 ('L16x4x4x4x3x1x1x1', 'f32', 2): ('one_row',),
 ('L16x4x4x4x3x1x1x1', 'f64', 1): ('one_row',),
 ('L16x4x4x4x3x1x1x1', 'f64', 2): ('one_row',),
 ('W16S128R16', 'f32', 1): ('no_last', 'one_row'),
 ('W16S128R16', 'f32', 2): ('no_last', 'one_row'),
 ('W16S128R16', 'f64', 1): ('no_last', 'one_row'),
 ('W16S32R4', 'f64', 2): ('no_last', 'one_row'),
 ('W16S64R8', 'f32', 2): ('no_last', 'one_row'),
 ('W16S64R8', 'f64', 1): ('no_last', 'one_row'),
 ('W16S64R8', 'f64', 2): ('no_last', 'one_row'),
 ('W1S16R4', 'f32', 1): ('one_row',),
 ('W1S16R4', 'f32', 2): ('one_row',),
 ('W1S16R4', 'f64', 1): ('one_row',),
 ('W1S16R4', 'f64', 2): ('one_row',),
 ('W1S20R5', 'f32', 1): ('one_row',),
 ('W1S20R5', 'f32', 2): ('one_row',),
 ('W1S20R5', 'f64', 1): ('one_row',),
 ('W1S20R5', 'f64', 2): ('one_row',),
 ('W4S16R4', 'f32', 1): ('one_row',),
 ('W4S16R4', 'f32', 2): ('one_row',),
 ('W4S16R4', 'f64', 1): ('one_row',),
 ('W4S16R4', 'f64', 2): ('one_row',),
 ('W4S64R16', 'f64', 2): ('no_last', 'one_row'),
 ('oc0_W4S0R2', 'f32', 1): ('one_row',),
 ('oc0_W4S0R2', 'f32', 2): ('one_row',),
 ('oc0_W4S0R2', 'f64', 1): ('one_row',),
 ('oc0_W4S0R2', 'f64', 2): ('one_row',),
 ('oc4_W1S20R4', 'f32', 1): ('one_row',),
 ('oc4_W1S20R4', 'f32', 2): ('one_row',),
 ('oc4_W1S20R4', 'f64', 1): ('one_row',),
 ('oc4_W1S20R4', 'f64', 2): ('one_row',),
 ('oc4_W1S24R4', 'f32', 1): ('one_row',),
 ('oc4_W1S24R4', 'f32', 2): ('one_row',),
 ('oc4_W1S24R4', 'f64', 1): ('one_row',),
 ('oc4_W1S24R4', 'f64', 2): ('one_row',),
 ('oc4_W1S28R5', 'f32', 1): ('one_row',),
 ('oc4_W1S28R5', 'f32', 2): ('one_row',),
 ('oc4_W1S28R5', 'f64', 1): ('one_row',),
 ('oc4_W1S28R5', 'f64', 2): ('one_row',),
 ('oc8_W16S48R3', 'f64', 2): ('one_row',),
 ('oc8_W16S64R3', 'f64', 1): ('one_row',),
 ('oc8_W16S64R3', 'f64', 2): ('one_row',),
 ('oc8_W1S48R5', 'f32', 1): ('one_row',),
 ('oc8_W1S48R5', 'f32', 2): ('one_row',),
 ('oc8_W1S48R5', 'f64', 1): ('one_row',),
 ('oc8_W1S48R5', 'f64', 2): ('one_row',),
 ('oc8_W4S40R2', 'f32', 1): ('one_row',),
 ('oc8_W4S40R2', 'f32', 2): ('one_row',),
 ('oc8_W4S40R2', 'f64', 1): ('one_row',),
 ('oc8_W4S40R2', 'f64', 2): ('one_row',),
 ('oc8_W4S48R4', 'f32', 1): ('one_row',),
 ('oc8_W4S48R4', 'f32', 2): ('one_row',),
 ('oc8_W4S48R4', 'f64', 1): ('one_row',),
 ('oc8_W4S48R4', 'f64', 2): ('one_row',)}
#: slots above S of the `beyond` pair of a full slot walk where no pair of the
#: pool walks exactly S + 1 (the walk is a sum of degree products)
SLOT_STEP = {'oc4_W1S28R5': 2, 'oc8_W16S32R2': 3, 'oc8_W1S32R3': 3, 'oc8_W4S32R3': 3}


class Edges(dict):
    """`expected_edges` of a fixture: name -> (i, j), a job of the symmetric
    call on the set.  With it travel `cross`: name -> (graph a, graph b), the
    edges taken as a call k([a], [b]) of their own (their recipes in
    `cross_recipes`); `beyond`: name -> (recipe, recipe), the next pair up,
    not the variant's; `N_full`, the rows of the `full` pair; and `recipes`,
    those of the set."""
    cross, cross_recipes, beyond, N_full, recipes = {}, {}, {}, 0, ()


def fixtures():
    """(variant, real, C, graphs, expected_edges) over the menu; the graph
    sets are built once per distinct set."""
    for v, rname, C, body in bodies():
        edges = Edges((k_, tuple(p)) for k_, p in body['edges'].items())
        edges.recipes = tuple(map(tuple, body['graphs']))
        edges.cross_recipes = {k_: (tuple(a), tuple(c)) for k_, (a, c)
                               in body.get('cross', {}).items()}
        edges.cross = {k_: tuple(_graphs_cached(p))
                       for k_, p in edges.cross_recipes.items()}
        edges.beyond = {k_: (tuple(a), tuple(c))
                        for k_, (a, c) in body['beyond'].items()}
        edges.N_full = body['N_full']
        yield (v, REALS[rname], C, _graphs_cached(edges.recipes), edges)


def bodies():
    """(variant, 'f32' | 'f64', C, fixture body) over the menu."""
    for rname, real in REALS.items():
        for C in (1, 2):
            for v in menu(real, C):
                sets, where = FOUND.get(variant_id(v), ((), {}))
                hit = where.get(f'{rname}/{C}')
                if hit is not None:
                    yield v, rname, C, sets[hit]


def nodal_representatives():
    """The entries whose nodal output the GPU tests check: every static
    layout, every on-the-fly variant, the largest R of every (W, D) of the
    dynamic menu and of every W of the two-stage menu."""
    out, best = [], {}
    for v in menu(np.float32, 1):
        what = kind_of(v)
        if what in ('static', 'fly'):
            out.append(v)
        else:
            key = (what, v.W, getattr(v, 'D', None))
            if key not in best or (v.R, v.S) > (best[key].R, best[key].S):
                best[key] = v
    return out + list(best.values())


def calls(v, rname):
    """(label, graphs, C, traits keywords) of the calls the GPU test of
    (v, real) makes."""
    by_c = {C: body for v_, r_, C, body in bodies()
            if v_ == v and r_ == rname}
    for C, body in sorted(by_c.items()):
        graphs = _graphs_cached(tuple(map(tuple, body['graphs'])))
        yield ('value' if C == 1 else 'gradient', graphs, C,
               dict(symmetric=True, eval_gradient=C == 2))
        if C == 1 and v in nodal_representatives():
            yield 'nodal', graphs, 1, dict(symmetric=True, nodal=True)
        if C == 1 and 'stride' in body['edges']:
            # the two roles of the even x odd pair, k(X, Y) and k(Y, X)
            i, j = body['edges']['stride']
            yield 'roles_xy', [graphs[i], graphs[j]], 1, {}
            yield 'roles_yx', [graphs[j], graphs[i]], 1, {}
        for name, pair in sorted(body.get('cross', {}).items()):
            yield (f'cross_{name}_C{C}', _graphs_cached(tuple(map(tuple, pair))),
                   C, dict(eval_gradient=C == 2))


def sources():
    """(label, hipcc flags, translation unit) of every code object the GPU
    tests of the fixtures load, in the shape of `compile_matrix.sources`."""
    done = set()
    for v, rname, C, body in bodies():
        if (v, rname) in done:
            continue
        done.add((v, rname))
        b = one_variant_backend(v, REALS[rname])
        k = kernel_on(b, REALS[rname])
        for label, graphs, C_, kw in calls(v, rname):
            traits = k.traits(**kw)
            jobs = triu_jobs(len(graphs)) if traits.symmetric \
                else cross_jobs([(0, 1)])
            host = host_plan(b, k, graphs, jobs, traits)
            srcs = b._sources(host.part[1], k.node_kernel, host.edge_kernel,
                              k.p, host.dgraphs, host.shape)
            for key, src in srcs.items():
                yield (f'menu_edges/{rname}/{label}/{variant_id(v)}/{key}',
                       tuple(b.hipcc_extra), src)


if __name__ == '__main__':
    import os
    import pprint
    import sys
    _here = os.path.dirname(os.path.abspath(__file__))
    for _p in (_here, os.path.dirname(_here)):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    if '--search' in sys.argv:
        result = search(log=lambda s: print(s, file=sys.stderr, flush=True),
                        only=set(sys.argv[2:]) or None)
        print('FOUND = ' + pprint.pformat(result, width=79, compact=True,
                                          sort_dicts=False))
        # the two tables that follow from it
        by_id = {variant_id(v): v for r in REALS.values() for C in (1, 2)
                 for v in menu(r, C)}
        unreachable, not_reached = {}, {}
        for vid, (sets, where) in result.items():
            for key, hit in where.items():
                rname, C = key.split('/')
                if hit is None:
                    unreachable[(vid, rname, int(C))] = 'lds'
                    continue
                miss = set(edges_of(by_id[vid])) - claimed(sets[hit])
                if miss:
                    not_reached[(vid, rname, int(C))] = tuple(sorted(miss))
        slot_step = {}
        for vid, (sets, where) in result.items():
            for body in sets:
                if 'slots_full' in body['beyond']:
                    v = by_id[vid]
                    b = one_variant_backend(v, np.float32)
                    m2 = pair_metrics(
                        b, kernel_on(b, np.float32),
                        make_graphs(body['beyond']['slots_full']), v, [0], [1])
                    if m2['slots'][0] != v.S + 1:
                        slot_step[vid] = int(m2['slots'][0]) - v.S
        print('SLOT_STEP = ' + pprint.pformat(slot_step, width=79))
        print('UNREACHABLE = ' + pprint.pformat(unreachable, width=79))
        print('NOT_REACHED = ' + pprint.pformat(not_reached, width=79,
                                                compact=True))
