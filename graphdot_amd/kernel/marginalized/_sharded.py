"""Pair-sharded Gram matrix over the GPUs of one node.

New capability (the reference has no multi-GPU code):
every graph pair is independent (reference job loop: template.cu:57-70), so the
job list is dealt to the ranks in cost order, every rank solves its shard into
a *packed* per-job slab (the output shape of the reference's
``alt_graph_kernel_solver``, experimental/alterantive_mgk/template.cu:71,103-118)
and one all-gather of equal-sized slabs reassembles the matrix.  There is no
other data-path collective.

The class is transport- and device-agnostic: ``solve_local(job_ids)`` computes
the shard (the HIP plan on a GPU, the oracle in the CPU tests) and
``all_gather(local)`` is ``torch.distributed.all_gather_into_tensor`` over RCCL
(backend "nccl") on GPUs or gloo on CPU.
"""
import json
import os
import numpy as np


def predict_cost(n_node, n_nz, ji, jj):
    """Relative cost of a pair: product-graph nonzeros plus vector work."""
    return n_nz[ji] * n_nz[jj] + 4 * n_node[ji] * n_node[jj]


# --------------------------------------------------------------------------
# measured cost model: time per pair by solver variant
# --------------------------------------------------------------------------
_COST_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                'cost_table.json')
_cost_table = None


def cost_table(path=None, reload=False):
    """{'f64/C1/oc4_W1_S25_R4_L16x4x4x1': [a_ns, b_ns], ..., 'tail_us': t}:
    the time a pair adds to a launch of its solver variant on MI355X,
    ``a + b (nnz1 nnz2 + 4 n1 n2)`` nanoseconds (throughput time: chip-wide
    launch duration / pairs), fitted by scripts/calibrate_cost.py from timed
    slices of the launches of the QM7-like benchmark set.  The time per pair
    steps with the solver variant (registers -> waves per SIMD), which is why
    one arithmetic-only weight for all pairs misses by up to 57 %
    (scripts/fit_cost_model.py)."""
    global _cost_table
    if path is not None:
        with open(path) as f:
            return json.load(f)
    if _cost_table is None or reload:
        try:
            with open(os.environ.get('GD_COST_TABLE', _COST_TABLE_PATH)) as f:
                _cost_table = json.load(f)
        except OSError:
            _cost_table = {}
    return _cost_table


def variant_key(v):
    """Name of a solver variant in the cost table."""
    if getattr(v, 'L', None):
        return f'oc{v.D}_W{v.W}_S{v.S}_R{v.R}_L' + 'x'.join(map(str, v.L))
    if hasattr(v, 'D'):
        return f'oc{v.D}_W{v.W}_S{v.S}_R{v.R}'
    return f'W{v.W}_S{v.S}_R{v.R}'


def job_times(variants, choice, arith, real, C, table=None):
    """Predicted nanoseconds per job: the table entry of its variant, or --
    for a variant that was never calibrated -- the arithmetic model scaled to
    the mean of the calibrated ones."""
    table = cost_table() if table is None else table
    f = 'f64' if np.dtype(real) == np.float64 else 'f32'
    arith = np.asarray(arith, dtype=np.float64)
    t = np.zeros(len(arith))
    known = [v for k, v in table.items()
             if k.startswith(f'{f}/C{C}/') and isinstance(v, list)]
    # fallback slope: ns per unit of arithmetic, mean over calibrated variants
    ref = table.get(f'{f}/C{C}/mean_ns_per_arith')
    if ref is None:
        ref = float(np.mean([b for _, b in known])) if known else 1.0
        if ref <= 0:
            ref = 1.0
    for k in np.unique(choice):
        sel = choice == k
        ab = table.get(f'{f}/C{C}/{variant_key(variants[k])}')
        if ab is None:
            t[sel] = ref * arith[sel] * (1.0 + 0.02 * getattr(
                variants[k], 'S', 0))
        else:
            t[sel] = ab[0] + ab[1] * arith[sel]
    return t


def partition_blocks(times, group, world_size, tail=0.0, snap=0,
                     group_tail=None):
    """Cut a job list that is already in launch order (by solver variant
    `group`, then descending cost) into `world_size` contiguous blocks whose
    predicted times -- the jobs' times plus `tail` per variant a block touches
    (every launch ends in a tail during which the chip drains) -- have the
    smallest possible maximum.  A rank then holds 1-3 variants, i.e. 1-3 large
    launches, instead of a sliver of every variant.  Cuts within `snap` jobs of
    a variant boundary move onto it (no launch of a few hundred pairs).
    `group_tail`: {variant: tail} overrides `tail` per variant (a launch of a
    large-pair variant drains for longer).  Returns the list of index ranges
    (start, stop)."""
    n = len(times)
    if n == 0:
        return [(0, 0)] * world_size
    c = np.concatenate(([0.0], np.cumsum(times, dtype=np.float64)))
    gstart = np.flatnonzero(np.concatenate(([True], group[1:] != group[:-1])))
    bounds = np.concatenate((gstart, [n]))
    # tails of the variants up to (and including) the one at each start
    gt = np.array([(group_tail or {}).get(int(group[g]), tail)
                   for g in gstart], dtype=np.float64)
    ct = np.concatenate(([0.0], np.cumsum(gt)))

    def fill(T):
        """greedy: longest prefix of predicted time <= T per rank"""
        cuts, a = [], 0
        for _ in range(world_size):
            if a >= n:
                cuts.append((a, a))
                continue
            lo, hi = a + 1, n
            # time of [a, e) = c[e] - c[a] + tail * (variants touched)
            def cost(e):
                # variants touched by [a, e): those whose segment holds a
                # ... e - 1
                v0 = np.searchsorted(gstart, a, side='right') - 1
                v1 = np.searchsorted(gstart, e - 1, side='right') - 1
                return c[e] - c[a] + ct[v1 + 1] - ct[v0]
            if cost(lo) > T:
                return None
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if cost(mid) <= T:
                    lo = mid
                else:
                    hi = mid - 1
            cuts.append((a, lo))
            a = lo
        return cuts if a >= n else None

    lo_T, hi_T = c[-1] / world_size, c[-1] + ct[-1]
    for _ in range(60):
        mid = 0.5 * (lo_T + hi_T)
        if fill(mid) is None:
            lo_T = mid
        else:
            hi_T = mid
    cuts = fill(hi_T)
    if snap > 0:
        out, a = [], 0
        for r, (_, e) in enumerate(cuts):
            if r < world_size - 1 and a < e < n:
                k = int(np.argmin(np.abs(bounds - e)))
                if abs(int(bounds[k]) - e) <= snap and bounds[k] > a:
                    e = int(bounds[k])
            e = max(e, a)
            out.append((a, e if r < world_size - 1 else n))
            a = out[-1][1]
        cuts = out
    return cuts


def partition(cost, world_size, mode=None):
    """Deal jobs to ranks.  Returns a list of job-id arrays, one per rank,
    each sorted by descending cost.

    'snake' (default): descending-cost snake order (LPT-like) -- every rank
    gets the same mix of pairs, balanced whatever the cost model is worth.
    'blocks': contiguous runs of the cost-sorted list with equal total cost --
    a rank gets pairs of similar size, i.e. of one or two solver variants
    (fewer, larger launches per rank), and is as well balanced as the cost
    model is accurate."""
    mode = mode or 'snake'
    order = np.argsort(-cost, kind='stable')
    if mode == 'blocks':
        c = np.cumsum(cost[order], dtype=np.float64)
        total = c[-1] if len(c) else 0.0
        cuts = np.searchsorted(c, total * np.arange(1, world_size) / world_size)
        return np.split(order, cuts)
    k = np.arange(len(order))
    rnd, pos = k // world_size, k % world_size
    rank = np.where(rnd % 2 == 0, pos, world_size - 1 - pos)
    return [order[rank == r] for r in range(world_size)]


class ShardPlan:
    """Static description of one rank's share and of the reassembly."""

    def __init__(self, ji, jj, n_node, n_nz, nX, nY, symmetric, rank,
                 world_size, launch_order=None, times=None, group=None,
                 tail=0.0, snap=2048, mode=None, group_tail=None,
                 merge_map=None, quotient=None):
        """`launch_order`, `times`, `group` (optional): the job ids in the
        backend's launch order (by solver variant, then descending cost), the
        predicted time of every job (`job_times`) and its solver variant --
        the shards are then contiguous blocks of that order with equal
        predicted time (`partition_blocks`); without them jobs are dealt in
        snake order by the arithmetic cost."""
        self.rank, self.world_size = rank, world_size
        self.ji, self.jj = np.asarray(ji), np.asarray(jj)
        self.nX, self.nY, self.symmetric = nX, nY, symmetric
        #: launch merging decided on the WHOLE job list ({variant index:
        #: variant index it rides in}): every rank applies it to its shard,
        #: so which solver a pair runs on does not depend on the rank count
        self.merge_map = merge_map
        #: the launch merging of the call on its twin-leaf quotient images
        #:, decided on the whole job list like `merge_map`, or
        #: None: the call keeps the full images
        self.quotient = quotient
        cost = predict_cost(np.asarray(n_node), np.asarray(n_nz),
                            self.ji, self.jj)
        self.mode = 'snake'
        if launch_order is not None and mode in (None, 'measured'):
            lo = np.asarray(launch_order, dtype=np.int64)
            self._model = dict(launch_order=lo, times=np.asarray(
                times, dtype=np.float64), group=np.asarray(group), tail=tail,
                snap=snap, group_tail=group_tail, n_node=n_node, n_nz=n_nz)
            cuts = partition_blocks(self._model['times'][lo],
                                    self._model['group'][lo], world_size,
                                    tail, snap, group_tail)
            self.shards = [lo[a:b] for a, b in cuts]
            # predicted nanoseconds per rank: pairs + launch tails
            self.predicted = []
            for s in self.shards:
                tails = sum((group_tail or {}).get(int(v), tail)
                            for v in np.unique(self._model['group'][s]))
                self.predicted.append(
                    float(self._model['times'][s].sum()) + tails)
            self.mode = 'measured'
        else:
            self.shards = partition(cost, world_size, mode)
        self.capacity = max(len(s) for s in self.shards) if len(cost) else 0
        self.local = self.shards[rank]
        # position of every job in the gathered [world_size, capacity] slab
        self.slot = np.empty(len(cost), dtype=np.int64)
        for r, s in enumerate(self.shards):
            self.slot[s] = r * self.capacity + np.arange(len(s))

    def rebalanced(self, measured):
        """A new plan after the ranks have timed their shards: `measured[r]`
        (any unit) is what rank r's solver launches took.  The predicted time
        of every job of shard r is scaled by measured[r] / predicted[r]
        (normalised so that the total stays), the cuts are taken again.  What
        the cost table misses on a particular set of graphs -- it was fitted
        on the QM7-like benchmark set -- is corrected from the only
        measurement that matters; two rounds bring the ranks within a few
        percent of each other (scripts/shard_sim.py).  Every rank computes the
        same new plan from the same all-gathered numbers."""
        if self.mode != 'measured':
            return self
        m = np.asarray(measured, dtype=np.float64)
        p = np.asarray(self.predicted, dtype=np.float64)
        ok = (m > 0) & (p > 0)
        if not ok.all() or len(m) != self.world_size:
            return self
        f = (m / p) / np.mean(m / p)
        md = self._model
        times = md['times'].copy()
        for r, s in enumerate(self.shards):
            times[s] *= f[r]
        return ShardPlan(self.ji, self.jj, md['n_node'], md['n_nz'], self.nX,
                         self.nY, self.symmetric, self.rank, self.world_size,
                         launch_order=md['launch_order'], times=times,
                         group=md['group'], tail=md['tail'], snap=md['snap'],
                         group_tail=md['group_tail'],
                         merge_map=self.merge_map, quotient=self.quotient)

    def scatter_index(self, starts_x, starts_y):
        """Flat F-order destinations (and mirrored destinations) of the
        gathered slab entries -- K(I1, I2) = gathered[slot]
        (tensor_view column-major: graphdot/cpp/tensor_view.h:22-33)."""
        a = starts_x[self.ji].astype(np.int64)
        b = starts_y[self.jj].astype(np.int64)
        dst = a + self.nX * b
        if self.symmetric:
            off = self.ji != self.jj
            mdst = b[off] + self.nX * a[off]
            return dst, self.slot, mdst, self.slot[off]
        return dst, self.slot, None, None

    def reassembly_index(self, n_grad=0):
        """(src, dst) flat indices that turn the all-gathered slabs into the
        column-major result on the device with one gather + one scatter
        (``out[dst] = gathered[src]``).  Every rank's slab is laid out as
        ``[capacity values | capacity * n_grad gradient entries, job-major]``
        (what the packed solver writes: mgk_solver.h, F_PACKED); the result is
        ``[nX * nY values | n_grad planes of nX * nY]`` with the mirrored
        entries of a symmetric matrix filled in."""
        n_cols = 1 + n_grad
        sx = np.arange(self.nX + 1, dtype=np.int64)
        jy = self.jj if self.symmetric else self.jj - self.nX
        saved, self.jj = self.jj, jy
        try:
            dst, slot, mdst, mslot = self.scatter_index(sx, sx if self.symmetric
                                                        else np.arange(self.nY + 1))
        finally:
            self.jj = saved
        if mdst is not None:
            dst = np.concatenate((dst, mdst))
            slot = np.concatenate((slot, mslot))
        cap = self.capacity
        rank, pos = slot // cap, slot % cap
        base = rank * cap * n_cols
        srcs, dsts = [base + pos], [dst]
        for c in range(n_grad):
            srcs.append(base + cap + pos * n_grad + c)
            dsts.append((c + 1) * self.nX * self.nY + dst)
        return np.concatenate(srcs), np.concatenate(dsts)

    def assemble(self, gathered, n_cols=1):
        """Host reassembly of the gathered slabs into the (nX, nY[, n_cols])
        matrix (graph-level outputs: starts are 0..n)."""
        sx = np.arange(self.nX + 1)
        sy = np.arange(self.nY + 1) if not self.symmetric else sx
        jy = self.jj if self.symmetric else self.jj - self.nX
        saved = self.jj
        self.jj = jy
        dst, src, mdst, msrc = self.scatter_index(sx, sy)
        self.jj = saved
        g = np.asarray(gathered).reshape(self.world_size * self.capacity,
                                         n_cols)
        out = np.zeros((self.nX * self.nY, n_cols), dtype=g.dtype)
        out[dst] = g[src]
        if mdst is not None:
            out[mdst] = g[msrc]
        out = out.reshape(self.nY, self.nX, n_cols).transpose(1, 0, 2)
        return out[:, :, 0] if n_cols == 1 else out


def measured_shard_plan(backend, graphs, node_kernel, edge_kernel, jobs, nX,
                        nY, traits, rank, world):
    """The ShardPlan of a job list on `backend`: the whole list is laid out
    as one rank would launch it (solver variant per job, launch order:
    HIPBackend._partition), every job gets the measured time of its variant
    (`cost_table`), and the ranks take contiguous blocks of that order with
    equal predicted time.  Host only and deterministic: every rank computes
    the same plan."""
    jobs = np.ascontiguousarray(jobs)
    # the host plans `prepare` itself chooses from (host only: no upload);
    # the last is that of the full images.  The first is that of the
    # twin-leaf quotient images where a plain HIPBackend takes them for the
    # WHOLE list: decided here, with their launch merging, and
    # applied by every rank.  (Cuts and predicted times stay those of the
    # full images: the cost table knows their variants, and the ranks
    # re-balance by measurement.)
    plans = list(backend._host_plans(graphs, node_kernel, edge_kernel, jobs,
                                     traits))
    quotient = dict(plans[0].part.merge_map) if plans[0].shape.quot else None
    dgraphs, C, part = plans[-1].dgraphs, plans[-1].shape.C, plans[-1].part
    order_all, launches, merge_map = part[2], part[3], dict(part.merge_map)
    ji, jj = jobs['i'].astype(np.int64), jobs['j'].astype(np.int64)
    n_node = np.array([g.n_node for g in dgraphs], np.int64)
    n_nz = np.array([g.n_nz for g in dgraphs], np.int64)
    group = np.zeros(len(jobs), dtype=np.int64)
    for L in launches:
        group[order_all[L['offset']:L['offset'] + L['count']]] = L['k']
    table = cost_table()
    times = job_times(backend.variants, group, predict_cost(
        n_node, n_nz, ji, jj), backend.real, C, table)
    f = 'f64' if np.dtype(backend.real) == np.float64 else 'f32'
    tail = 1e3 * float(table.get(f'{f}/C{C}/tail_us',
                                 table.get('tail_us', 12.0)))
    group_tail = {}
    for L in launches:
        t_ = table.get(f'{f}/C{C}/{variant_key(L["variant"])}/tail_us')
        if t_ is not None:
            group_tail[int(L['k'])] = 1e3 * float(t_)
    return ShardPlan(ji, jj, n_node, n_nz, int(nX), int(nY),
                     bool(traits.symmetric), rank, world,
                     launch_order=order_all.astype(np.int64), times=times,
                     group=group, tail=tail, group_tail=group_tail,
                     merge_map=merge_map, quotient=quotient)


def balance_by_measurement(step, plan, build, rounds=2, group=None):
    """Re-balance a sharded step from the ranks' own timings: every rank
    times its solver launches, the times are all-gathered (one number per
    rank) and the cuts are taken again (`ShardPlan.rebalanced`); `build(plan)`
    makes the step of a plan.  Returns (step, plan)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    for _ in range(max(0, rounds)):
        if plan.mode != 'measured':
            break
        t = torch.tensor([step.time_local()], dtype=torch.float64)
        if cuda_collective(group):
            t = t.to(step.device)
        ts = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(ts, t, group=group)
        plan = plan.rebalanced([float(x.item()) for x in ts])
        step = build(plan)
    return step, plan


def cuda_collective(group=None):
    """Does the process group run its collectives on device memory through
    RCCL?  Decided from the group's backend map (``cpu:gloo,cuda:nccl`` for a
    composite group), not from string equality with "nccl"."""
    import torch.distributed as dist
    try:
        cfg = str(dist.get_backend_config(group))
    except Exception:                                  # older torch
        cfg = str(dist.get_backend(group))
    if ':' not in cfg:
        return cfg == 'nccl'
    parts = dict(item.split(':', 1) for item in cfg.split(',') if ':' in item)
    return parts.get('cuda') == 'nccl'


_communicators = {}


def _abi_communicator(group, runtime):
    """The RCCL communicator of this process for `group`, created through the
    C ABI (one per group, cached): rank 0 makes the unique id, the process
    group broadcasts it."""
    import torch.distributed as dist
    key = id(group) if group is not None else None
    if key not in _communicators:
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [runtime.Communicator.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0)
                                   if group is not None else 0, group=group)
        _communicators[key] = runtime.Communicator(world, box[0], rank)
    return _communicators[key]


class ShardedStep:
    """One rank's device-resident evaluation of a pair-sharded Gram matrix
    (+ gradient planes): the single code path of ``bench.py --gpus N`` and of
    ``distributed_backend()``.

    * the solver kernels write this rank's packed slab
      ``[capacity values | capacity * n_grad gradient entries]`` straight into
      the tensor the collective reads (``HIPBackend.prepare(gramian_ptr=)``);
    * one ``all_gather_into_tensor`` of equal-capacity slabs (RCCL over xGMI
      when the group's CUDA backend is nccl; staged through host memory for a
      gloo group -- CPU-only development boxes and tests);
    * one gather + scatter on the device (``ShardPlan.reassembly_index``)
      turns the gathered slabs into the column-major ``(nX, nY[, 1 + n_grad])``
      result, mirrored entries included.

    `enqueue()` issues all of that without a host synchronisation: every
    solver stream waits (device-side event) for the null stream's position at
    the start of the step, the null stream -- on which torch runs the
    collective and the reassembly -- waits for every solver stream.  The result stays on the device
    (`values` / `gradient` tensors); `download()` copies it out once.
    """

    def __init__(self, backend, graphs, node_kernel, edge_kernel, p, q, eps,
                 ftol, gtol, jobs, starts, nX, nY, nJ, traits, group=None,
                 timer=None, shard_plan=None, collective='torch',
                 pipeline=False, gather_gradient=True):
        """`gather_gradient=False` (value + gradient steps): only the VALUES
        are all-gathered and reassembled; the gradient entries of this rank's
        pairs stay in its slab (`local_gradient`, rows in the order of
        `local_index`) for a consumer that reduces over pairs -- the Gaussian
        process contracts them with K^-1 - a a^T and all-reduces n_theta
        numbers instead of moving n_theta planes (gpr.py:287-298)."""
        import torch
        import torch.distributed as dist
        from ...hip import runtime
        self.backend, self.group = backend, group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.on_device = cuda_collective(group)
        # collective='rccl': the all-gather goes through the C ABI
        # (gd_all_gather, include/gdhip.h) on a communicator of its own; the
        # process group only carries the 128-byte unique id to the ranks
        self.comm = None
        if collective == 'rccl':
            self.comm = _abi_communicator(group, runtime)
            self.on_device = True
        elif collective != 'torch':
            raise ValueError(f'collective={collective!r}: "torch" or "rccl"')
        device = runtime.ensure_device(backend.device)
        # the tensors live on the device the *backend* runs on, whatever
        # torch's current device is
        self.device = torch.device('cuda', device)
        self.nX, self.nY = int(nX), int(nY)
        self.n_grad = int(nJ) if traits.eval_gradient is True else 0
        n_cols = self.n_cols = 1 + self.n_grad
        self.gather_gradient = bool(gather_gradient) or self.n_grad == 0
        # columns that travel: the collective and the reassembly see the
        # first `g_cols` * capacity entries of a slab
        g_cols = self.g_cols = n_cols if self.gather_gradient else 1
        jobs = np.ascontiguousarray(jobs)
        if shard_plan is None:
            shard_plan = measured_shard_plan(
                backend, graphs, node_kernel, edge_kernel, jobs, self.nX,
                self.nY, traits, self.rank, self.world)
        self.shard = sp = shard_plan
        cap = self.capacity = sp.capacity
        rs = np.dtype(backend.real)
        self.tdtype = torch.float32 if rs == np.float32 else torch.float64
        # pipeline: two slab / gather buffers and a front stream, so that the
        # solvers of step i + 1 run while the collective and the reassembly of
        # step i are still on the null stream (they only wait for the buffer
        # pair they write, i.e. for the reassembly of step i - 1)
        self.depth = 2 if pipeline else 1
        self.front = runtime.Stream() if pipeline else None
        self.buffer_free = [runtime.Event() for _ in range(self.depth)]
        self._count = 0
        with torch.cuda.device(self.device):
            self.local_outs = [torch.zeros(max(cap * n_cols, 1),
                                           dtype=self.tdtype,
                                           device=self.device)
                               for _ in range(self.depth)]
            self.gathereds = [torch.empty(self.world * max(cap * g_cols, 1),
                                          dtype=self.tdtype,
                                          device=self.device)
                              for _ in range(self.depth)]
            self.local_out, self.gathered = self.local_outs[0], \
                self.gathereds[0]
            self.result = torch.zeros(g_cols * self.nX * self.nY,
                                      dtype=self.tdtype, device=self.device)
            src, dst = sp.reassembly_index(self.n_grad if self.gather_gradient
                                           else 0)
            self.t_src = torch.from_numpy(src).to(self.device)
            self.t_dst = torch.from_numpy(dst).to(self.device)
            # every element of the result has a source (the usual case: the
            # jobs cover the matrix): the reassembly is one gather kernel
            self.t_perm = None
            perm = np.full(self.result.numel(), -1, dtype=np.int64)
            perm[dst] = src
            if len(perm) and perm.min() >= 0:
                self.t_perm = torch.from_numpy(perm).to(self.device)
            torch.cuda.synchronize(self.device)
        local_jobs = jobs[sp.local]
        local_jobs.flags.writeable = False         # recognised by identity
        self.local_jobs = local_jobs
        self._args = (graphs, jobs, starts, nX, nY, nJ, traits)
        from ._backend_hip import LaunchSet
        self.launch_set = LaunchSet()
        self.bind(node_kernel, edge_kernel, p, q, eps, ftol, gtol, timer)

    def bind(self, node_kernel, edge_kernel, p, q, eps, ftol, gtol,
             timer=None):
        """(Re)build the launch plan for the given hyperparameters: same
        graphs, jobs, buffers and streams, new kernel arguments -- what a
        repeated evaluation in a training loop costs."""
        from ...hip import runtime
        graphs, _, starts, nX, nY, nJ, traits = self._args
        rs = np.dtype(self.backend.real)
        self.plans = [self.backend.prepare(
            graphs, node_kernel, edge_kernel, p, q, eps, ftol, gtol,
            self.local_jobs, starts, nX, nY, nJ, traits, timer, packed=True,
            gramian_ptr=out.data_ptr(),
            gradient_ptr=out.data_ptr() + self.capacity * rs.itemsize,
            merge_map=self.shard.merge_map,
            quotient=getattr(self.shard, 'quotient', None))
            for out in self.local_outs]
        self.plan = self.plans[0]

    def enqueue(self, events=None, serial=False, phases=None):
        """One step: solver launches, all-gather, reassembly -- all
        asynchronous (`LaunchSet` orders the solver streams against the null
        stream, on which torch runs the collective and the reassembly).
        `events[k] = (start, stop)` are recorded around launch k on the
        stream it runs on (bench.py's per-kernel timing).  `phases`: four
        events recorded on the null stream -- step start, solvers done,
        all-gather done, reassembly done (`phase_ms`)."""
        import torch
        import torch.distributed as dist
        b = self._count % self.depth
        self._count += 1
        local_out, gathered = self.local_outs[b], self.gathereds[b]
        self.local_out, self.gathered = local_out, gathered   # (the latest)
        if phases is not None:
            phases[0].record()
        self.launch_set.enqueue(self.plans[b], events, serial,
                                front=self.front,
                                after=(self.buffer_free[b],))
        if phases is not None:
            phases[1].record()        # (the null stream waits for the solvers)
        if not self.gather_gradient:
            local_out = local_out[:max(self.capacity, 1)]     # values only
        with torch.cuda.device(self.device):
            if self.comm is not None:
                # null stream: behind the solvers (LaunchSet) and in front of
                # the reassembly torch enqueues there
                self.comm.all_gather(
                    local_out.data_ptr(), gathered.data_ptr(),
                    local_out.numel(), self.backend.real)
            elif self.on_device:
                dist.all_gather_into_tensor(gathered, local_out,
                                            group=self.group)
            else:
                h = local_out.cpu()                # waits for the solvers
                g = torch.empty(self.world * h.numel(), dtype=h.dtype)
                dist.all_gather_into_tensor(g, h, group=self.group)
                gathered.copy_(g)
            if phases is not None:
                phases[2].record()
            if self.t_perm is not None:
                torch.index_select(gathered, 0, self.t_perm, out=self.result)
            else:
                self.result.index_copy_(
                    0, self.t_dst, gathered.index_select(0, self.t_src))
        if phases is not None:
            phases[3].record()
        self.buffer_free[b].record()       # (null stream: slabs are consumed)

    def enqueue_solvers(self):
        """The solver launches of this rank's shard alone, DETACHED: no
        collective, no reassembly, and the null stream does not wait for them
        -- work enqueued there next runs beside the solvers.  `join()` orders
        the null stream behind them; the slab (`local_gradient`) is complete
        after it."""
        b = self._count % self.depth
        self._count += 1
        self.local_out, self.gathered = self.local_outs[b], self.gathereds[b]
        self.launch_set.enqueue(self.plans[b], front=self.front,
                                after=(self.buffer_free[b],), detached=True)

    def join(self):
        self.launch_set.join()

    def phase_ms(self, steps=5):
        """Device time of the three phases of a step on this rank, averaged
        over `steps` steps: {'shard_ms': this rank's solver launches,
        'all_gather_ms': the collective (for a gloo group: the copies through
        host memory included), 'reassembly_ms': slabs -> matrix}.  What makes
        a multi-GPU run diagnosable: the slowest shard, the collective and the
        reassembly add up to the step."""
        from ...hip import runtime
        ev = [[runtime.Event() for _ in range(4)] for _ in range(steps)]
        self.enqueue()
        self.synchronize()
        for k in range(steps):
            self.enqueue(phases=ev[k])
            self.synchronize()      # (phases of different steps do not overlap)
        out = {}
        for name, a in (('shard_ms', 0), ('all_gather_ms', 1),
                        ('reassembly_ms', 2)):
            out[name] = float(np.mean([e[a].elapsed_ms(e[a + 1]) for e in ev]))
        return out

    @property
    def local_index(self):
        """(i, j) of this rank's pairs, in the order of its slab."""
        return (self.local_jobs['i'].astype(np.int64),
                self.local_jobs['j'].astype(np.int64))

    @property
    def local_gradient(self):
        """(pairs of this rank, n_grad) device view of the gradient entries
        in this rank's slab (row p: pair `local_index[p]`)."""
        n, cap = len(self.local_jobs), self.capacity
        return self.local_out[cap:cap + n * self.n_grad].view(n, self.n_grad)

    def synchronize(self):
        import torch
        from ...hip import runtime
        runtime.synchronize()
        torch.cuda.synchronize(self.device)

    def time_local(self, steps=5):
        """Milliseconds of this rank's solver launches alone (no collective,
        no reassembly): what `ShardPlan.rebalanced` balances."""
        import time
        from ...hip import runtime
        for _ in range(2):
            self.launch_set.enqueue(self.plans[0])
        runtime.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.launch_set.enqueue(self.plans[0])
        runtime.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    @property
    def values(self):
        """(nX, nY) column-major device tensor view of the matrix."""
        return self.result[:self.nX * self.nY].view(self.nY, self.nX).t()

    @property
    def gradient(self):
        """(nX, nY, n_grad) device view of the gradient planes."""
        if not self.gather_gradient:
            raise RuntimeError('this step keeps the gradient in the ranks\' '
                               'slabs (gather_gradient=False): local_gradient')
        n = self.nX * self.nY
        return self.result[n:].view(self.n_grad, self.nY, self.nX).permute(
            2, 1, 0)

    def download(self, gramian=None, gradient=None):
        """Copy the reassembled result to the host (one D2H), into the
        caller's flat column-major arrays when given."""
        self.synchronize()
        host = self.result.cpu().numpy()
        n = self.nX * self.nY
        if gramian is not None:
            gramian[:] = host[:n].reshape(np.shape(gramian))
        if gradient is not None and self.n_grad:
            gradient[:] = host[n:].reshape(np.shape(gradient))
        return host[:n], host[n:]


def distributed_backend(**kwargs):
    """A HIPBackend that shards every graph-level evaluation over the ranks
    of the initialised ``torch.distributed`` process group (one process per
    GPU, launched e.g. by ``python -m torch.distributed.run``):

        kernel = MarginalizedGraphKernel(knode, kedge, q=q,
                                         backend=distributed_backend())
        K = kernel(graphs)          # every rank gets the full matrix

    Pairs are independent, so each rank solves its cost-balanced share of the
    job list into a packed slab (`ShardPlan`) that is already the input of the
    all-gather (RCCL for a group whose CUDA backend is nccl, host memory for
    gloo), the gathered slabs are scattered into the matrix on the device and
    downloaded once into the caller's arrays (`ShardedStep`, the code path of
    ``bench.py --gpus N``).  Nodal and diagonal evaluations, and runs without
    a process group, take the single-GPU path.  ``shard_single_rank=True``
    routes a one-rank group through the sharded path too (tests).
    ``collective='rccl'`` runs the all-gather through the C ABI
    (``gd_all_gather``) instead of ``torch.distributed``.  Other keyword
    arguments as for HIPBackend."""
    from ._backend_hip import HIPBackend

    class DistributedHIPBackend(HIPBackend):

        def __init__(self, shard_single_rank=False, collective='torch',
                     pipeline=False, rebalance=2, **kw):
            # Which solver variant a pair runs on must not depend on the
            # shard it falls into: the variants are different instantiations
            # (compiled with fast-math) and agree to round-off only.  Launch
            # merging is therefore decided once, on the whole job list
            # (`ShardPlan.merge_map`), and applied by every rank: the results
            # are bit-identical for any number of ranks, and to a plain
            # HIPBackend on one GPU.
            super().__init__(**kw)
            self.shard_single_rank = shard_single_rank
            self.collective = collective
            self.pipeline = pipeline
            #: rounds of measured re-balancing when a sharded step is first
            #: built (every rank times its shard, the times are all-gathered,
            #: the cuts are taken again: ShardPlan.rebalanced)
            self.rebalance = int(rebalance)
            #: job lists shorter than this per rank are not re-balanced
            self.rebalance_min_jobs = 4096
            #: consumers that factor the kernel matrix (model.gaussian_process)
            #: may overlap the factorisation with the gradient solves: values
            #: first (their own sharded step), then the value + gradient
            #: solvers detached beside the dense algebra.  OFF by default
            #: (None): measured on one GPU with the shards of a world of
            #: eight (scripts/gpr_step_sim.py), the overlapped step takes
            #: 2.44 ms against 1.63 ms one after the other with round 6's
            #: one-launch factorisation (profiles/r06_gpr_step_sim_f64.log;
            #: round 5, with its chain of ~50 launches: 2.96 against 2.51) --
            #: the value step is paid on top, and a factorisation that is one
            #: latency-bound chain gains nothing from compute units it shares
            #: with the solver grids.  `overlap_min_ranks = n` turns it on for
            #: a measurement on real ranks.
            self.overlap_min_ranks = None
            self._shard_plans = {}
            self._steps = {}      # (shard plan, nJ, traits) -> ShardedStep
            # (clones of a kernel -- clone_with_theta, every objective
            # evaluation of the regressor -- hold shallow copies of the
            # backend: what the copies must see of each other lives here)
            self._shared = {}

        @property
        def last_step(self):
            """The `ShardedStep` of the latest sharded evaluation on this
            backend or any of its copies."""
            return self._shared.get('last_step')

        @last_step.setter
        def last_step(self, step):
            self._shared['last_step'] = step

        def overlaps_dense_algebra(self):
            import torch.distributed as dist
            return (self.overlap_min_ranks is not None
                    and self.shards_over_ranks()
                    and dist.get_world_size() >= self.overlap_min_ranks)

        def shards_over_ranks(self):
            """True when a process group with more than one rank is up."""
            import torch.distributed as dist
            return (dist.is_available() and dist.is_initialized()
                    and (dist.get_world_size() > 1 or self.shard_single_rank))

        def _shard_plan(self, graphs, dgraphs, node_kernel, edge_kernel,
                        jobs, nX, nY, traits, rank, world):
            # (C: value and value + gradient launches have different
            # variants and times per pair, hence different plans)
            key = (tuple(map(id, dgraphs)), id(jobs) if not
                   jobs.flags.writeable else hash(jobs.tobytes()),
                   nX, nY, bool(traits.symmetric), rank, world,
                   self._call_shape(None, traits,
                                    1 + (traits.eval_gradient is True),
                                    edge_kernel))
            hit = self._shard_plans.get(key)
            if hit is None:
                if len(self._shard_plans) > 8:
                    self._shard_plans.clear()
                sp = measured_shard_plan(self, graphs, node_kernel,
                                         edge_kernel, jobs, nX, nY, traits,
                                         rank, world)
                hit = self._shard_plans[key] = (sp, jobs, list(dgraphs))
            return key, hit

        def sharded_step(self, graphs, node_kernel, edge_kernel, p, q, eps,
                         ftol, gtol, jobs, starts, nX, nY, nJ, traits,
                         timer=None, gather_gradient=True, solvers_only=False):
            """Evaluate the graph-level job list over the ranks and leave the
            reassembled result on this rank's device: returns the
            `ShardedStep` (`.values` / `.gradient` / `.result`), enqueued and
            synchronised.  Steps are cached per (graphs, jobs, traits): a
            repeated evaluation with new hyperparameters only re-binds the
            kernel arguments.  `gather_gradient=False`: the gradient stays
            in the ranks' slabs (`ShardedStep.local_gradient`).
            `solvers_only`: the step is enqueued DETACHED and without its
            collective (`ShardedStep.enqueue_solvers`) and not synchronised:
            the caller goes on enqueueing on the null stream and calls
            `step.join()` before it reads `local_gradient`."""
            import torch.distributed as dist
            rank, world = dist.get_rank(), dist.get_world_size()
            jobs = np.ascontiguousarray(jobs) if not isinstance(
                jobs, np.ndarray) else jobs
            if not isinstance(graphs, (list, tuple)):
                graphs = list(graphs)
            dgraphs = [self._register_graph(g) for g in graphs]
            plan_key, (sp, _, kept) = self._shard_plan(
                graphs, dgraphs, node_kernel, edge_kernel, jobs, int(nX),
                int(nY), traits, rank, world)
            gather_gradient = bool(gather_gradient)
            key = (id(sp), int(nJ), traits, gather_gradient)
            step = self._steps.get(key)
            if step is None:
                if len(self._steps) > 4:
                    self._steps.clear()

                def build(plan):
                    return ShardedStep(
                        self, graphs, node_kernel, edge_kernel, p, q, eps,
                        ftol, gtol, jobs, starts, nX, nY, nJ, traits,
                        timer=timer, shard_plan=plan,
                        collective=self.collective, pipeline=self.pipeline,
                        gather_gradient=gather_gradient)
                step = build(sp)
                if (world > 1 and self.rebalance > 0
                        and len(jobs) >= self.rebalance_min_jobs * world):
                    step, sp = balance_by_measurement(step, sp, build,
                                                      self.rebalance)
                    # later calls find the tuned plan -- under the key of
                    # THIS evaluation only: the job list of an n x n matrix
                    # is one cached object shared by every set of n graphs
                    # and by value and value + gradient evaluations
                    self._shard_plans[plan_key] = (sp, jobs, kept)
                    key = (id(sp), int(nJ), traits, gather_gradient)
                self._steps[key] = step
            else:
                step.bind(node_kernel, edge_kernel, p, q, eps, ftol, gtol,
                          timer)
            if solvers_only:
                step.enqueue_solvers()
                self.last_step = step
                return step
            if timer is not None:
                timer.tic('GPU kernel execution')
            step.enqueue()
            step.synchronize()
            if timer is not None:
                timer.toc('GPU kernel execution')
            self.last_step = step
            return step

        def __call__(self, graphs, node_kernel, edge_kernel, p, q, eps, ftol,
                     gtol, jobs, starts, gramian, gradient, nX, nY, nJ,
                     traits, timer):
            graph_level = (traits.nodal is False and not traits.diagonal)
            if not (self.shards_over_ranks() and graph_level):
                return super().__call__(
                    graphs, node_kernel, edge_kernel, p, q, eps, ftol, gtol,
                    jobs, starts, gramian, gradient, nX, nY, nJ, traits,
                    timer)
            step = self.sharded_step(
                graphs, node_kernel, edge_kernel, p, q, eps, ftol, gtol, jobs,
                starts, nX, nY, nJ, traits, timer)
            step.download(gramian,
                          gradient if traits.eval_gradient is True else None)

    return DistributedHIPBackend(**kwargs)
