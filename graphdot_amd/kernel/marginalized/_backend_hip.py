"""HIP backend of the marginalized graph kernel for MI355X (gfx950).

Serves the reference's backend seam (``Backend.__call__``,
``graphdot/kernel/marginalized/_backend_cuda.py:247-368``): graph images are
packed and cached per graph, node/edge microkernels are printed as HIP C++
functors and JIT-compiled with hipcc, hyperparameters are handed to the
kernel as by-value arguments, and the job list is partitioned over a small
menu of register-resident solver variants (see ``csrc/device/mgk_solver.h``).

There is no CPU path: a missing ``libgdhip.so`` / hipcc / device raises.
"""
import copy
import os
import re
import uuid
import zlib
from collections import OrderedDict, namedtuple
import numpy as np
from ...codegen import Template
from ...util import gcpause
from ...util.cookie import IdentityCache
from ...codegen.sympy_printer import to_real_expr
from ...codegen.typetool import _dtype_util
from ...hip import jit, runtime
from ...microkernel import TensorProduct, Product
from ...util.iterable import flatten, fold_like
from ._backend import Backend
from ._devicegraph import (DeviceGraph, GraphArena, HIST_BINS, class_bytes,
                           term_bytes,
                           degree_histograms, graph_features, pack_many,
                           quotient_graph)
# the solver menu; every name of it that lived here
# stays importable from here
from ._menu import (  # noqa: F401
    SolverMenu, Variant, OCVariant, OCStatic, VARIANTS, OC_QUOTIENT_LAYOUTS,
    OC_STATIC_VARIANTS, OC_FLY_VARIANTS, OC_VARIANTS, FLY_MIN_DEGREE,
    GENERAL, TABLES, MFMA, STREAM, _LARGE_PAIR_SOLVERS, GENERAL_THREADS,
    MFMA_MAX_NODES, STREAM_THREADS, STREAM_ROWS, STREAM_CAP,
    STREAM_MAX_PARTS, STREAM_LDS_BUDGET, LDS_LIMIT, WPB1, TABLE_LDS_LIMIT,
    GLOBAL_TABLE_LIMIT, STREAM_PART_EFFICIENCY, stream_parts, ClassPairs,
    Partition, CallShape, NotOwnerComputes, quotient_images)

_TEMPLATE = os.path.join(os.path.dirname(__file__), 'template.hip')

# solver flags, mirror graphdot::mgk::F_* (mgk_solver.h)
F_NODAL, F_DIAGONAL, F_SYMMETRIC, F_LMIN1, F_BLOCK, F_PACKED, F_REFCOMPAT, \
    F_DENSE = 1, 2, 4, 8, 16, 32, 64, 128

#: bytes allocated behind the last blob of an arena on the device: the
#: one-wave quotient solvers stage an image with unguarded 16-byte loads, two
#: per lane and trip (mgk_oc.h QSET); the host arena and its bytes stay as
#: they are
ARENA_SLACK = 2 * 64 * 16


def _real_name(real):
    return {np.dtype(np.float32): 'float', np.dtype(np.float64): 'double'}[
        np.dtype(real)]


# --------------------------------------------------------------------------
# struct printing and packing
# --------------------------------------------------------------------------
def declstruct(dtype, name):
    """C++ definition ``struct name {...};`` of an aligned numpy struct dtype.
    Unlike ``decltype`` every nested struct is *named* (``name_field``) so
    that zero-size members can be declared ``constexpr static`` (not allowed
    inside unnamed structs in standard C++)."""
    dtype = np.dtype(dtype)
    members = []
    for key in dtype.names or ():
        ft = dtype.fields[key][0]
        if key.startswith('$'):
            n, tpl, *args = key[1:].split('::')
            targs = ','.join(np.dtype(a).name for a in args)
            members.append(f'{tpl}<{targs}> {n};')
        elif _dtype_util.is_object(ft):
            if ft.itemsize == 0:
                members.append(f'constexpr static _empty {key} {{}};')
            else:
                sub = f'{name}_{key}'
                members.append(declstruct(ft, sub)[:-1] + f' {key};')
        elif _dtype_util.is_array(ft):
            dims = ''.join(f'[{d}]' for d in ft.shape)
            members.append(f'{ft.base.name} {key}{dims};')
        else:
            members.append(f'{ft.name} {key};')
    return f'struct {name} {{' + ' '.join(members) + '};'


def packable(dtype):
    """Can two records of this struct dtype ride in one record of pairs
    (`declstruct2`)?  Every leaf a 4-byte number, no arrays, no
    variable-length attributes, no padding."""
    dtype = np.dtype(dtype)
    if dtype.names is None:
        return False

    def leaves(t):
        n = 0
        for key in t.names:
            ft = t.fields[key][0]
            if key.startswith('$') or _dtype_util.is_array(ft):
                return -1
            if _dtype_util.is_object(ft):
                if ft.itemsize == 0:
                    continue
                sub = leaves(ft)
                if sub < 0:
                    return -1
                n += sub
            elif ft.kind in 'fiu' and ft.itemsize == 4:
                n += 1
            else:
                return -1
        return n
    n = leaves(dtype)
    return n > 0 and 4 * n == dtype.itemsize


def declstruct2(dtype, name):
    """`declstruct` with every 4-byte leaf a pair, ``graphdot::pk2<T>``: two
    records side by side, leaf by leaf (device/fmath.h; mgk_oc.h evaluates the
    edge microkernel of the dense product on two terms at once)."""
    dtype = np.dtype(dtype)
    members = []
    for key in dtype.names:
        ft = dtype.fields[key][0]
        if _dtype_util.is_object(ft):
            if ft.itemsize == 0:
                members.append(f'constexpr static _empty {key} {{}};')
            else:
                members.append(declstruct2(ft, f'{name}_{key}')[:-1]
                               + f' {key};')
        else:
            members.append(f'graphdot::pk2<{ft.name}> {key};')
    return f'struct {name} {{' + ' '.join(members) + '};'


#: calls a packed evaluation can make (overloaded for pairs in device/fmath.h)
_PACKED_CALLS = re.compile(
    r'graphdot::(?:exp|ipow<\d+>|ripow<\d+>)$')


def packed_expression(expr):
    """Does the generated expression only call what device/fmath.h overloads
    for pairs?"""
    calls = re.findall(r'([A-Za-z_][\w:]*(?:<[^<>()]*>)?)\s*\(', expr)
    return all(_PACKED_CALLS.match(c) for c in calls)


def widen_theta(dtype, real):
    """theta structs hold float32 hyperparameters in the reference; an fp64
    build stores them as float64."""
    dtype = np.dtype(dtype)
    if np.dtype(real) == np.float32:
        return dtype
    if dtype.names is not None:
        return np.dtype([(k, widen_theta(dtype.fields[k][0], real))
                         for k in dtype.names], align=True)
    if dtype.subdtype is not None:
        return np.dtype((widen_theta(dtype.base, real), dtype.shape))
    return np.dtype(real) if dtype == np.float32 else dtype


def raw_state(obj):
    """Like ``obj.state`` but without the float32 rounding of cpptype, so an
    fp64 build sees the hyperparameters at full precision."""
    values = getattr(obj, '_theta_values', None)
    if values is not None:
        return tuple(values.values())
    out = []
    dt = obj.dtype
    for key in dt.names or ():
        ft = dt.fields[key][0]
        v = getattr(obj, key)
        out.append(raw_state(v) if _dtype_util.is_object(ft) else v)
    return tuple(out)


def fill_struct(view, dtype, state):
    """Write nested tuple `state` into the 0-d structured array `view`."""
    for key, value in zip(dtype.names or (), state):
        ft = dtype.fields[key][0]
        if _dtype_util.is_object(ft):
            if ft.itemsize:
                fill_struct(view[key], ft, value)
        else:
            view[key] = value


def pack_theta(obj, real):
    dt = widen_theta(obj.dtype, real)
    buf = np.zeros((), dtype=dt) if dt.itemsize else None
    if buf is not None:
        fill_struct(buf, dt, raw_state(obj) if np.dtype(real) != np.float32
                    else obj.state)
    return dt, buf


# --------------------------------------------------------------------------
# backend
# --------------------------------------------------------------------------
#: one record of `HIPBackend._host_plans`: images a call may run on and what
#: the host decides for them; `layout` holds it all (`HIPBackend._layout`)
HostPlan = namedtuple('HostPlan',
                      'dgraphs edge_kernel fields shape arena part layout')


class Plan:
    """Everything resident on the device for one kernel evaluation."""


class Layout:
    """The hyperparameter-independent part of a Plan (HIPBackend._layout)."""


#: code objects loaded in this process, by JIT cache key (shared by backends)
_MODULES = {}
#: rendered translation units, by (code signature, variant, build options):
#: pure text work on hyperparameter-independent inputs, shared by backends
_SOURCES = {}
#: HIP streams / events are expensive to create (milliseconds each): every
#: LaunchSet draws from this process-wide pool, in order
_STREAM_POOL, _EVENT_POOL = [], []
_LOW_STREAM_POOL, _LOW_EVENT_POOL = [], []     # streams of the lowest priority


class _DeviceGraphList(list):
    """The packed graphs of one call, with the tuple of their identities
    (the key of the arena and layout caches) computed once."""
    ids = None


def _ids(dgraphs):
    return getattr(dgraphs, 'ids', None) or tuple(map(id, dgraphs))


class LaunchSet:
    """The streams and events that run the launches of a plan, step after
    step, without a host synchronisation: the launches every solver depends
    on (the table kernel) go to the null stream, every solver variant to a
    non-blocking stream of its own (longest first), ordered device-side --
    the solver streams wait for the `start` event of the step (recorded on
    the null stream behind the table kernel and behind everything the caller
    enqueued there before, e.g. the previous step's collective), the null
    stream waits for every solver stream.  `events[k] = (begin, end)` are
    recorded around solver launch k on the stream it runs on."""

    def __init__(self):
        self.streams, self.done = [], []
        # detached launches (`enqueue(detached=True)`) run on streams of the
        # lowest priority: what overlaps them on the null stream -- a chain of
        # small dependent launches, the Cholesky factorisation -- gets compute
        # units as soon as it has a workgroup to dispatch instead of queueing
        # behind the solver grids
        self.low_streams, self.low_done = [], []
        self._last_done = self.done
        self.start = runtime.Event()
        self._n_last = 0
        self.max_streams = int(os.environ.get('GD_MAX_STREAMS', '3'))
        self.streams_forced = 'GD_MAX_STREAMS' in os.environ

    def enqueue(self, plan, events=None, serial=False, front=None, after=(),
                detached=False):
        """`front`: a stream that takes the place of the null stream for the
        table kernel and the start event (pipelined steps: the null stream
        may still be busy with the previous step's collective).  It first
        waits for the events in `after` and for the solver launches of the
        previous `enqueue` (they read the table buffer this step rewrites).
        `detached`: the null stream does NOT wait for the solver streams --
        what the caller enqueues there next (the Gaussian process factors the
        kernel matrix while the gradient solves run) overlaps the solvers;
        `join()` makes it wait later."""
        fh = None
        if front is not None and not serial:
            fh = front.h
            for e in after:
                front.wait_event(e)
            for slot in range(self._n_last):
                front.wait_event(self._last_done[slot])
        for L in plan.pre_launches:
            runtime.launch(L['fn'], L['grid'], L['threads'], L['args'],
                           stream=fh, dynamic_lds=L['dynamic_lds'],
                           cooperative=L.get('cooperative', False))
        n = len(plan.launches)
        if serial:
            for k, L in enumerate(plan.launches):
                if events is not None:
                    events[k][0].record()
                runtime.launch(L['fn'], L['grid'], L['threads'], L['args'],
                               dynamic_lds=L['dynamic_lds'],
                           cooperative=L.get('cooperative', False))
                if events is not None:
                    events[k][1].record()
            self._n_last = 0
            return
        # longest launch first, each to the stream with the least work so far
        # (at most `max_streams` streams: the runtime multiplexes them onto a
        # few hardware queues, and every stream costs two cross-queue
        # dependencies per step)
        cost = [plan.launches[k]['count'] * (plan.launches[k]['variant'].S + 8)
                for k in range(n)]
        order = sorted(range(n), key=lambda k: -cost[k])
        ns = max(1, min(n, self.max_streams or n))
        # (a plan may ask for fewer: HIPBackend.prepare, `stream_hint`)
        hint = getattr(plan, 'stream_hint', None)
        if hint and not self.streams_forced:
            ns = max(1, min(ns, hint))
        low = detached
        streams, done, spool, epool = (
            (self.low_streams, self.low_done, _LOW_STREAM_POOL,
             _LOW_EVENT_POOL) if low else
            (self.streams, self.done, _STREAM_POOL, _EVENT_POOL))
        while len(streams) < ns:
            k = len(streams)
            if len(spool) <= k:
                spool.append(runtime.Stream(low_priority=low))
                epool.append(runtime.Event())
            streams.append(spool[k])
            done.append(epool[k])
        self.start.record(fh)
        load = [0] * ns
        for slot in range(ns):
            streams[slot].wait_event(self.start)
        for k in order:
            slot = load.index(min(load))
            load[slot] += cost[k]
            L, s = plan.launches[k], streams[slot]
            if events is not None:
                events[k][0].record(s.h)
            runtime.launch(L['fn'], L['grid'], L['threads'], L['args'],
                           stream=s.h, dynamic_lds=L['dynamic_lds'],
                           cooperative=L.get('cooperative', False))
            if events is not None:
                events[k][1].record(s.h)
        for slot in range(ns):
            done[slot].record(streams[slot].h)
            if not detached:
                runtime.null_stream_wait_event(done[slot])
        self._n_last, self._last_done = ns, done
        self._detached = ns if detached else 0

    def join(self):
        """The null stream waits for the solver launches of a detached
        `enqueue` (device-side)."""
        for slot in range(getattr(self, '_detached', 0)):
            runtime.null_stream_wait_event(self._last_done[slot])
        self._detached = 0


class HIPBackend(SolverMenu, Backend):
    """MI355X backend: the solver menu (`_menu.SolverMenu`: variants, fit
    rules, LDS and occupancy figures, the partition into launches) with the
    generated source, the device state and the three phases of a call.

    Parameters
    ----------
    device: int or None
        HIP device ordinal (default: ``$LOCAL_RANK`` or 0).
    real: numpy float32 (reference arithmetic, default) or float64
    jobs_per_unit: int
        Graph pairs handled by one wave (small pairs) or workgroup (large
        pairs) before it retires; sets the launch grid.  Default 1.
    hipcc_extra: list of str
        Extra compiler flags (also ``$GD_HIPCC_EXTRA``).
    variants: list of Variant
        Solver menu ``(W, S, R)`` in order of preference; ``GENERAL`` (the
        global-scratch solver for pairs of any size) last.
    record_iterations: bool
        Keep per-job CG iteration counts on the device (`iterations(plan)`).
    occupancy: dict (W, S) -> waves per SIMD, or None
        Overrides the measured occupancy targets (also ``$GD_OCCUPANCY``).
    concurrent: bool
        One HIP stream per solver variant (default) or all on one stream.
    tables: 'global' (default), 'lds' or False
        Microkernel values per pair of label classes from tables instead of
        per nonzero pair (see __init__).
    min_launch: int
        Owner-computes launches of fewer waves (pairs x waves per pair) are
        merged into the next larger compatible variant in use (default 8192;
        0: never).
    nodal_gradient_in_kernel: bool
        Nodal Jacobians inside the launch (default) or by re-launches.
    native: bool
        Host side of a call in C++ (libgdhost.so, default) or in numpy.
    quotient: bool
        Plain graph-level value calls solve every pair on the twin-leaf
        quotient images of its graphs (default; also ``$GD_QUOTIENT=0``: off).
    """

    @staticmethod
    def array(ndarray):
        return np.array(ndarray, copy=True)

    @staticmethod
    def zeros(size, dtype=np.float32):
        return np.zeros(size, dtype)

    @staticmethod
    def empty(size, dtype=np.float32):
        """Output buffers of the caller (reference: managed memory,
        graphdot/cuda/array.py:14-31): large ones come from a pool of pinned
        host blocks, so that `collect` copies the result by DMA straight into
        the array the user gets (hip/runtime.py::pinned_empty)."""
        return runtime.pinned_empty(size, dtype)

    def __init__(self, **kwargs):
        self.uuid = uuid.uuid4()
        self.device = kwargs.pop('device', None)
        real = kwargs.pop('real', np.float32)
        jobs_per_unit = kwargs.pop('jobs_per_unit', 1)
        self.hipcc_extra = list(kwargs.pop('hipcc_extra', [])) + \
            os.environ.get('GD_HIPCC_EXTRA', '').split()
        variants = kwargs.pop('variants', None)
        if os.environ.get('GD_VARIANTS'):  # experiments: "W:S:R[:D],L16x4x1,..."
            def parse(item):
                if item.startswith('L'):
                    return OCStatic(*map(int, item[1:].split('x')))
                f = list(map(int, item.split(':')))
                return OCVariant(*f) if len(f) == 4 else Variant(*f)
            variants = [parse(item) for item in
                        os.environ['GD_VARIANTS'].split(',')] \
                + _LARGE_PAIR_SOLVERS
        self.record_iterations = kwargs.pop('record_iterations', False)
        occupancy = kwargs.pop('occupancy', None)
        self.concurrent = kwargs.pop('concurrent', True)
        # microkernel value tables over label classes (GraphArena.classes):
        #   'global' (default): one tiny launch per evaluation fills a global
        #       table per pair of classes, the owner-computes solvers look
        #       values up (mgk_oc.h) -- whenever the labels can be numbered;
        #   'lds' (or True): the two-stage solvers rebuild the tables per
        #       workgroup in LDS (round 1; slower than direct evaluation with
        #       one pair per workgroup, kept for microkernels much more
        #       expensive than a Gaussian); the owner-computes menu is off;
        #   False: every microkernel value is evaluated where it is used.
        tables = kwargs.pop('tables', 'global')
        if tables is True:
            tables = 'lds'
        if tables not in (False, 'lds', 'global'):
            raise ValueError(f'tables={tables!r}: False, "lds" or "global"')
        self.tables = tables
        self._launch_set = None
        min_launch = kwargs.pop(
            'min_launch', os.environ.get('GD_MIN_LAUNCH', 8192))
        self.nodal_gradient_in_kernel = bool(kwargs.pop(
            'nodal_gradient_in_kernel', True))
        # host side of a call (graph packing, label classes, variant per job,
        # launch order): libgdhost.so (csrc/gdhost.cpp), or -- native=False --
        # the numpy restatements it is tested against
        native = bool(kwargs.pop('native', True))
        self.quotient = bool(kwargs.pop(
            'quotient', os.environ.get('GD_QUOTIENT', '1') != '0'))
        if native:
            from ...hip import hostlib
            hostlib.lib()                  # fail loudly if it cannot be built
            hostlib.collector()            # (optional helper: loaded here, not in the first call)
        if occupancy is None and os.environ.get('GD_OCCUPANCY'):
            # e.g. GD_OCCUPANCY="1:16:5,1:24:4"  (W:S:waves)
            occupancy = {
                (int(a), int(b)): int(c) for a, b, c in
                (item.split(':') for item in
                 os.environ['GD_OCCUPANCY'].split(','))}
        if kwargs:
            raise TypeError(f'unknown HIPBackend options {sorted(kwargs)}')
        SolverMenu.__init__(self, real=real, variants=variants,
                            occupancy=occupancy, native=native,
                            min_launch=min_launch,
                            jobs_per_unit=jobs_per_unit)
        runtime.lib()                      # fail loudly if the library is absent
        self._modules = _MODULES           # (tu key) -> runtime.Module
        self._arenas = OrderedDict()       # tuple(id(DeviceGraph)) -> (arena, buf)
        self._pool = {}                    # name -> DeviceBuffer (grow-only)
        self._dgraph_lists = IdentityCache()
        self._layouts = OrderedDict()      # job-list key -> Layout (LRU)
        self._source_cache = _SOURCES      # (code signature, variant) -> text
        self._module_sets = {}             # (code signature, variants) -> (modules, argument dtype)
        self.layout_cache_size = 8
        self._props = None
        self.last_plan = None

    def __deepcopy__(self, memo):
        # clones of a kernel (clone_with_theta) share device state, like the
        # reference backend (_backend_cuda.py:63-64)
        return copy.copy(self)

    # -- device helpers -------------------------------------------------------
    @property
    def props(self):
        if self._props is None:
            self._props = runtime.device_props(self.device)
        return self._props

    @staticmethod
    def _zeroed_buffer(nbytes):
        """A device buffer of zeros (the barrier cells of the streamed
        solver; owned by the plan that asked for it)."""
        buf = runtime.DeviceBuffer(max(int(nbytes), 256))
        buf.upload(np.zeros(buf.nbytes, dtype=np.uint8))
        runtime.synchronize()
        return buf

    def _buffer(self, name, nbytes):
        """Grow-only pool of per-call device buffers.  A buffer that is too
        small is *dropped from the pool*, never freed here: earlier plans and
        the zero-copy views handed out by `device_gram` (torch tensors alias
        them) hold references, and `DeviceBuffer.__del__` releases the
        allocation when the last of those is gone."""
        buf = self._pool.get(name)
        if buf is None or buf.nbytes < nbytes:
            buf = self._pool[name] = runtime.DeviceBuffer(
                max(int(nbytes * 1.25), 256))
        return buf

    def detach_outputs(self, plan):
        """Hand the output buffers of `plan` over to whoever holds the
        plan: the pool forgets them, so that the next evaluation on this
        backend writes into buffers of its own instead of over these
        (`MarginalizedGraphKernel.device_cross_gram` / `device_diag`)."""
        for name in ('gramian', 'gradient'):
            buf = plan.buffers.get(name)
            if buf is not None and self._pool.get(name) is buf:
                del self._pool[name]

    # -- graphs ---------------------------------------------------------------
    def _register_graph(self, graph):
        key = (self.uuid.int, np.dtype(self.real).str)   # (an int hashes in C)
        if key not in graph.cookie:
            graph.cookie[key] = DeviceGraph(graph, real=self.real)
        return graph.cookie[key]

    @staticmethod
    def _assert_homogeneous(x, y):
        if (x.weighted != y.weighted or x.node_t != y.node_t
                or x.edge_t != y.edge_t):
            raise TypeError(
                'All nodes/edges must be of the same type: '
                f'{x.node_t} / {x.edge_t} vs {y.node_t} / {y.edge_t}. '
                'If the graph attributes match in name but differ in type, '
                'try to normalize automatically with '
                '`Graph.unify_datatype`.')

    @staticmethod
    def _used_fields(kernel):
        """Attributes a microkernel reads, taken from the code it generates:
        ``x1.<name>`` / ``x2.<name>`` accesses.  () for a kernel that ignores
        its arguments (Constant), None (= every attribute) if an argument is
        used as a whole."""
        fun, jac = kernel.gen_expr('x1', 'x2')
        text = ' '.join([fun, *jac])
        names = set(re.findall(r'\bx[12]\.([A-Za-z_]\w*)', text))
        bare = re.search(r'\bx[12]\b(?!\.[A-Za-z_])', text)
        return None if bare else tuple(sorted(names))

    def _table_bytes(self, arena):
        """LDS bytes of the per-workgroup microkernel tables (tables='lds')
        of `arena`'s label classes, or 0 if this call evaluates the
        microkernels directly (other modes, labels not numberable, or tables
        beyond TABLE_LDS_LIMIT)."""
        c = arena.classes
        if self.tables != 'lds' or c is None:
            return 0
        b = (c['nv']**2 + c['ne']**2) * self.rsize
        return int(-(-b // 16) * 16) if b <= TABLE_LDS_LIMIT else 0

    def _global_tables(self, arena):
        """Do the owner-computes solvers of this call read the microkernels
        from the per-evaluation global tables (tables='global' and the labels
        fall into classes)?"""
        c = arena.classes
        return (self.tables == 'global' and c is not None
                and c['nv']**2 + c['ne']**2 <= GLOBAL_TABLE_LIMIT)

    def _host_arena(self, dgraphs, fields):
        # (label classes are only numbered when the tables are in use)
        # (and the half-term records of quotient images only for the solvers
        # that read them: mgk_oc.h RECS, double)
        return GraphArena(dgraphs, *fields, classes=bool(self.tables),
                          native=self.native,
                          terms=self.f64)

    def _arena(self, dgraphs, fields=(None, None)):
        key = (_ids(dgraphs), fields if self.tables else None)
        hit = self._arenas.get(key)
        if hit is not None:
            self._arenas.move_to_end(key)
            return hit
        arena = self._host_arena(dgraphs, fields)
        # (slack behind the last blob: the staging loads of the one-wave
        # quotient solvers carry no per-lane guard, mgk_oc.h QSET)
        buf = runtime.DeviceBuffer(arena.nbytes + ARENA_SLACK)
        buf.upload(arena.relocated(buf.ptr))
        runtime.synchronize()
        self._arenas[key] = (arena, buf, list(dgraphs))
        # evicted arenas are released when the last layout / plan that points
        # into them is gone (DeviceBuffer frees on destruction)
        while len(self._arenas) > 4:
            self._arenas.popitem(last=False)
        return self._arenas[key]

    # -- code generation --------------------------------------------------------
    @staticmethod
    def gencode_kernel(kernel, name, real=np.float32):
        """HIP C++ for a microkernel: ``struct <name>_theta_t`` (the packed
        hyperparameters) and functor ``<name>_t`` with ``operator()`` and
        ``_j_a_c_o_b_i_a_n_`` (reference: _backend_cuda.py:157-193)."""
        fun, jac = kernel.gen_expr('x1', 'x2')
        rn = _real_name(real)
        fun = to_real_expr(fun, np.dtype(real).name)
        jac = [to_real_expr(j, np.dtype(real).name) for j in jac]
        return Template(r'''
${theta_t}
struct ${name}_t : ${name}_theta_t {
    constexpr static int jac_dims = ${jac_dims};
    template<class X> __device__ __forceinline__
    auto operator() (X const &x1, X const &x2) const {
        return ${expr};
    }
    template<class X> __device__ __forceinline__
    auto _j_a_c_o_b_i_a_n_(X const &x1, X const &x2) const {
        graphdot::array<real_t, jac_dims> j;
        ${jac;}
        return j;
    }
};
''').render(
            name=name, jac_dims=len(jac), expr=fun,
            theta_t=declstruct(widen_theta(kernel.dtype, real),
                               f'{name}_theta_t'),
            jac=[f'j[{i}] = {e};' for i, e in enumerate(jac)] + [''],
        ).replace('real_t', 'real_t') + f'// real = {rn}\n'

    @staticmethod
    def gencode_probability(pfunc, name, real=np.float32):
        """Functor for the starting probability on a node ``n``
        (reference: _backend_cuda.py:195-228)."""
        fun, jac = pfunc.gen_expr()
        fun = to_real_expr(fun, np.dtype(real).name)
        jac = [to_real_expr(j, np.dtype(real).name) for j in jac]
        return Template(r'''
${theta_t}
struct ${name}_t : ${name}_theta_t {
    constexpr static int jac_dims = ${jac_dims};
    template<class N> __device__ __forceinline__
    auto operator() (N const &n) const {
        return ${expr};
    }
    template<class N> __device__ __forceinline__
    auto _j_a_c_o_b_i_a_n_(N const &n) const {
        graphdot::array<real_t, jac_dims> j;
        ${jac;}
        return j;
    }
};
''').render(
            name=name, jac_dims=len(jac), expr=fun,
            theta_t=declstruct(widen_theta(pfunc.dtype, real),
                               f'{name}_theta_t'),
            jac=[f'j[{i}] = {e};' for i, e in enumerate(jac)] + [''],
        )

    @staticmethod
    def pack_state(obj, diff_grid=False, diff_eps=1e-2):
        """[state] or, with diff_grid, [state, state(theta_0 e^+eps),
        state(theta_0 e^-eps), ...] (reference: _backend_cuda.py:230-245)."""
        pack = [obj.state]
        if diff_grid is True:
            logtheta = np.log(list(flatten(obj.theta)))
            for i in range(len(logtheta)):
                for delta in (diff_eps, -diff_eps):
                    o = copy.deepcopy(obj)
                    t = logtheta.copy()
                    t[i] += delta
                    o.theta = fold_like(np.exp(t), o.theta)
                    pack.append(o.state)
        return pack

    def _theta_dtype(self, obj):
        dt = widen_theta(obj.dtype, self.real)
        return dt if dt.itemsize else np.dtype(np.uint8)

    def _params_dtype(self, node_kernel, edge_kernel, p):
        P, theta = np.uintp, self._theta_dtype
        return np.dtype([
            ('arena', P), ('jobs', P), ('order', P), ('starts', P),
            ('gramian', P), ('gradient', P), ('iters', P), ('scratch', P),
            ('sync', P), ('tables', P), ('diag', P), ('diag_grad', P), ('hotspot', P),
            ('node_starts', P), ('diag_ld', np.uint32),
            ('n_launch_jobs', np.uint32), ('nX', np.uint32),
            ('nY', np.uint32), ('nJ', np.uint32), ('flags', np.uint32),
            ('order_offset', np.uint32), ('u_capacity', np.uint32),
            ('g_capacity', np.uint32), ('parts', np.uint32),
            ('n_vclass', np.uint32), ('n_eclass', np.uint32),
            ('vrep', np.uint32), ('erep', np.uint32),
            ('q', self.real), ('q0', self.real), ('eps', self.real),
            ('ftol', self.real), ('gtol', self.real),
            ('node_kernel', theta(node_kernel)),
            ('edge_kernel', theta(edge_kernel)),
            ('p_start', theta(p)),
        ], align=True)

    def _params_fd_dtype(self, node_kernel, edge_kernel, p):
        """Kernel arguments of the nodal finite-difference gradient solver:
        graphdot::mgk::params_fd_t (mgk_oc.h)."""
        theta = self._theta_dtype
        nv = len(node_kernel.gen_expr('x1', 'x2')[1])
        ne = len(edge_kernel.gen_expr('x1', 'x2')[1])
        return np.dtype([
            ('base', self._params_dtype(node_kernel, edge_kernel, p)),
            ('q_plus', self.real), ('q_minus', self.real),
            ('node_theta', self.real, (max(nv, 1),)),
            ('edge_theta', self.real, (max(ne, 1),)),
            ('node_diff', theta(node_kernel), (max(2 * nv, 1),)),
            ('edge_diff', theta(edge_kernel), (max(2 * ne, 1),)),
        ], align=True)

    def kernel_name(self, v, C, nodal=False, tab=False, ngrad=False,
                    maximin=False, quot=False):
        """Entry point name: arithmetic, solver variant, flavour."""
        f = 'f64' if self.f64 else 'f32'
        if v == GENERAL:
            return f'mgk_{f}_general_T{GENERAL_THREADS}_C{C}'
        if v == TABLES:
            return f'mgk_{f}_tables_C{C}'
        if v == MFMA:
            return f'mgk_{f}_mfma_C{C}'
        if v == STREAM:
            return f'mgk_{f}_stream_T{STREAM_THREADS}_C{C}'
        if isinstance(v, OCVariant):
            return f'mgk_{f}_oc{v.D}_W{v.W}_S{v.S}_R{v.R}_C{C}' + \
                ('_L' + 'x'.join(map(str, v.L)) if v.L else '') + \
                ('_nodal' if nodal else '') + ('_tab' if tab else '') + \
                ('_ngrad' if ngrad else '') + (
                    '_m3' if maximin == 2 else '_maximin' if maximin else '') \
                + ('_quot' if quot else '')
        return f'mgk_{f}_W{v.W}_S{v.S}_R{v.R}_C{C}' + \
            ('_nodal' if nodal else '') + ('_tab' if tab else '')

    def _entry_point(self, v, C, nodal=False, tab=False, ngrad=False,
                     maximin=False, quot=False):
        if v == TABLES:
            return Template(r'''
extern "C" __global__ __launch_bounds__(256)
void ${name}(params_t prm) {
    graphdot::mgk::fill_tables<real_t, ${C}>(prm);
}
''').render(name=self.kernel_name(v, C), C=C)
        if isinstance(v, OCVariant):
            return Template(r'''
extern "C" __global__ __launch_bounds__(${threads})
__attribute__((amdgpu_waves_per_eu(${waves})))
void ${name}(${params} prm) {
    using solver = graphdot::mgk::oc_solver<real_t, ${S}, ${R}, ${W}, ${C},
        ${nodal}, ${D}, ${tab}, ${ngrad}, ${maximin}, ${layout}, graph_t,
        node_kernel_t, edge_kernel_t, p_start_t${quot}>;
    static_assert(solver::DLDS == ${dlds}, "Jacobi diagonals in LDS: the host sized the [Y] region for the other answer (HIPBackend.diagonals_in_lds)");
    __shared__ typename solver::lds_t lds;
    extern __shared__ __attribute__((aligned(16))) char dyn_lds[];
    solver::run(prm, lds, reinterpret_cast<real_t *>(dyn_lds));
}
''').render(threads=64 * v.W,
            name=self.kernel_name(v, C, nodal, tab, ngrad, maximin, quot),
            quot=', true' if quot else '',
            dlds='true' if self.diagonals_in_lds(v, C, nodal or ngrad
                                                 or bool(maximin)) else 'false',
            maximin='2' if maximin == 2 else 'true' if maximin else 'false',
            layout=('graphdot::mgk::seg_layout<%s>' % ', '.join(map(str, v.L))
                    if v.L else 'graphdot::mgk::dynamic_layout'),
            S=v.S, R=v.R, W=v.W, C=C, D=v.D if v.S else 1,
            waves=self._oc_waves(v, C, ngrad) if ngrad
            else self._waves_without_lds_diagonals(v, C, nodal or bool(maximin)),
            nodal='true' if nodal else 'false',
            tab='true' if tab else 'false',
            ngrad='true' if ngrad else 'false',
            params='params_fd_t' if ngrad else 'params_t')
        if v == GENERAL:
            return Template(r'''
extern "C" __global__ __launch_bounds__(${threads})
void ${name}(params_t prm) {
    using solver = graphdot::mgk::general_solver<real_t, ${threads}, ${C},
        graph_t, node_kernel_t, edge_kernel_t, p_start_t>;
    __shared__ typename solver::lds_t lds;
    solver::run(prm, lds, prm.scratch);
}
''').render(threads=GENERAL_THREADS, name=self.kernel_name(v, C), C=C)
        if v == MFMA:
            return Template(r'''
extern "C" __global__ __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(3)))
void ${name}(params_t prm) {
    using solver = graphdot::mgk::mfma_solver<real_t, graph_t, node_kernel_t,
        edge_kernel_t, p_start_t>;
    __shared__ typename solver::lds_t lds;
    extern __shared__ __attribute__((aligned(16))) char dyn_lds[];
    solver::run(prm, lds, dyn_lds);
}
''').render(name=self.kernel_name(v, C))
        if v == STREAM:
            return Template(r'''
extern "C" __global__ __launch_bounds__(${threads})
void ${name}(params_t prm) {
    using solver = graphdot::mgk::stream_solver<real_t, ${threads}, ${C},
        graph_t, node_kernel_t, edge_kernel_t, p_start_t>;
    static_assert(solver::A_ROWS == ${rows} && solver::SEG_CAP == ${cap} && solver::LDS_BUDGET == ${budget}, "rows of p staged per pass, neighbours per segment, LDS budget: host and device disagree");
    __shared__ typename solver::lds_t lds;
    extern __shared__ __attribute__((aligned(16))) char dyn_lds[];
    solver::run(prm, lds, dyn_lds, prm.scratch);
}
''').render(threads=STREAM_THREADS, name=self.kernel_name(v, C), C=C,
            rows=STREAM_ROWS[self.rsize], cap=STREAM_CAP,
            budget=STREAM_LDS_BUDGET)
        threads = 64 * v.W * (WPB1 if v.W == 1 else 1)
        return Template(r'''
extern "C" __global__ __launch_bounds__(${threads})
__attribute__((amdgpu_waves_per_eu(${waves})))
void ${name}(params_t prm) {
    using solver = graphdot::mgk::pair_solver<real_t, ${S}, ${R}, ${W}, ${C},
        ${nodal}, ${tab}, graph_t, node_kernel_t, edge_kernel_t, p_start_t>;
    __shared__ typename solver::lds_t lds;
    extern __shared__ __attribute__((aligned(16))) char dyn_lds[];
    solver::run(prm, lds, reinterpret_cast<real_t *>(dyn_lds));
}
''').render(threads=threads, name=self.kernel_name(v, C, nodal, tab),
            S=v.S, R=v.R, W=v.W, C=C, waves=self.waves_per_eu(v, C),
            nodal='true' if nodal else 'false',
            tab='true' if tab else 'false')

    def render_source(self, node_kernel, edge_kernel, p, node_t, edge_t,
                      variants, C, nodal=False, tab=False, weighted=False,
                      ngrad=False, maximin=False, quot=False):
        """Full translation unit for the given solver variants."""
        pd = self._params_dtype(node_kernel, edge_kernel, p)
        pfd = self._params_fd_dtype(node_kernel, edge_kernel, p)
        edge_code = self.gencode_kernel(edge_kernel, 'edge_kernel', self.real)
        edge2_t = ''
        # float builds: the edge microkernel on two records at once where the
        # record and the expression allow it (mgk_oc.h, dense product)
        if (not self.f64 and packable(edge_t)
                and packed_expression(to_real_expr(
                    edge_kernel.gen_expr('x1', 'x2')[0], 'float32'))):
            edge2_t = '\n' + declstruct2(edge_t, 'edge2_t')
            head = 'struct edge_kernel_t : edge_kernel_theta_t {\n'
            assert head in edge_code
            edge_code = edge_code.replace(
                head, head + '    using packed_edge_t = edge2_t;\n', 1)
        return Template(_TEMPLATE).render(
            real=_real_name(self.real),
            weighted='1' if weighted else '0',
            node_t=declstruct(node_t, 'node_t'),
            edge_t=declstruct(edge_t, 'edge_t') + edge2_t,
            node_kernel=self.gencode_kernel(node_kernel, 'node_kernel',
                                            self.real),
            edge_kernel=edge_code,
            p_start=self.gencode_probability(p, 'p_start', self.real),
            node_size=np.dtype(node_t).itemsize,
            edge_size=max(np.dtype(edge_t).itemsize, 1),
            params_size=pd.itemsize, params_fd_size=pfd.itemsize,
            entry_points=[self._entry_point(
                v, C, nodal, tab, ngrad, maximin,
                quot and isinstance(v, OCVariant)) for v in variants] + [''],
        )

    def _module(self, source):
        # loaded code objects are shared by every backend of the process
        key = jit.cache_key(source, self.hipcc_extra)
        mod = self._modules.get(key)
        if mod is None:
            path = jit.compile_source(source, self.hipcc_extra)
            mod = self._modules[key] = runtime.Module(jit.load_image(path))
        return mod

    # -- the three phases -----------------------------------------------------------
    def _graphs_and_kernels(self, graphs, node_kernel, edge_kernel, traits,
                            timer=None, ngrad=False):
        """Pack (or fetch the cached packing of) every graph; wrap the edge
        kernel for weighted graphs; pick the solver flavour C."""
        tic = timer.tic if timer else (lambda *_: None)
        toc = timer.toc if timer else (lambda *_: None)
        tic('transferring graphs to GPU')
        # graphs seen for the first time are packed together in one
        # vectorised pass (_devicegraph.pack_many)
        # (the same list of graphs as in a recent call, none touched since:
        # the same packings -- util.cookie.IdentityCache)
        if not isinstance(graphs, (list, tuple)):
            graphs = list(graphs)
        ckey, dgraphs = self._dgraph_lists.get(graphs)
        if dgraphs is None:
            key = (self.uuid.int, np.dtype(self.real).str)   # (an int hashes in C)
            new = [g for g in graphs if key not in g.cookie]
            if new:
                for g, dg in zip(new, pack_many(new, real=self.real,
                                                native=self.native)):
                    g.cookie[key] = dg
            dgraphs = _DeviceGraphList(g.cookie[key] for g in graphs)
            sig0 = dgraphs[0].signature
            for dg in dgraphs:
                if dg.signature != sig0:
                    self._assert_homogeneous(dgraphs[0], dg)
            dgraphs.ids = tuple(map(id, dgraphs))
            self._dgraph_lists.put(ckey, graphs, dgraphs)
        toc('transferring graphs to GPU')
        if traits.eval_gradient is True and traits.nodal is not False \
                and not ngrad:
            raise NotImplementedError(
                'nodal gradients are evaluated by finite differences over '
                'value launches (HIPBackend._nodal_gradient), not by a '
                'gradient plan')
        C = 2 if traits.eval_gradient is True and not ngrad else 1
        # attributes the microkernels read: label classes are numbered over
        # these (before the weighted wrapper: the weight is not a label)
        fields = (self._used_fields(node_kernel),
                  self._used_fields(edge_kernel))
        if dgraphs[0].weighted:
            edge_kernel = TensorProduct(weight=Product(), label=edge_kernel)
        return dgraphs, edge_kernel, C, fields

    def _quotient_graphs(self, graphs, dgraphs, traits, C, ngrad=False,
                         maximin=False):
        """The twin-leaf quotient images of the graphs of a call
        (_devicegraph.quotient_graph), or None when the
        call keeps the full images: anything but a plain graph-level value
        call -- gradient, nodal, lmin = 1, a maximin / M3 epilogue --, a graph
        with variable-length attributes, or no twin group in the whole call.
        Decided from the traits and the graphs alone; a quotient is made once
        per graph and kept in its cookie."""
        if (not self.quotient or C != 1 or ngrad or maximin
                or traits.nodal is not False
                or traits.lmin != 0 or not len(dgraphs)):
            return None
        hit = getattr(dgraphs, 'quotient', False)
        if hit is not False:
            return hit
        key = ('quotient', self.uuid.int, np.dtype(self.real).str)
        out, merged = _DeviceGraphList(), 0
        for g, dg in zip(graphs, dgraphs):
            q = g.cookie.get(key) if hasattr(g.cookie, 'get') else None
            if q is None or q.n_orig != dg.n_node:
                q = quotient_graph(dg, native=self.native)
                if q is None:
                    out = None
                    break
                g.cookie[key] = q
            merged += q.n_merged
            out.append(q)
        if out is not None and merged == 0:
            out = None
        if out is not None:
            out.ids = tuple(map(id, out))
        try:
            dgraphs.quotient = out
        except AttributeError:             # a plain list
            pass
        return out

    @staticmethod
    def _quotient_launches(launches):
        """Do all launches of a layout of quotient images run on slot
        variants of the owner-computes solver (mgk_oc.h QUOT)?"""
        return all(isinstance(L['variant'], OCVariant) and L['variant'].S > 0
                   for L in launches)

    @staticmethod
    def _code_signature(node_kernel, edge_kernel, p, dgraphs, shape):
        """What the generated code depends on: the microkernel expressions
        and record types (not the hyperparameter values), the graphs' record
        types and the output mode.  (The dtypes themselves, not their
        strings: numpy takes 15 us to print a structured dtype.)"""
        return (node_kernel.gen_expr('x1', 'x2')[0], np.dtype(node_kernel.dtype),
                edge_kernel.gen_expr('x1', 'x2')[0], np.dtype(edge_kernel.dtype),
                p.gen_expr()[0], np.dtype(p.dtype), dgraphs[0].signature,
                shape.C, shape.nodal, shape.tab, shape.gtab, shape.ngrad,
                shape.maximin, shape.quot)

    def _sources(self, used, node_kernel, edge_kernel, p, dgraphs, shape):
        """One translation unit per solver variant in use (+ the one of the
        table kernel, key 'tables', when the owner-computes solvers read
        global tables).  The node / edge / start-probability code is shared
        text; only the entry point differs."""
        # rendering is pure text work on hyperparameter-independent inputs:
        # memoised on the generated expressions and the record types
        sig = self._code_signature(node_kernel, edge_kernel, p, dgraphs,
                                   shape)
        C, gtab, ngrad = shape.C, shape.gtab, shape.ngrad
        out = {}
        todo = [(k, self.variants[k]) for k in used]
        if gtab and any(isinstance(v, OCVariant) for _, v in todo):
            todo.append(('tables', TABLES))
        opts = (np.dtype(self.real).str, tuple(self.hipcc_extra), WPB1,
                self.tables)
        for k, v in todo:
            # (the entry point also carries the variant's occupancy target)
            waves = None if v in (GENERAL, TABLES, STREAM, MFMA) else (
                self._oc_waves(v, C, ngrad) if ngrad and isinstance(
                    v, OCVariant) else self.waves_per_eu(v, C))
            key = (sig, tuple(v), waves, opts)
            if key not in self._source_cache:
                self._source_cache[key] = self.render_source(
                    node_kernel, edge_kernel, p, dgraphs[0].node_t,
                    dgraphs[0].edge_t, [v], C, shape.nodal,
                    tab=gtab if isinstance(v, OCVariant) else (
                        shape.tab and v not in (GENERAL, TABLES, STREAM,
                                                MFMA)),
                    weighted=dgraphs[0].weighted, ngrad=ngrad,
                    maximin=shape.maximin if isinstance(v, OCVariant)
                    else False, quot=shape.quot)
            out[k] = self._source_cache[key]
        return out

    def _label_blind(self, edge_kernel):
        """Is the edge microkernel (as the caller gave it, without the weight
        wrapper) a constant -- separable in one term, what the dense-tile
        MFMA solver takes (mgk_mfma.h)?  Float builds only."""
        return (not self.f64
                and os.environ.get('GD_MFMA', '1') != '0'
                and getattr(edge_kernel, 'name', None) == 'Constant')

    # -- the host plan of a call ("The host plan of a call") ---------
    def _call_shape(self, arena, traits, C, edge_kernel_in, ngrad=False,
                    maximin=0, quot=False):
        """The `CallShape` of a call on the images of `arena`: every rule on
        tables and solver menu, here and nowhere else.  `edge_kernel_in`: as
        the caller gave it.  `arena` None: tables undecided (0, False) -- the
        layout cache is keyed before an arena exists."""
        # (owner-computes solvers that evaluate the microkernels directly)
        direct = bool(ngrad or maximin)
        return CallShape(
            C=C, nodal=not quot and traits.nodal is not False, ngrad=ngrad,
            maximin=maximin, quot=quot,
            tab_bytes=0 if arena is None or direct
            else self._table_bytes(arena),
            gtab=bool(arena is not None and self._global_tables(arena)
                      and not ngrad),
            oc_only=direct,
            mfma=not quot and self._label_blind(edge_kernel_in))

    def _host_plans(self, graphs, node_kernel, edge_kernel, jobs, traits,
                    ngrad=False, maximin=0, merge_map=None, quotient=None,
                    layout_of=None, timer=None):
        """The `HostPlan`s of a call, best first and made lazily: the
        twin-leaf quotient images, when `_quotient_graphs` offers them and
        `_quotient_launches` takes their partition, then the full images.
        `precompile` and `prepare` take the first, `measured_shard_plan` all.
        `merge_map` / `quotient`: as for `prepare`; a shard runs on the
        quotient only where its whole list does.  `layout_of(dgraphs, fields,
        shape without tables, merging, make)`: the device path (`_layout`):
        its uploaded arena, and a cache hit makes neither arena nor partition."""
        tic = timer.tic if timer else (lambda *_: None)
        toc = timer.toc if timer else (lambda *_: None)
        edge_kernel_in = edge_kernel
        dgraphs, edge_kernel, C, fields = self._graphs_and_kernels(
            graphs, node_kernel, edge_kernel, traits, timer, ngrad)
        qgraphs = self._quotient_graphs(graphs, dgraphs, traits, C, ngrad,
                                        maximin) \
            if merge_map is None or quotient is not None else None
        for dgs, quot, mm in ((qgraphs, True, quotient),
                              (dgraphs, False, merge_map)):
            if dgs is None:
                continue

            def make():        # (closes over dgs, quot, mm: call it at once)
                lay = Layout()
                tic('  arena and label classes')
                if layout_of is None:
                    lay.arena = self._host_arena(dgs, fields)
                else:
                    lay.arena, lay.arena_buf, _ = self._arena(dgs, fields)
                toc('  arena and label classes')
                lay.shape = self._call_shape(
                    lay.arena, traits, C, edge_kernel_in, ngrad, maximin, quot)
                tic('  solver variants and launch order')
                lay.part = self._partition(dgs, jobs, lay.shape, mm)
                toc('  solver variants and launch order')
                return lay
            lay = make() if layout_of is None else layout_of(
                dgs, fields, self._call_shape(None, traits, C, edge_kernel_in,
                                              ngrad, maximin, quot),
                mm, make)
            if not quot or self._quotient_launches(lay.part[3]):
                yield HostPlan(dgs, edge_kernel, fields, lay.shape, lay.arena,
                               lay.part, lay)

    def precompile(self, graphs, node_kernel, edge_kernel, p, jobs, traits):
        """Compile (into the on-disk JIT cache) every code object that
        `prepare` would need for this call.  Needs hipcc but no device."""
        host = next(self._host_plans(graphs, node_kernel, edge_kernel, jobs,
                                     traits))
        sources = self._sources(host.part[1], node_kernel, host.edge_kernel,
                                p, host.dgraphs, host.shape)
        return jit.compile_many(list(sources.values()), self.hipcc_extra)

    def _layout(self, jobs, starts, timer, dgraphs, fields, shape, merge_map,
                make):
        """Everything of a plan that depends only on WHICH pairs of WHICH
        graphs are evaluated: variant per job, launch order and geometry
        (`make`: `_host_plans`), and the device copies of the job list, the
        order and `starts`.  Cached (LRU) on the identity of the packed
        graphs and a checksum of the job list, so that repeated evaluations
        with new hyperparameters -- the training loop of a Gaussian process
        -- skip the host-side work and the uploads."""
        jobs = np.ascontiguousarray(jobs)
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        # a read-only job list is recognised by identity (the kernel object
        # keeps its lists that way), anything else by checksum
        jobs_id = ('id', id(jobs)) if not jobs.flags.writeable else \
            ('crc', zlib.crc32(jobs.view(np.uint8)))
        key = (_ids(dgraphs), len(jobs), jobs_id,
               zlib.crc32(starts.view(np.uint8)), shape.C, fields,
               self.tables, shape.ngrad, shape.maximin, shape.nodal,
               shape.mfma,
               None if merge_map is None else tuple(sorted(merge_map.items())))
        hit = self._layouts.get(key)
        if hit is not None:
            self._layouts.move_to_end(key)
            return hit
        tic = timer.tic if timer else (lambda *_: None)
        toc = timer.toc if timer else (lambda *_: None)
        tic('calculating launch configuration')
        lay = make()
        lay.dgraphs, lay.jobs_host = list(dgraphs), jobs   # (keeps ids alive)
        lay.tab_bytes, lay.gtab = lay.shape.tab_bytes, lay.shape.gtab
        jobs, lay.used, lay.order_host, lay.launches = part = lay.part
        tic('  job list to the device')
        lay.n_jobs = len(jobs)
        lay.b_jobs = runtime.DeviceBuffer(max(jobs.nbytes, 8))
        lay.b_order = runtime.DeviceBuffer(max(lay.order_host.nbytes, 4))
        lay.b_starts = runtime.DeviceBuffer(max(starts.nbytes, 4))
        # jobs travel in launch order: the kernel reads jobs[t] directly
        sorted_jobs = part.jobs_sorted if part.jobs_sorted is not None \
            else np.ascontiguousarray(jobs[lay.order_host])
        part.jobs_sorted = None              # (only the device keeps them)
        lay.b_jobs.upload(sorted_jobs.view(np.uint32))
        lay.b_order.upload(lay.order_host)
        lay.b_starts.upload(starts)
        # uploads were issued on the null stream; solver launches may go to
        # non-blocking streams, which do not wait for it
        runtime.synchronize()
        toc('  job list to the device')
        self._layouts[key] = lay
        while len(self._layouts) > self.layout_cache_size:
            self._layouts.popitem(last=False)    # freed with its last plan
        toc('calculating launch configuration')
        return lay

    def _modules_of(self, host, node_kernel, p, timer=None):
        """(module per solver variant in use, dtype of the argument block):
        a repeated call -- same code -- renders, hashes and looks up nothing."""
        tic = timer.tic if timer else (lambda *_: None)
        toc = timer.toc if timer else (lambda *_: None)
        tic('code generation')
        used, edge_kernel = host.part[1], host.edge_kernel
        mkey = (self._code_signature(node_kernel, edge_kernel, p,
                                     host.dgraphs, host.shape), tuple(used),
                tuple(self.hipcc_extra), self.tables,
                None if self.occupancy is None
                else tuple(sorted(self.occupancy.items())))
        hit = self._module_sets.get(mkey)
        if hit is not None:
            toc('code generation')
            return hit
        sources = self._sources(used, node_kernel, edge_kernel, p,
                                host.dgraphs, host.shape)
        toc('code generation')
        tic('JIT')
        missing = [s for s in sources.values()
                   if jit.cache_key(s, self.hipcc_extra) not in self._modules]
        if len(missing) > 1:
            jit.compile_many(missing, self.hipcc_extra)
        modules = {k: self._module(s) for k, s in sources.items()}
        toc('JIT')
        hit = self._module_sets[mkey] = (
            modules, self._params_dtype(node_kernel, edge_kernel, p))
        return hit

    @staticmethod
    def _flag_word(traits, packed, maximin):
        return sum(flag for flag, on in (
            (F_NODAL, traits.nodal is True or traits.nodal == 'block'),
            (F_BLOCK, traits.nodal == 'block'),
            (F_DIAGONAL, traits.diagonal), (F_SYMMETRIC, traits.symmetric),
            (F_LMIN1, traits.lmin == 1), (F_PACKED, packed),
            (F_REFCOMPAT, maximin and maximin.get('reference_compat')),
        ) if on)

    def _launch_geometry(self, L):
        """Grid and global scratch of the launches whose geometry follows
        the chip: the streamed solver (cooperative) and the general solver."""
        rsize = self.rsize
        if L['variant'] == STREAM:
            # few pairs: several workgroups per pair, a cooperative
            # launch (mgk_stream.h).  M = what the chip holds at once over
            # the pairs; one workgroup per pair from half the chip up.
            # (workgroups the chip holds at once, by this build's own
            # arithmetic as well as by the runtime's: a grid beyond it
            # would wait for workgroups that wait for it)
            per_cu = max(1, min(
                runtime.max_active_blocks(L['fn'], L['threads'],
                                          L['dynamic_lds']),
                LDS_LIMIT // (L['dynamic_lds'] + 1024),
                2048 // L['threads']))
            resident = self.props.compute_units * per_cu
            parts = int(os.environ.get('GD_STREAM_PARTS', 0)) or \
                stream_parts(L.get('costs'), L['count'], resident,
                             2 * self.props.compute_units)
            parts = max(1, min(parts, resident))
            slots = int(min(L['count'], max(1, resident // parts)))
            if parts == 1:
                slots = int(min(L['count'], 2 * self.props.compute_units))
            L['parts'], L['cooperative'] = parts, parts > 1
            L['grid'] = slots * parts
            L['scratch_bytes'] = slots * L['per_wg'] * rsize
            L['sync_bytes'] = slots * 4 * (
                16 + 2 * parts * 4 * (rsize // 4)) if parts > 1 else 0
        elif L['variant'] == GENERAL:
            L['grid'] = int(min(L['count'], 2 * self.props.compute_units))
            L['scratch_bytes'] = L['grid'] * L['per_wg'] * rsize

    @staticmethod
    def _stream_hint(shape, launches, ftol):
        # Streams the launches are dealt onto (LaunchSet): three by default
        # (short launches fill the tails of long ones: +4-6 % over one, the
        # dense molecular set +10 % over two), TWO for the double value plans
        # of one-wave static layouts -- latency-bound kernels at two or three
        # waves per SIMD whose dominant launch loses more residency to a
        # third concurrent grid than its tail gains: 168.4-168.6 against
        # 166.1-166.3 M pairs/s on the headline, alternating on one box
        # (profiles/sessions.md r5_session29; float: equal; double value +
        # gradient: three, 64.5 against 63.7 M; the same plans run to
        # convergence, ftol 1e-13 and 26 iterations instead of 17: three, 126.6
        # against 125.7 M, r5_session36 -- hence the tolerance in the rule).
        # Round 6: the float value plans too -- equal on the full matrix, and on
        # a rank's share of it (354 graphs, five launches) 0.342 against 0.373 ms
        # per step (double: 0.447 against 0.455; one stream: 0.513 / 0.392;
        # scripts/fixed_cost_experiment.sh, profiles/r06_fixed_cost.log).
        return 2 if (
            shape.C == 1 and not shape.nodal and not shape.ngrad
            and len(launches) > 2 and ftol >= 1e-10
            and all(isinstance(L['variant'], OCVariant) and L['variant'].L
                    for L in launches)) else None

    def _call_buffers(self, plan, modules, node_kernel, edge_kernel):
        """The per-call device buffers (outputs, scratch) of `plan`, from the
        grow-only pool; its launches get their scratch offsets."""
        lay, launches, C = plan.layout, plan.launches, plan.C
        rsize = self.rsize
        b = dict(jobs=lay.b_jobs, order=lay.b_order, starts=lay.b_starts)
        b['gramian'] = self._buffer('gramian', plan.n_out * rsize)
        b['gradient'] = self._buffer('gradient', plan.n_grad * rsize) \
            if plan.n_grad else None
        b['iters'] = self._buffer('iters', 4 * lay.n_jobs) \
            if self.record_iterations else None
        # (launches run concurrently on several streams: every launch that
        # keeps CG vectors in global memory gets a region of its own)
        scratch_bytes = 0
        for L in launches:
            if L.get('scratch_bytes', 0):
                L['scratch_offset'] = scratch_bytes
                scratch_bytes += -(-L['scratch_bytes'] // 256) * 256
        b['scratch'] = self._buffer('scratch', scratch_bytes) \
            if scratch_bytes else None
        sync_bytes = max([L.get('sync_bytes', 0) for L in launches] + [0])
        # (a buffer of its OWN per plan: the kernels leave the barrier cells
        # clean at THIS plan's slot stride -- a pooled buffer re-used by a
        # plan of another M had its counters on leftover partial sums, and
        # the second evaluation of a backend dead-locked in its first barrier)
        b['sync'] = self._zeroed_buffer(sync_bytes) if sync_bytes else None
        # global microkernel tables of this evaluation: values (and, for the
        # gradient solvers, one plane per hyperparameter) per pair of classes
        b['tables'] = None
        if 'tables' in modules:
            c = lay.arena.classes
            planes = 1 + (len(node_kernel.gen_expr('x1', 'x2')[1]) +
                          len(edge_kernel.gen_expr('x1', 'x2')[1])
                          if C == 2 else 0)
            # (+ 2: the scalars of the evaluation, mgk_oc.h fill_tables)
            n_tab = (c['nv']**2 + c['ne']**2) * planes + 2
            b['tables'] = self._buffer('tables', n_tab * rsize)
        b['hotspot'] = self._buffer('hotspot', 4 * plan.n_out) \
            if plan.maximin else None
        return b

    def _fd_block(self, node_kernel, edge_kernel, p, q, eps):
        """The hyperparameter sets exp(log(theta) +- eps) of the central
        differences (pack_state(diff_grid=True), _backend_cuda.py:230-245)."""
        fd = np.zeros((), dtype=self._params_fd_dtype(
            node_kernel, edge_kernel, p))
        fd['q_plus'] = np.exp(np.log(q) + eps)
        fd['q_minus'] = np.exp(np.log(q) - eps)
        for which, kern in (('node', node_kernel), ('edge', edge_kernel)):
            theta = np.array(list(flatten(kern.theta)), dtype=float)
            for j_, t_ in enumerate(theta):
                fd[which + '_theta'][j_] = t_
                for s_, delta in enumerate((eps, -eps)):
                    k2 = copy.deepcopy(kern)
                    lt = np.log(theta)
                    lt[j_] += delta
                    k2.theta = fold_like(np.exp(lt), k2.theta)
                    _, val = pack_theta(k2, self.real)
                    if val is not None:
                        fd[which + '_diff'][2 * j_ + s_] = val
        return fd

    def _argument_blocks(self, plan, b, base, fd):
        """`L['args']` of every launch of `plan`: `base` with the launch's
        own fields, inside `fd` (`_fd_block`) when there is one."""
        lay = plan.layout
        for L in plan.launches:
            a = base.copy()
            a['order'] = lay.b_order.ptr + 4 * L['offset']
            a['jobs'] = lay.b_jobs.ptr + 8 * L['offset']
            a['g_capacity'] = L['gcap']
            a['n_launch_jobs'] = L['count']
            a['order_offset'] = L['offset']
            a['u_capacity'] = L['ucap']
            if L.get('scratch_bytes', 0):
                a['scratch'] = b['scratch'].ptr + L['scratch_offset']
            if L.get('parts', 1) > 1:
                a['parts'], a['sync'] = L['parts'], b['sync'].ptr
                plan.sync = (b['sync'], L['sync_bytes'])
            if L.get('dense'):
                a['flags'] |= F_DENSE
            if fd is not None:
                f_ = fd.copy()
                f_['base'] = a
                L['args'] = f_.tobytes()
            else:
                L['args'] = a.tobytes()

    def prepare(self, graphs, node_kernel, edge_kernel, p, q, eps, ftol, gtol,
                jobs, starts, nX, nY, nJ, traits, timer=None, packed=False,
                gramian_ptr=None, gradient_ptr=None, ngrad=False,
                maximin=None, merge_map=None, quotient=None):
        """Upload graphs / jobs, generate + compile code, partition the jobs.
        Returns a Plan whose launches can be replayed.  `gramian_ptr` /
        `gradient_ptr` (device addresses) make the kernels write into
        caller-owned memory, e.g. the tensor handed to the all-gather.
        `ngrad`: nodal outputs with their finite-difference Jacobian in the
        same launch (owner-computes solvers only: raises NotOwnerComputes if
        some pair does not fit one).  `maximin`: dict(diag=, diag_grad=,
        node_starts=, ld=) of device addresses -- the launch writes the
        maximin distance, its hotspot (and with `ngrad` its gradient) per
        pair instead of the nodal matrix (`maximin_distance`).  `merge_map`:
        {variant index: variant index} launch merging decided on a larger job
        list that `jobs` is a shard of (instead of by this list's counts).
        `quotient`: with a `merge_map`, the launch merging of the call on its
        twin-leaf quotient images, decided on that larger list too
        (`_sharded.measured_shard_plan`: which images and which solver a pair
        runs on must not depend on the shard it falls into), or None: the
        full images."""
        runtime.ensure_device(self.device)
        # epilogue flavour: 0 none, 1 maximin, 2 M3 (mgk_oc.h MAXIMIN)
        flavour = 0 if maximin is None else (2 if maximin.get('m3') else 1)
        # the first host plan: on the quotient images where they are taken
        host = next(self._host_plans(
            graphs, node_kernel, edge_kernel, jobs, traits, ngrad, flavour,
            merge_map, quotient, timer=timer,
            layout_of=lambda *a: self._layout(jobs, starts, timer, *a)))
        lay, shape, dgraphs = host.layout, host.shape, host.dgraphs
        edge_kernel, C = host.edge_kernel, shape.C
        modules, pd = self._modules_of(host, node_kernel, p, timer)

        plan = Plan()
        plan.layout, plan.quotient, plan.packed = lay, shape.quot, packed
        plan.traits, plan.C, plan.n_jobs = traits, C, lay.n_jobs
        plan.nX, plan.nY, plan.nJ = int(nX), int(nY), int(nJ)
        plan.keep = (lay.arena, lay.arena_buf, dgraphs)
        plan.order_host = lay.order_host
        plan.n_out = lay.n_jobs if packed else plan.nX * plan.nY
        plan.maximin, plan.ngrad = maximin is not None, ngrad
        plan.n_grad = plan.n_out * plan.nJ if (C == 2 or ngrad) else 0

        plan.launches = []
        for G in lay.launches:
            L = dict(G)
            L['module'] = modules[L['k']]
            L['tab'] = L.get('tab', False) \
                if isinstance(L['variant'], OCVariant) \
                else shape.tab and L['variant'] not in (GENERAL, STREAM, MFMA)
            L['fn'] = L['module'].function(
                self.kernel_name(L['variant'], C, shape.nodal, L['tab'],
                                 ngrad, flavour, shape.quot))
            if L['dynamic_lds'] > 64 * 1024:
                runtime.set_max_dynamic_lds(L['fn'], L['dynamic_lds'])
            self._launch_geometry(L)
            plan.launches.append(L)
        plan.stream_hint = self._stream_hint(shape, plan.launches, ftol)
        b = self._call_buffers(plan, modules, node_kernel, edge_kernel)
        plan.buffers = {k: b[k] for k in (
            'jobs', 'order', 'starts', 'gramian', 'gradient', 'iters',
            'tables', 'hotspot')}

        # the argument block all launches share
        base = np.zeros((), dtype=pd)
        base['arena'], base['jobs'], base['starts'] = \
            lay.arena_buf.ptr, lay.b_jobs.ptr, lay.b_starts.ptr
        base['gramian'] = gramian_ptr if gramian_ptr else b['gramian'].ptr
        base['gradient'] = gradient_ptr if gradient_ptr else (
            b['gradient'].ptr if b['gradient'] is not None else 0)
        for name in ('iters', 'scratch', 'tables'):
            base[name] = b[name].ptr if b[name] is not None else 0
        if maximin:
            base['diag'], base['diag_grad'] = maximin['diag'], \
                maximin.get('diag_grad', 0)
            base['node_starts'], base['diag_ld'] = maximin['node_starts'], \
                maximin['ld']
            base['hotspot'] = b['hotspot'].ptr
        base['nX'], base['nY'], base['nJ'] = plan.nX, plan.nY, plan.nJ
        base['flags'] = self._flag_word(traits, packed, maximin)
        if shape.tab or b['tables'] is not None:
            c = lay.arena.classes
            base['n_vclass'], base['n_eclass'] = c['nv'], c['ne']
            base['vrep'], base['erep'] = c['vrep'], c['erep']
        base['q'] = base['q0'] = q
        base['eps'], base['ftol'], base['gtol'] = eps, ftol, gtol
        for field, obj in (('node_kernel', node_kernel),
                           ('edge_kernel', edge_kernel), ('p_start', p)):
            dt, val = pack_theta(obj, self.real)
            if val is not None:
                base[field] = val
        self._argument_blocks(plan, b, base, self._fd_block(
            node_kernel, edge_kernel, p, q, eps) if ngrad else None)
        # launches that every solver launch depends on: the table kernel
        plan.pre_launches = []
        if b['tables'] is not None:
            c = lay.arena.classes
            plan.pre_launches.append(dict(
                variant=TABLES, module=modules['tables'],
                fn=modules['tables'].function(self.kernel_name(TABLES, C)),
                grid=int(-(-(c['nv']**2 + c['ne']**2) // 256)), threads=256,
                args=base.tobytes(), dynamic_lds=0))
        plan.params_dtype = pd
        self.last_plan = plan
        return plan

    def launch(self, plan, stream=None, concurrent=None):
        """Enqueue every launch of `plan` (asynchronous).  With `concurrent`
        (default: the backend's setting) each solver variant goes to its own
        HIP stream so that the short launches fill the tails of the long
        ones; `synchronize()` / `collect()` wait for all of them."""
        concurrent = self.concurrent if concurrent is None else concurrent
        if stream is not None:
            for L in plan.pre_launches + plan.launches:
                runtime.launch(L['fn'], L['grid'], L['threads'], L['args'],
                               stream=stream, dynamic_lds=L['dynamic_lds'],
                           cooperative=L.get('cooperative', False))
            return
        if self._launch_set is None:
            self._launch_set = LaunchSet()
        self._launch_set.enqueue(
            plan, serial=not concurrent or len(plan.launches) < 2)

    def synchronize(self):
        runtime.synchronize()

    def collect(self, plan, gramian=None, gradient=None):
        """Copy results back.  A packed plan returns one value (and nJ
        gradient entries) per job, in job order."""
        runtime.synchronize()
        rs = np.dtype(self.real)
        sync = getattr(plan, 'sync', None)
        if sync is not None:
            # the streamed solver's grid barriers: a slot whose parts did not
            # all arrive was poisoned by the watchdog (mgk_stream.h) -- its
            # results are not solutions
            cells = np.empty(sync[1] // 4, dtype=np.uint32)
            sync[0].download(cells)
            L = [L for L in plan.launches if L.get('parts', 1) > 1][0]
            stride = len(cells) // max(L['grid'] // L['parts'], 1)
            if np.any(cells[2::stride][:L['grid'] // L['parts']]):
                sync[0].upload(np.zeros(sync[0].nbytes, dtype=np.uint8))
                runtime.synchronize()
                raise RuntimeError(
                    'streamed solver: a grid-wide barrier of a cooperative '
                    f'launch ({L["grid"]} workgroups, {L["parts"]} per pair) '
                    'timed out -- the grid was not co-resident; set '
                    'GD_STREAM_PARTS=1 for one workgroup per pair')

        def fetch(buf, n, dest):
            # straight into the caller's array when it can take the bytes
            if (isinstance(dest, np.ndarray) and dest.dtype == rs
                    and dest.size == n and dest.flags.c_contiguous
                    and dest.flags.writeable):
                buf.download(dest.reshape(-1))
                return dest.reshape(-1)
            out = np.empty(n, dtype=rs)
            buf.download(out)
            if dest is not None:
                dest[:] = out.reshape(dest.shape)
            return out

        out = fetch(plan.buffers['gramian'], plan.n_out, gramian)
        grad = None
        if plan.C == 2 or getattr(plan, 'ngrad', False):
            grad = fetch(plan.buffers['gradient'], plan.n_grad, gradient)
        return out, grad

    def iterations(self, plan):
        if plan.buffers['iters'] is None:
            raise RuntimeError('create the backend with '
                               'record_iterations=True')
        it = np.empty(plan.n_jobs, dtype=np.uint32)
        plan.buffers['iters'].download(it)
        return it

    # -- nodal gradients: central finite differences in log-theta ----------------------
    def _nodal_gradient(self, graphs, node_kernel, edge_kernel, p, q, eps,
                        ftol, gtol, jobs, starts, gramian, gradient, nX, nY,
                        nJ, traits, timer):
        """Value + Jacobian of nodal outputs, as the reference defines them
        (template.cu:226-418): d/dp analytic, d/dq, d/d(node theta),
        d/d(edge theta) by central differences of re-solves at
        exp(log(theta) +- eps).  The reference warm-starts those re-solves
        in-kernel with tolerance gtol; here each perturbed system is a fresh
        value launch (hyperparameters are kernel arguments, no recompilation),
        which converges to the same differences."""
        def solve(nk, ek, qq, lmin):
            tr = traits._replace(eval_gradient=False, lmin=lmin)
            plan = self.prepare(graphs, nk, ek, p, qq, eps, ftol, gtol, jobs,
                                starts, nX, nY, nJ, tr, None)
            self.launch(plan)
            out, _ = self.collect(plan)
            return out.astype(np.float64)

        value = solve(node_kernel, edge_kernel, q, traits.lmin)
        gramian[:] = value
        shape = (nX, nJ) if traits.diagonal else (nX, nY, nJ)
        J = np.zeros(shape, dtype=np.float64, order='F')
        K = value.reshape(shape[:-1], order='F')

        # d/dp (analytic): K_nodal * (dp1/p1 + dp2/p2)   (template.cu:258-284)
        def node_p(gs):
            pv, dpv = [], []
            for g in gs:
                order = np.argsort(np.asarray(g.nodes['!i']))
                a, b = p(g.nodes)
                a = np.asarray(a, dtype=float)[order]
                b = np.asarray(b, dtype=float)
                b = b[:, order] if b.size else np.zeros((0, len(order)))
                pv.append(a)
                dpv.append(b)
            return np.concatenate(pv), np.concatenate(dpv, axis=1)
        n_p = len(list(flatten(p.theta)))
        if traits.diagonal or traits.symmetric:
            px, dpx = node_p(graphs)
            py, dpy = px, dpx
        else:
            sizes = np.array([len(g.nodes) for g in graphs])
            split = int(np.searchsorted(np.cumsum(sizes), nX, side='left')) + 1
            px, dpx = node_p(graphs[:split])
            py, dpy = node_p(graphs[split:])
        for j in range(n_p):
            if traits.diagonal:
                J[:, j] = K * 2 * dpx[j] / px
            else:
                J[:, :, j] = K * ((dpx[j] / px)[:, None]
                                  + (dpy[j] / py)[None, :])
        col = n_p

        def central(plus, minus, denom):
            nonlocal col
            d = (solve(*plus, 0) - solve(*minus, 0)) / denom
            J[..., col] = d.reshape(shape[:-1], order='F')
            col += 1

        central((node_kernel, edge_kernel, float(np.exp(np.log(q) + eps))),
                (node_kernel, edge_kernel, float(np.exp(np.log(q) - eps))),
                2 * eps * q)
        for which, kern in (('node', node_kernel), ('edge', edge_kernel)):
            theta = np.array(list(flatten(kern.theta)), dtype=float)
            for j in range(len(theta)):
                pair = []
                for delta in (eps, -eps):
                    k2 = copy.deepcopy(kern)
                    t = np.log(theta)
                    t[j] += delta
                    k2.theta = fold_like(np.exp(t), k2.theta)
                    pair.append(k2)
                if which == 'node':
                    central((pair[0], edge_kernel, q),
                            (pair[1], edge_kernel, q), 2 * eps * theta[j])
                else:
                    central((node_kernel, pair[0], q),
                            (node_kernel, pair[1], q), 2 * eps * theta[j])
        assert col == nJ, (col, nJ)
        gradient[:] = J.ravel(order='F')

    # -- maximin graph distance, fused ------------------------------------------------
    def maximin_distance(self, graphs, node_kernel, edge_kernel, p, q, eps,
                         ftol, gtol, jobs, nX, nY, nJ, traits, timer=None,
                         reference_compat=False):
        """Maximin distances (+ hotspots, + gradients with
        `traits.eval_gradient`) of the graph pairs in `jobs` without the
        nodal Gram matrix ever leaving the compute units (reference:
        metric/maximin/_backend.cu:40-407, one fused CUDA kernel): a `diag`
        launch leaves the nodal self-similarities of every graph (and their
        Jacobian) on the device, the pair launch reduces row minima / column
        minima / their maximum in LDS (mgk_oc.h, MAXIMIN).  `traits` are
        graph-level (`nodal=False`); nX, nY count graphs.  Owner-computes
        solvers only: raises NotOwnerComputes otherwise.  `reference_compat`:
        the gradient columns from q on are formed with k12 (and the distance in
        the denominator) of the last perturbed solve, as the reference's kernel
        does (_backend.cu:383); default: the unperturbed solution.  Returns (distance
        [nX nY], hotspot int32 [nX nY], gradient [nX nY nJ] or None), flat
        column-major like the other outputs."""
        plan = self._maximin_launch(
            graphs, node_kernel, edge_kernel, p, q, eps, ftol, gtol, jobs, nX,
            nY, nJ, traits, timer, reference_compat)
        dist, g = self.collect(plan)
        hot = np.empty(plan.n_out, dtype=np.int32)
        plan.buffers['hotspot'].download(hot)
        return dist, hot, g

    def maximin_distance_device(self, graphs, node_kernel, edge_kernel, p, q,
                                eps, ftol, gtol, jobs, nX, nY, nJ, traits,
                                timer=None, reference_compat=False):
        """`maximin_distance` whose results stay on the device: the same
        launches, then the pair plan's output buffers are handed over
        (`detach_outputs`) instead of collected -- ``plan.buffers['gramian']``
        holds the distances, ``plan.buffers['gradient']`` the gradient (nJ
        columns), flat column-major; no hotspots are downloaded.  Returns the
        plan once its launches are complete."""
        plan = self._maximin_launch(
            graphs, node_kernel, edge_kernel, p, q, eps, ftol, gtol, jobs, nX,
            nY, nJ, traits, timer, reference_compat, detach=True)
        self.synchronize()
        return plan

    # -- M3 graph distance, fused ------------------------------------------------------
    def m3_distance(self, graphs, node_kernel, edge_kernel, p, q, eps, ftol,
                    gtol, jobs, nX, nY, nJ, traits, timer=None):
        """M3 distances (graphdot_amd.experimental.metric.m3) of the graph
        pairs in `jobs`, fused like `maximin_distance`: a `diag` launch leaves
        the nodal self-similarities on the device, the pair launch reduces
        them with the pair's nodal solution in LDS (mgk_oc.h, MAXIMIN == 2,
        kernels named ``*_m3``).  Double backends only, no gradient;
        owner-computes solvers only (NotOwnerComputes otherwise).  Returns the
        distances [nX nY], flat column-major."""
        plan = self.m3_distance_device(graphs, node_kernel, edge_kernel, p, q,
                                       eps, ftol, gtol, jobs, nX, nY, nJ,
                                       traits, timer, detach=False)
        dist, _ = self.collect(plan)
        return dist

    def m3_distance_device(self, graphs, node_kernel, edge_kernel, p, q, eps,
                           ftol, gtol, jobs, nX, nY, nJ, traits, timer=None,
                           detach=True):
        """`m3_distance` whose result stays on the device: returns the pair
        plan once its launches are complete, ``plan.buffers['gramian']``
        holding the distances (handed over with `detach_outputs` unless
        `detach` is False)."""
        if not self.f64:
            raise TypeError('M3 distances need a double backend '
                            '(HIPBackend(real=np.float64))')
        if traits.eval_gradient is True:
            raise NotImplementedError('M3 has no gradient')
        plan = self._maximin_launch(
            graphs, node_kernel, edge_kernel, p, q, eps, ftol, gtol, jobs, nX,
            nY, nJ, traits, timer, detach=detach, m3=True)
        self.synchronize()
        return plan

    def _maximin_launch(self, graphs, node_kernel, edge_kernel, p, q, eps,
                        ftol, gtol, jobs, nX, nY, nJ, traits, timer=None,
                        reference_compat=False, detach=False, m3=False):
        """The launches of `maximin_distance` (both enqueued, nothing
        collected); returns the pair plan.  `detach`: its output buffers
        leave the pool (`detach_outputs`).  `m3`: the M3 epilogue instead
        (`m3_distance`)."""
        grad = traits.eval_gradient is True
        n = len(graphs)
        sizes = np.array([len(g.nodes) for g in graphs], dtype=np.uint32)
        node_starts = np.zeros(n + 1, dtype=np.uint32)
        np.cumsum(sizes, out=node_starts[1:])
        total = int(node_starts[-1])
        rs = np.dtype(self.real)
        # 1. nodal self-similarities (diag, nodal): stays on the device
        djobs = np.zeros(n, dtype=np.dtype([('i', np.uint32),
                                            ('j', np.uint32)]))
        djobs['i'] = djobs['j'] = np.arange(n)
        dtraits = traits._replace(symmetric=False, nodal=True, diagonal=True,
                                  eval_gradient=grad)
        dplan = self.prepare(graphs, node_kernel, edge_kernel, p, q, eps,
                             ftol, gtol, djobs, node_starts, total, 1, nJ,
                             dtraits, timer, ngrad=grad)
        if any(not isinstance(L['variant'], OCVariant)
               for L in dplan.launches):
            raise NotOwnerComputes
        self.launch(dplan)
        b_diag = self._buffer('mm_diag', total * rs.itemsize)
        b_dgrad = self._buffer('mm_diag_grad', total * nJ * rs.itemsize) \
            if grad else None
        b_ns = self._buffer('mm_node_starts', node_starts.nbytes)
        runtime.synchronize()
        runtime.check(runtime.lib().gd_memcpy_d2d(
            b_diag.ptr, dplan.buffers['gramian'].ptr, total * rs.itemsize,
            None))
        if grad:
            runtime.check(runtime.lib().gd_memcpy_d2d(
                b_dgrad.ptr, dplan.buffers['gradient'].ptr,
                total * nJ * rs.itemsize, None))
        b_ns.upload(node_starts)
        runtime.synchronize()
        # 2. the pairs
        starts = np.arange(n + 1, dtype=np.uint32)
        if not traits.symmetric:
            starts[nX:] = np.arange(n - nX + 1)
        mtraits = traits._replace(nodal=True, eval_gradient=grad)
        plan = self.prepare(
            graphs, node_kernel, edge_kernel, p, q, eps, ftol, gtol, jobs,
            starts, nX, nY, nJ, mtraits, timer, ngrad=grad,
            maximin=dict(diag=b_diag.ptr,
                         diag_grad=b_dgrad.ptr if grad else 0,
                         node_starts=b_ns.ptr, ld=total,
                         reference_compat=bool(reference_compat),
                         m3=bool(m3)))
        if detach:
            self.detach_outputs(plan)
        if grad:
            plan.buffers['gradient'].zero()
        self.launch(plan)
        return plan

    # -- the reference's backend call ---------------------------------------------------
    def __call__(self, graphs, node_kernel, edge_kernel, p, q, eps, ftol,
                 gtol, jobs, starts, gramian, gradient, nX, nY, nJ, traits,
                 timer):
        if traits.eval_gradient is True and traits.nodal is True:
            # nodal Jacobian: in the same launch as the solve (owner-computes
            # solvers, mgk_oc.h NGRAD); graphs they do not cover take the
            # host-orchestrated re-launches
            try:
                plan = self.prepare(graphs, node_kernel, edge_kernel, p, q,
                                    eps, ftol, gtol, jobs, starts, nX, nY,
                                    nJ, traits, timer, ngrad=True) \
                    if self.nodal_gradient_in_kernel else None
            except NotOwnerComputes:
                plan = None
            timer.tic('GPU kernel execution')
            if plan is not None:
                self.launch(plan)
                runtime.synchronize()
                timer.toc('GPU kernel execution')
                self.collect(plan, gramian, gradient)
                return
            self._nodal_gradient(graphs, node_kernel, edge_kernel, p, q, eps,
                                 ftol, gtol, jobs, starts, gramian, gradient,
                                 nX, nY, nJ, traits, timer)
            timer.toc('GPU kernel execution')
            return
        if traits.eval_gradient is True and traits.nodal == 'block':
            # the reference computes no gradient in this mode either
            # (template.cu:226,422: neither branch is compiled for 'block')
            traits = traits._replace(eval_gradient=False)
            gradient = None
        # (the host side of a first call makes a few thousand small objects --
        # packed-graph handles, cookies -- none of them part of a cycle: the
        # cyclic collector, which would walk the caller's whole heap of graphs
        # for ~8 ms if its threshold fell inside, waits until the call is over)
        # (counted and thread-safe, GD_PAUSE_GC=0 turns it off: util/gcpause.py)
        with gcpause.paused():
            plan = self.prepare(graphs, node_kernel, edge_kernel, p, q, eps,
                                ftol, gtol, jobs, starts, nX, nY, nJ, traits,
                                timer)
            timer.tic('GPU kernel execution')
            self.launch(plan)
            runtime.synchronize()
            timer.toc('GPU kernel execution')
            self.collect(plan, gramian, gradient)
