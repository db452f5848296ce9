#!/usr/bin/env python
"""Gram-matrix throughput of the marginalized graph kernel on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W]
                    [--config 3|2|tang2019|large] [--dtype f64|f32] [--gradient]
                    [--graphs n] [--sharded] [--serial] [--dump-outputs DIR]

A *step* is one full pass of the hot path over the batch: every pair of the
symmetric Gram matrix of the workload is solved from device-resident graphs,
job list and hyperparameters into the device-resident result.

  --config 3 (default)  the synthetic QM7-like set, 1000 molecules, 500 500
                        pairs (BASELINE.json's headline configuration;
                        SURVEY.md 8d), fp64 by default as BASELINE.json names it
  --config 2            256 weighted Newman-Watts-Strogatz graphs of 8..48
                        nodes, 32 896 pairs, KroneckerDelta node x
                        SquareExponential edge kernels (BASELINE.json config 2;
                        reference workload benchmark/kernel/marginalized/
                        time_kernel.py:14-29), fp32 by default (the reference
                        solver's arithmetic)
  --config tang2019     256 dense from_ase-like molecular graphs under the
                        reference's Tang2019MolecularKernel preset (on-the-fly
                        solvers)
  --config large        protein-like spatial graphs of 150-600 atoms (default
                        32 graphs = 528 pairs; --graphs n for fewer): the
                        regime of example/perfbench/protein-time-to-solution.py,
                        the streamed solver of csrc/device/mgk_stream.h
  --gradient            value + dK/dtheta (the kernel part of config 5)
  --gpr                 config 5 end to end on one GPU: GPR log marginal
                        likelihood + gradient step (kernel + dense algebra)

With N > 1 (launched by torch.distributed.run, one rank per GPU) the pairs are
sharded over the ranks and one RCCL all-gather per step reassembles the packed
results (`graphdot_amd.kernel.marginalized._sharded.ShardedStep`, the code
path of `distributed_backend()`); `--sharded` takes that path on one rank too.

`--dump-outputs DIR` writes what the timed path computed in its last step --
the arrays a caller of that path receives, in the solver's arithmetic -- as
DIR/<name>.npy (rank 0), for comparing two builds output for output: the
inputs are seeded, so the same arguments give the same inputs.

Prints ONE JSON line on rank 0 (contract in the task statement) with
"roofline" (dominant kernel; durations from HIP events on the launch streams),
"step_aggregate" (all launches of a step against the step time),
"cpu_baseline" (the C oracle timed on this host, rank 0, N = 1) and
"api_inclusive" (numpy in -> numpy out through MarginalizedGraphKernel).
"""
import argparse
import json
import os
import sys
import time

# the host driver only supports dmabuf IPC (RCCL / cross-process tensors)
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0                       # MI355X_MICROARCH.md
VALU_PEAK_TF = {'f32': 157.3, 'f64': 78.6}  # vector (non-MFMA) peaks
LDS_PEAK_TBS = {'f32': 75.0, 'f64': 150.0}  # ds_read_b32 / ds_read_b64 aggregate


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=None,
                    help='timed steps (default: 200; 5 for --config large, '
                         '9 second launches for --config nws48)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', default='3',
                    choices=['2', '3', 'nws48', 'tang2019', 'large'])
    ap.add_argument('--batch', default='1,16,128',
                    help='--config nws48: batch sizes of the reference harness')
    ap.add_argument('--graphs', type=int, default=None,
                    help='number of graphs (default: 1000 for config 3, '
                         '256 for config 2)')
    ap.add_argument('--dtype', default=None, choices=['f32', 'f64'],
                    help='arithmetic of the solver (default: f64 for config '
                         '3 as BASELINE.json names it; f32, the reference '
                         'CUDA solver\'s arithmetic, for config 2)')
    ap.add_argument('--ftol', type=float, default=None,
                    help='stopping tolerance of the value solve, sqrt(rTr) < '
                         'ftol N (reference marginalized_kernel.h:449; '
                         'default: the reference\'s, 1e-8).  The fp64 line '
                         'also carries a figure at 1e-13 (converged)')
    ap.add_argument('--no-f32', action='store_true',
                    help='skip the short measurement in the other arithmetic')
    ap.add_argument('--gradient', action='store_true',
                    help='also evaluate dK/dtheta (config 5 kernel part)')
    ap.add_argument('--gpr', action='store_true',
                    help='configuration 5 end to end on one GPU: a step is one '
                         'log-marginal-likelihood + gradient evaluation of a '
                         'Gaussian process on the set (kernel + dK/dtheta on '
                         'the solver, dense algebra through torch on the same '
                         'GPU); value = pairs of the Gram matrix per second of '
                         'that step')
    ap.add_argument('--fit', action='store_true',
                    help='with --gpr: configuration 5 as BASELINE.json words '
                         'it, a hyperparameter FIT -- L-BFGS-B on the log '
                         'marginal likelihood from the default '
                         'hyperparameters (reference gpr.py:62-136) with '
                         'synthetic energies as targets; reports '
                         'iterations, objective evaluations, ms per '
                         'evaluation and the total')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-api', action='store_true',
                    help='skip the numpy-in / numpy-out measurement')
    ap.add_argument('--sharded', action='store_true',
                    help='one rank through the multi-GPU code path (process '
                         'group of size 1, RCCL all-gather, device reassembly)')
    ap.add_argument('--share-devices', action='store_true',
                    help='allow more ranks than GPUs: ranks share devices and '
                         'the all-gather goes through gloo on host memory '
                         '(tests on a one-GPU box; without it a node with '
                         'fewer GPUs than --gpus is an error on every rank)')
    ap.add_argument('--pipeline', action='store_true',
                    help='sharded steps overlap: the solvers of a step run '
                         'during the all-gather and the reassembly of the '
                         'previous one (default: one after the other -- on '
                         'one GPU the extra cross-stream dependencies cost '
                         'more than the overlap hides, DESIGN.md section 8)')
    ap.add_argument('--serial', action='store_true',
                    help='all solver variants on one stream (default: dealt '
                         'onto three HIP streams so short launches fill the '
                         'tails of long ones)')
    ap.add_argument('--isolated-steps', type=int, default=3,
                    help='serial steps after the timed region that give the '
                         'isolated per-kernel durations (0: skip)')
    ap.add_argument('--cpu-seconds', type=float, default=12.0)
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the outputs of the last timed step as '
                         'DIR/<name>.npy (float32/float64, at most 64 MiB '
                         'in all; a fixed seeded sample of the pairs beyond '
                         'that)')
    args = ap.parse_args()
    if args.steps is not None and args.steps < 1:
        ap.error('--steps must be at least 1')
    return args


DUMP_LIMIT_BYTES = 64 << 20
NPY_HEADER_BYTES = 128


def dump_outputs(dirname, arrays, pairs=None):
    """`--dump-outputs`: `arrays` by name as DIR/<name>.npy, float32 or
    float64.  If together they exceed DUMP_LIMIT_BYTES and `pairs` = (i, j)
    is given, the arrays whose two leading axes are the matrix are written
    at a fixed seeded sample of those pairs instead (DIR/<name>_sample.npy,
    the pairs as DIR/sample_pairs.npy)."""
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    for k, v in arrays.items():
        if v.dtype not in (np.float32, np.float64):
            arrays[k] = v.astype(np.float64)

    def size(arrays):
        return sum(v.nbytes + NPY_HEADER_BYTES for v in arrays.values())
    total = size(arrays)
    if total > DUMP_LIMIT_BYTES and pairs is not None:
        i, j = pairs
        per_pair = sum(v[0, 0].nbytes for v in arrays.values() if v.ndim >= 2)
        rest = sum(v.nbytes for v in arrays.values() if v.ndim < 2) \
            + NPY_HEADER_BYTES * (len(arrays) + 1)
        m = min(len(i), (DUMP_LIMIT_BYTES - rest) // (per_pair + 16))
        sel = np.sort(np.random.default_rng(0).choice(len(i), size=m,
                                                      replace=False))
        si, sj = i[sel], j[sel]
        arrays = {(k + '_sample' if v.ndim >= 2 else k):
                  (v[si, sj] if v.ndim >= 2 else v)
                  for k, v in arrays.items()}
        arrays['sample_pairs'] = np.column_stack((si, sj)).astype(np.float64)
        total = size(arrays)
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f'--dump-outputs: {total} bytes exceed the limit')
    os.makedirs(dirname, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(dirname, k + '.npy'), v)


# ---- algorithmic work of a set of jobs ----------
def algorithmic_bytes(arena, ji, jj, rsize, n_cols):
    """Compulsory HBM bytes of a pair = both graph images (as packed in HBM)
    + two 32-byte headers + the result."""
    blob = np.diff(np.concatenate((arena.blob_start, [arena.nbytes])))
    return (blob[ji] + blob[jj] + 64 + rsize * n_cols).astype(np.int64)


def survey_bytes_per_graph(graphs):
    """the compulsory HBM bytes of one graph in the
    REFERENCE's device layout -- 32-byte header, per node the AoS record
    (fp32 attributes) + 4-byte degree, per directed nonzero the edge record,
    32 bytes per non-empty 8 x 8 adjacency tile (octile header)."""
    from graphdot_amd.kernel.marginalized._devicegraph import pack_many
    dgs = pack_many(graphs, real=np.float32)
    out = np.zeros(len(dgs), dtype=np.int64)
    for k, g in enumerate(dgs):
        oi = g.perm[g.nz['i']].astype(np.int64)     # original node ids
        oj = g.perm[g.nz['j']].astype(np.int64)
        n_octile = len(np.unique((oi // 8) * 65536 + oj // 8))
        out[k] = 32 + g.n_node * (np.dtype(g.node_t).itemsize + 4) \
            + g.n_nz * np.dtype(g.edge_t).itemsize + 32 * n_octile
    return out


def algorithmic_flops(n_node, n_nz, ji, jj, iters, Fv=9, Fe=8):
    """k (2 nnzx + 17 N) + nnzx F_e + N F_v (cached edge/node values)."""
    N = n_node[ji] * n_node[jj]
    nnzx = n_nz[ji] * n_nz[jj]
    return iters * (2 * nnzx + 17 * N) + nnzx * Fe + N * Fv


def algorithmic_lds_reals(n_node, n_nz, ji, jj, iters):
    """Per CG iteration 2 reals per product-graph nonzero (gather + U) and
    10 per row."""
    N = n_node[ji] * n_node[jj]
    nnzx = n_nz[ji] * n_nz[jj]
    return iters * (2 * nnzx + 10 * N)


class LocalStep:
    """One rank, no collective: the plan's launches through a `LaunchSet`
    (table kernel on the null stream, solver launches on three streams, ordered
    against the previous step by device-side events)."""

    def __init__(self, backend, plan):
        from graphdot_amd.hip import runtime
        from graphdot_amd.kernel.marginalized._backend_hip import LaunchSet
        self.rt, self.plan, self.set = runtime, plan, LaunchSet()

    def enqueue(self, events=None, serial=False):
        self.set.enqueue(self.plan, events, serial)

    def synchronize(self):
        self.rt.synchronize()


def workload(args):
    import cases
    if args.config == 'tang2019':
        n = args.graphs or 256
        graphs = cases.tang2019_graphs(n)
        knode, kedge, q = cases.tang2019_kernels()
        name = (f'Tang2019-style dense molecular graphs ({n} from_ase-like '
                'molecules, <= 23 atoms, tent-weighted adjacency within '
                '3 sqrt(r_i r_j): 88 % dense, degree up to 22; seed 2019, '
                f'{n * (n + 1) // 2} pairs incl. diagonal), '
                'Tang2019MolecularKernel: KroneckerDelta(0.2) element x '
                'SquareExponential(0.05) length, q=0.01')
        return graphs, knode, kedge, q, name, (2, 6)
    if args.config == 'large':
        n = args.graphs or 32
        graphs = cases.protein_like_graphs(n)
        knode, kedge, q = cases.tang2019_kernels()
        name = (f'large spatial graphs ({n} protein-like point clouds of '
                '150-600 atoms, edges within 2.7 A with tent weights: 6-25 '
                'neighbours per atom, product graphs of 2e4-3.6e5 rows; seed '
                f'3000, {n * (n + 1) // 2} pairs incl. diagonal; the regime of '
                'example/perfbench/protein-time-to-solution.py), '
                'Tang2019MolecularKernel: KroneckerDelta(0.2) element x '
                'SquareExponential(0.05) length, q=0.01')
        return graphs, knode, kedge, q, name, (2, 6)
    if args.config == 3:
        n = args.graphs or 1000
        graphs = cases.config3_graphs(n)
        knode, kedge, q = cases.config3_kernels()
        name = (f'QM7-like synthetic set ({n} molecules, seed 7165, '
                f'{n * (n + 1) // 2} pairs incl. diagonal), TensorProduct '
                'atom/bond microkernels, q=0.01')
        F = (9, 8)
    else:
        n = args.graphs or 256
        graphs = cases.config2_graphs(n, seed=0)
        knode, kedge, q = cases.config2b_kernels()
        name = (f'config 2: {n} weighted Newman-Watts-Strogatz graphs (k=5, '
                f'p=0.05, 8..48 nodes, seed 0, {n * (n + 1) // 2} pairs incl. '
                'diagonal), KroneckerDelta node x SquareExponential edge '
                'microkernels, q=0.05')
        F = (2, 6)
    return graphs, knode, kedge, q, name, F


def measure_other_arithmetic(name, graphs, knode, kedge, q, jobs, starts, n,
                             steps, warmup, device, ftol=None, note=None):
    """Short measurement of the same step in the other arithmetic, or at
    another stopping tolerance (N = 1): reported next to the headline number,
    never instead of it.  Returns (dict, result matrix)."""
    from graphdot_amd.hip import runtime
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend, \
        LaunchSet
    real = np.float32 if name == 'f32' else np.float64
    backend = HIPBackend(device=device, real=real, record_iterations=True)
    kernel = MarginalizedGraphKernel(knode, kedge, q=q, backend=backend)
    ftol = kernel.ftol if ftol is None else ftol
    plan = backend.prepare(graphs, knode, kedge, kernel.p, kernel.q,
                           kernel.eps, ftol, kernel.gtol, jobs, starts,
                           n, n, kernel.n_dims,
                           kernel.traits(symmetric=True))
    # (issued like the headline's steps: back to back through a LaunchSet,
    # one host synchronisation at the end)
    ls = LaunchSet()
    for _ in range(max(warmup, 1)):
        ls.enqueue(plan)
    runtime.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ls.enqueue(plan)
    runtime.synchronize()
    dt = (time.perf_counter() - t0) / steps
    got, _ = backend.collect(plan)
    iters = backend.iterations(plan)
    return {'dtype': name, 'ftol': ftol, 'value': len(jobs) / dt,
            'unit': 'graph-pairs/s', 'ms_per_step': 1e3 * dt, 'steps': steps,
            'mean_cg_iterations': float(np.mean(iters)),
            'note': note or 'same step, same graphs, solver built for the '
                    'other arithmetic (f32 = the reference CUDA solver\'s)'}, \
        np.array(got).reshape(n, n, order='F')


def measure_api(graphs, knode, kedge, q, real, device, gradient, n_pairs):
    """numpy in -> numpy out, as a user of the reference calls it
    (`MarginalizedGraphKernel.__call__`): a fresh backend's first call (graph
    packing, code-object load, upload, solve, download) and the repeated call
    of a training loop (cached layout; new kernel arguments, solve, D2H of the
    matrix, the reference's float64 conversion)."""
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    def forget():
        for g in graphs:                  # forget earlier packings
            for key in [k_ for k_ in g.cookie if k_ != 'rowtypes']:
                del g.cookie[key]

    forget()
    backend = HIPBackend(device=device, real=real)
    kernel = MarginalizedGraphKernel(knode, kedge, q=q, backend=backend)
    t0 = time.perf_counter()
    # (GD_API_TIMING=1: the call's own timer report, on stderr)
    kernel(graphs, eval_gradient=gradient,
           timing=os.environ.get('GD_API_TIMING') == '1')
    first = time.perf_counter() - t0
    # (the code objects of this workload are already loaded in this process:
    # `first` is graph packing + job layout + uploads + solve + download)
    reps = 5
    each = []
    for _ in range(reps):
        t0 = time.perf_counter()
        kernel(graphs, eval_gradient=gradient)
        each.append(time.perf_counter() - t0)
    # the same on two more fresh backends: what the first call of THIS
    # process paid once (the job list of an n x n matrix, first touches of
    # the host library's code and of numpy's) is not in these
    again = []
    for _ in range(2):
        forget()
        k2 = MarginalizedGraphKernel(knode, kedge, q=q, backend=HIPBackend(
            device=device, real=real))
        t0 = time.perf_counter()
        k2(graphs, eval_gradient=gradient)
        again.append(time.perf_counter() - t0)
        del k2
    rep = float(np.median(each))     # (an occasional collector pause in one
    #                                    of the calls is not the call's cost)
    return {'first_call_ms': 1e3 * first,
            'fresh_backend_call_ms': [round(1e3 * t, 3) for t in again],
            'repeat_call_ms': 1e3 * rep,
            'repeat_calls_ms': [round(1e3 * t, 3) for t in each],
            'value': n_pairs / rep, 'unit': 'graph-pairs/s',
            'note': 'host-, PCIe- and conversion-inclusive; never `value`'}


def init_ranks(world, local_rank, share_devices=False):
    """Process group of a multi-rank run: RCCL ("nccl") with one GPU per rank.
    A node that shows fewer GPUs than ranks is an ERROR (every rank leaves
    with a non-zero code before any group is formed: a number measured with
    ranks sharing a device over gloo must never pass for an N-GPU number)
    unless `--share-devices` asks for exactly that (tests on a one-GPU box:
    ranks share devices, the all-gather goes through gloo on host memory).
    Returns (torch, dist, host_collective, device ordinal)."""
    import torch
    import torch.distributed as dist
    if world == 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(29500 + os.getpid() % 400))
        os.environ.setdefault('RANK', '0')
        os.environ.setdefault('WORLD_SIZE', '1')
    n_dev = torch.cuda.device_count()
    host_collective = False
    if n_dev >= world:
        torch.cuda.set_device(local_rank)
        dist.init_process_group('nccl', device_id=torch.device(
            'cuda', local_rank))
    elif not share_devices:
        sys.stderr.write(
            f'bench.py: --gpus {world} needs {world} distinct GPUs, this '
            f'node shows {n_dev} (rank {os.environ.get("RANK", 0)}); '
            'pass --share-devices to let ranks share a device over gloo '
            '(tests only)\n')
        sys.exit(3)
    else:
        # fewer GPUs than ranks, asked for explicitly: ranks share devices
        # and the all-gather goes through gloo on host memory
        host_collective = True
        local_rank = local_rank % max(n_dev, 1)
        torch.cuda.set_device(local_rank)
        dist.init_process_group('gloo')
    return torch, dist, host_collective, local_rank


def gpr_step_line(args, world, rank, local_rank):
    """`--gpr`: the caller of configuration 5 (SURVEY 8f rank 3,
    graphdot/model/gaussian_process/gpr.py:222-268): one log marginal
    likelihood + gradient evaluation per step.  On N ranks the kernel matrix
    and its gradient are pair-sharded (`distributed_backend`), all-gathered
    and reassembled on every rank's device, where the regressor picks them up
    (`device_gram`): no host arrays on the way; the dense algebra (1-2 ms) is
    replicated."""
    import torch                                    # noqa: F401  (first)
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.marginalized._sharded import distributed_backend
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    real = np.float32 if args.dtype == 'f32' else np.float64
    n = args.graphs or 1000
    graphs = cases.config3_graphs(n)
    knode, kedge, q = cases.config3_kernels()
    dist, host_collective = None, False
    if world > 1 or args.sharded:
        torch, dist, host_collective, local_rank = init_ranks(
            world, local_rank, args.share_devices)
        backend = distributed_backend(real=real, device=local_rank,
                                      shard_single_rank=True)
    else:
        backend = HIPBackend(real=real, device=local_rank)
    if args.fit:
        line = gpr_fit_line(args, world, rank, backend, graphs, real, dist,
                            host_collective)
        if dist is not None:
            dist.destroy_process_group()
        return line
    kernel = MarginalizedGraphKernel(knode, kedge, q=q, backend=backend)
    y = np.random.default_rng(0).normal(size=n)
    d = kernel.diag(graphs)
    gpr = GaussianProcessRegressor(kernel, alpha=float(1e-2 * d.mean()),
                                   normalize_y=True)
    gpr.X, gpr.y = graphs, y
    theta = np.array(kernel.theta)
    parts = {'kernel': 0.0, 'linalg': 0.0}

    def barrier():
        torch.cuda.synchronize()
        if dist is not None and world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    value = None
    for w in range(max(args.warmup, 1)):
        value = gpr.log_marginal_likelihood(theta + 1e-3 * w,
                                            eval_gradient=True)
    barrier()
    t0 = time.perf_counter()
    for it in range(args.steps):
        last = gpr.log_marginal_likelihood(theta + 1e-3 * it,
                                           eval_gradient=True)
        for k in parts:
            parts[k] += gpr.last_timing[k]
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {
            'log_marginal_likelihood': np.atleast_1d(np.asarray(
                last[0], dtype=np.float64)),
            'log_marginal_likelihood_gradient': last[1]})
    # (the sharded step the likelihood's gradient came from)
    step_ = getattr(backend, 'last_step', None)
    # (was the regressor handed device tensors -- device_gram -- or did it
    # fall back to the numpy kernel protocol?)
    on_device = gpr._device_gramian(gpr._dense(), kernel, graphs,
                                    False) is not None
    # per rank: kernel part (solvers of the shard + all-gather of the values
    # + reassembly), dense algebra (replicated factorisation + this rank's
    # share of the gradient contraction + the all-reduce of n_theta numbers),
    # and the phases of the sharded kernel step by device events
    mine = {'kernel_ms': 1e3 * parts['kernel'] / args.steps,
            'dense_ms': 1e3 * parts['linalg'] / args.steps}
    if step_ is not None:
        ph = step_.phase_ms(steps=3)
        mine.update(shard_ms=ph['shard_ms'], collective_ms=ph[
            'all_gather_ms'] + ph['reassembly_ms'], all_gather_ms=ph[
            'all_gather_ms'], reassembly_ms=ph['reassembly_ms'],
            gradient_gathered=bool(step_.gather_gradient),
            factorisation_overlaps_gradient_solves=bool(
                backend.overlaps_dense_algebra()))
    per_rank = [mine]
    if dist is not None and world > 1:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    if dist is not None and world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device='cpu' if host_collective else 'cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # every rank evaluated the same objective from its own copy
        v = torch.tensor([value[0]], dtype=torch.float64,
                         device='cpu' if host_collective else 'cuda')
        lo, hi = v.clone(), v.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        assert float(lo) == float(hi), 'ranks disagree on the likelihood'
    if dist is not None:
        dist.destroy_process_group()
    if rank != 0:
        return None
    dt = elapsed / args.steps
    n_pairs = n * (n + 1) // 2
    return {
        'metric': 'graph-pairs/sec (GPR likelihood + gradient step)',
        'value': n_pairs / dt, 'unit': 'graph-pairs/s', 'n_gpus': world,
        'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': 1e3 * dt,
        'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None,
        'dtype': args.dtype, 'data': 'synthetic',
        'config': {'workload': f'GPR log marginal likelihood + gradient on '
                               f'the QM7-like set ({n} molecules, {n_pairs} '
                               'pairs, 7 hyperparameters): value + dK/dtheta '
                               'on the solver, Cholesky and the gradient '
                               'contractions in float64 torch on the same GPU',
                   'graphs': n, 'pairs': n_pairs,
                   'parallelism': (f'pair-sharded x{world}: values '
                                   'all-gathered and reassembled on the '
                                   'device, gradient contracted pair shard '
                                   'by pair shard + one all-reduce of '
                                   'n_theta numbers, factorisation replicated')
                   if dist is not None else 'single'},
        'kernel_ms': 1e3 * parts['kernel'] / args.steps,
        'dense_algebra_ms': 1e3 * parts['linalg'] / args.steps,
        'per_rank': {k: [r.get(k) for r in per_rank] for k in per_rank[0]},
        'device_resident_kernel_matrix': bool(on_device),
        'collective': None if dist is None else
        ('gloo/host' if host_collective else 'nccl(RCCL)'),
        'roofline': None, 'cpu_baseline': None}


def gpr_fit_line(args, world, rank, backend, graphs, real, dist,
                 host_collective):
    """`--gpr --fit`: BASELINE.json's configuration 5 as it is worded, a
    hyperparameter fit.  `GaussianProcessRegressor.fit` with
    `optimizer=True` (reference model/gaussian_process/gpr.py:62-136:
    scipy L-BFGS-B on the log marginal likelihood within the kernel's
    bounds, gradient from dK/dtheta), from the default hyperparameters, on
    the QM7-like set with synthetic energies.  Every objective evaluation is
    one value + gradient Gram matrix on the solver plus the dense algebra on
    the same GPU; on N ranks the pairs are sharded and every rank runs the
    same optimiser on the same (bit-equal) numbers."""
    import torch
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    n = len(graphs)
    knode, kedge, q = cases.config3_fit_kernels()
    kernel = MarginalizedGraphKernel(knode, kedge, q=q, q_bounds=(1e-3, 0.5),
                                     backend=backend)
    y = cases.synthetic_energies(graphs)
    gpr = GaussianProcessRegressor(kernel, alpha=1e-2, optimizer=True,
                                   normalize_y=True)
    # warm-up: code objects, graph images, job layout, torch's handles
    gpr.X, gpr.y = graphs, y
    theta0 = np.array(kernel.theta)
    start = None
    for _ in range(max(args.warmup, 1)):
        start = gpr.log_marginal_likelihood(theta0, eval_gradient=True)[0]
    # (the line search of this fit overshoots once into hyperparameters whose
    # kernel matrix is not positive definite: that evaluation takes the
    # pseudo-inverse like the reference's, base.py:108-127 -- 22 ms of
    # torch.linalg.eigh at n = 1000, but 205 ms the first time a process
    # calls it (library initialisation, scripts/fit_probe.py): warmed here
    # like the code objects above)
    if torch.cuda.is_available():
        w_ = torch.randn(256, 256, dtype=torch.float64, device='cuda')
        torch.linalg.eigh(w_ + w_.T)
        del w_
    evals, parts = [0], {'kernel': 0.0, 'linalg': 0.0}
    objective = gpr.log_marginal_likelihood

    def counted(*a, **kw):
        out = objective(*a, **kw)
        evals[0] += 1
        for k in parts:
            parts[k] += gpr.last_timing[k]
        return out
    gpr.log_marginal_likelihood = counted
    torch.cuda.synchronize()
    if dist is not None and world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    gpr.fit(graphs, y)            # (tol: the reference's default, 1e-5)
    torch.cuda.synchronize()
    if dist is not None and world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    n_fit_evals = evals[0]
    res = gpr.optimization_result
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {
            'theta': np.exp(res.x),
            'objective': np.atleast_1d(np.asarray(res.fun,
                                                  dtype=np.float64))})
    if dist is not None and world > 1:
        dev = 'cpu' if host_collective else 'cuda'
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        v = torch.tensor([float(res.fun)], dtype=torch.float64, device=dev)
        lo, hi = v.clone(), v.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        assert float(lo) == float(hi), 'ranks disagree on the optimum'
    if rank != 0:
        return None
    n_pairs = n * (n + 1) // 2
    return {
        'metric': 'graph-pairs/sec (GPR hyperparameter fit)',
        'value': n_fit_evals * n_pairs / elapsed, 'unit': 'graph-pairs/s',
        'n_gpus': world, 'steps': n_fit_evals, 'warmup': args.warmup,
        'ms_per_step': 1e3 * elapsed / max(n_fit_evals, 1),
        'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None,
        'dtype': args.dtype, 'data': 'synthetic',
        'config': {'workload': f'GPR hyperparameter fit on the QM7-like set '
                               f'({n} molecules, {n_pairs} pairs per kernel '
                               'matrix, 7 hyperparameters, synthetic '
                               'energies): scipy L-BFGS-B on the log '
                               'marginal likelihood from the default '
                               'hyperparameters, tol 1e-5 (the reference\'s default); a step is one '
                               'objective evaluation (value + dK/dtheta on '
                               'the solver, Cholesky and gradient '
                               'contractions in float64 on the same GPU)',
                   'graphs': n, 'pairs': n_pairs,
                   'parallelism': (f'pair-sharded x{world}, device-resident '
                                   'reassembly, replicated dense algebra')
                   if dist is not None else 'single'},
        'fit': {'iterations': int(res.nit), 'objective_evaluations':
                n_fit_evals, 'total_s': elapsed,
                'ms_per_evaluation': 1e3 * elapsed / max(n_fit_evals, 1),
                'kernel_ms_per_evaluation':
                1e3 * parts['kernel'] / max(n_fit_evals, 1),
                'dense_algebra_ms_per_evaluation':
                1e3 * parts['linalg'] / max(n_fit_evals, 1),
                'objective_start': float(start),
                'objective_final': float(res.fun),
                'theta_start': [float(v) for v in np.exp(theta0)],
                'theta_final': [float(v) for v in np.exp(res.x)],
                'message': str(res.message)},
        'collective': None if dist is None else
        ('gloo/host' if host_collective else 'nccl(RCCL)'),
        'roofline': None, 'cpu_baseline': None}


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks as
    children (the driver's own launch line) and leave with their exit code.
    Nothing in THIS process has touched the GPU yet."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] \
        + sys.argv[1:]
    return subprocess.call(cmd)


def nws48_line(args):
    """`--config nws48`: the reference's own benchmark harness
    (benchmark/kernel/marginalized/time_kernel.py:43-72): `batch` graphs of 48
    nodes (one Newman-Watts-Strogatz topology, random labels and weights),
    KroneckerDelta label kernels; first launch = a fresh kernel object's first
    evaluation (graph packing, job layout, code-object load from the JIT
    cache -- the reference compiles CUDA here -- upload, solve, download),
    second launch = the same evaluation again; numpy in, numpy out."""
    import cases
    from graphdot_amd.hip import runtime
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    real = np.float32 if args.dtype == 'f32' else np.float64
    runtime.ensure_device()
    runtime.DeviceBuffer(1 << 20)             # context and allocator are up
    knode, kedge, q = cases.nws48_kernels()
    rows, outputs = [], {}
    # second launches per round: round 0 (which loads the code objects) is
    # the warm-up, the --steps timed ones are dealt over rounds 1-3
    reps = [3] + [args.steps // 3 + (r < args.steps % 3) for r in range(3)]
    for batch in [int(b) for b in args.batch.split(',')]:
        graphs = cases.nws48_graphs(batch)
        first, second = [], []
        for rnd in range(4):
            for g in graphs:
                for key in [k_ for k_ in g.cookie if k_ != 'rowtypes']:
                    del g.cookie[key]
            kernel = MarginalizedGraphKernel(
                knode, kedge, q=q, backend=HIPBackend(real=real))
            t0 = time.perf_counter()
            K = kernel(graphs, nodal=False)
            first.append(time.perf_counter() - t0)
            for _ in range(reps[rnd]):
                t0 = time.perf_counter()
                K_last = kernel(graphs, nodal=False)
                second.append(time.perf_counter() - t0)
        outputs[f'K_batch{batch}'] = K_last
        plan = kernel.backend.last_plan
        n_pairs = batch * (batch + 1) // 2
        rows.append({
            'batch': batch, 'pairs': n_pairs,
            'first_launch_cold_ms': 1e3 * first[0],
            'first_launch_ms': 1e3 * float(np.median(first[1:])),
            'second_launch_ms': 1e3 * float(np.median(second[3:])),
            'launches': [[L['variant'].W, L['variant'].S, L['variant'].R,
                          int(L['count'])] for L in plan.launches],
            'finite': bool(np.all(np.isfinite(K))),
            'symmetric': bool(np.array_equal(K, K.T))})
    big = rows[-1]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, outputs)
    return {
        'metric': 'graph-pairs/sec (Gram matrix, 2nd launch, numpy in/out)',
        'value': big['pairs'] / (1e-3 * big['second_launch_ms']),
        'unit': 'graph-pairs/s', 'n_gpus': 1, 'steps': args.steps,
        'warmup': 1,
        'ms_per_step': big['second_launch_ms'], 'higher_is_better': True,
        'scaling': 'strong', 'vs_baseline': None, 'dtype': args.dtype,
        'data': 'synthetic',
        'config': {'workload': 'reference benchmark harness '
                               '(time_kernel.py:14-72): batches of 48-node '
                               'NWS graphs (k=5, p=0.05, seed 0), integer '
                               'node / edge labels, weights 1..4, '
                               'KroneckerDelta(0.5) kernels, q=0.01; '
                               f'value: batch {big["batch"]}, 2nd launch',
                   'graphs': big['batch'], 'pairs': big['pairs'],
                   'parallelism': 'single'},
        'latency': rows,
        'note': 'host-, PCIe- and conversion-inclusive latencies of the '
                'public API; first_launch_cold_ms also loads the code '
                'objects from the on-disk JIT cache',
        'roofline': None, 'cpu_baseline': None}


def effective_cpus():
    """CPUs this process may really use: the affinity mask, capped by the
    container's CPU quota (cgroup v2 cpu.max / v1 cfs quota)."""
    n = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, per = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if q != 'max':
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = int(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
            per = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    return n, quota


_STDOUT = None


def quiet_stdout():
    """The contract is ONE JSON line on stdout: everything else a library
    prints there (gloo's "[Gloo] Rank 0 is connected ..." banner, a
    collective library's version line) goes to stderr.  File-descriptor
    level, because those writes come from C++."""
    global _STDOUT
    if _STDOUT is None:
        sys.stdout.flush()
        _STDOUT = os.dup(1)
        os.dup2(2, 1)


def emit(line):
    text = (json.dumps(line) + '\n').encode()
    sys.stdout.flush()
    os.write(_STDOUT if _STDOUT is not None else 1, text)


def main():
    args = parse()
    if not (args.gpus > 1 and 'WORLD_SIZE' not in os.environ):
        quiet_stdout()          # (the spawner's children each do their own)
    if args.config in ('2', '3'):
        args.config = int(args.config)
    if args.config == 'nws48':
        if args.dtype is None:
            args.dtype = 'f32'
        if args.steps is None:
            args.steps = 9
        emit(nws48_line(args))
        return
    if args.steps is None:
        # (a step of --config large is 528 pairs of ~1e5 rows each)
        args.steps = 5 if args.config == 'large' else 200
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))
    world = int(os.environ.get('WORLD_SIZE', 1))
    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    if world != args.gpus:
        raise SystemExit(f'--gpus {args.gpus} but WORLD_SIZE={world}')
    if args.gpr:
        if args.dtype is None:
            # (a fit wants gradients consistent with the objective to the
            # optimiser's line-search precision: double)
            args.dtype = 'f64' if args.fit else 'f32'
        line = gpr_step_line(args, world, rank, local_rank)
        if line is not None:
            try:
                import ctypes
                ctypes.CDLL(None).fflush(None)
            except Exception:
                pass
            emit(line)
        return
    if args.dtype is None:
        args.dtype = 'f64' if args.config == 3 else 'f32'
    sharded = world > 1 or args.sharded

    dist = torch = None
    host_collective = False
    if sharded:
        torch, dist, host_collective, local_rank = init_ranks(
            world, local_rank, args.share_devices)

    from graphdot_amd.hip import runtime
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.marginalized._sharded import ShardedStep

    real = np.float32 if args.dtype == 'f32' else np.float64
    # (sharded: launch merging is decided on the whole job list and applied
    # by every rank -- ShardPlan.merge_map -- so which solver variant a pair
    # runs on does not depend on the rank count)
    backend = HIPBackend(device=local_rank, real=real, record_iterations=True)
    graphs, knode, kedge, q, workload_name, (Fv, Fe) = workload(args)
    kernel = MarginalizedGraphKernel(knode, kedge, q=q, backend=backend,
                                     **({} if args.ftol is None
                                        else {'ftol': args.ftol}))
    n = len(graphs)
    i, j = np.triu_indices(n)
    job_t = np.dtype([('i', np.uint32), ('j', np.uint32)])
    all_jobs = np.column_stack((i, j)).astype(np.uint32).ravel().view(job_t)
    n_pairs = len(all_jobs)
    traits = kernel.traits(symmetric=True, eval_gradient=args.gradient)
    nJ = kernel.n_dims
    n_cols = 1 + (nJ if args.gradient else 0)
    starts = np.arange(n + 1, dtype=np.uint32)

    dgs = [backend._register_graph(g) for g in graphs]
    n_node = np.array([g.n_node for g in dgs], dtype=np.int64)
    n_nz = np.array([g.n_nz for g in dgs], dtype=np.int64)
    if sharded:
        step = ShardedStep(backend, graphs, knode, kedge, kernel.p, kernel.q,
                           kernel.eps, kernel.ftol, kernel.gtol, all_jobs,
                           starts, n, n, nJ, traits,
                           pipeline=args.pipeline)
        if world > 1:
            # the ranks time their shards and take the cuts again, as
            # `distributed_backend` does when it first builds a step
            from graphdot_amd.kernel.marginalized._sharded import \
                balance_by_measurement
            step, _ = balance_by_measurement(
                step, step.shard,
                lambda sp_: ShardedStep(
                    backend, graphs, knode, kedge, kernel.p, kernel.q,
                    kernel.eps, kernel.ftol, kernel.gtol, all_jobs, starts,
                    n, n, nJ, traits, pipeline=args.pipeline,
                    shard_plan=sp_),
                rounds=2)
        plan, local_jobs, shard = step.plan, step.local_jobs, step.shard
    else:
        plan = backend.prepare(graphs, knode, kedge, kernel.p, kernel.q,
                               kernel.eps, kernel.ftol, kernel.gtol, all_jobs,
                               starts, n, n, nJ, traits)
        step, local_jobs, shard = LocalStep(backend, plan), all_jobs, None

    nL = len(plan.launches)
    # one (start, stop) event pair per timed step and launch: durations are
    # read after the timed region, so a step never waits on the host
    ev_sets = [[(runtime.Event(), runtime.Event()) for _ in range(nL)]
               for _ in range(args.steps + 1)]

    def sync():
        step.synchronize()

    def barrier():
        if world > 1:
            dist.barrier()

    for w in range(args.warmup):
        step.enqueue(ev_sets[args.steps], serial=args.serial)
    sync()
    barrier()
    sync()
    t0 = time.perf_counter()
    for it in range(args.steps):
        step.enqueue(ev_sets[it], serial=args.serial)
    host_enqueue_ms = 1e3 * (time.perf_counter() - t0) / max(args.steps, 1)
    sync()
    barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device='cpu' if host_collective else 'cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # what the timed path computed in its last step (before the isolated
    # steps below launch the same plan again)
    if args.dump_outputs and rank == 0:
        vals, grads = step.download() if sharded else backend.collect(plan)
        out = {'K': vals.reshape(n, n, order='F')}
        if args.gradient:
            out['dK'] = grads.reshape(n, n, nJ, order='F')[
                :, :, np.asarray(kernel.active_theta_mask)]
        dump_outputs(args.dump_outputs, out, (i, j))
    # per-kernel durations inside the timed region: HIP events on the stream
    # each kernel ran on (the streams share the chip: durations overlap)
    kernel_ms = np.zeros(nL)
    for it in range(args.steps):
        for k in range(nL):
            kernel_ms[k] += ev_sets[it][k][0].elapsed_ms(ev_sets[it][k][1])
    kernel_ms /= max(args.steps, 1)

    # isolated durations: the same launches one after another on one stream
    isolated_ms = None
    if args.isolated_steps > 0:
        isolated_ms = np.zeros(nL)
        iso_ev = [(runtime.Event(), runtime.Event()) for _ in range(nL)]
        # (one untimed pass first: the launches of the timed region ran on the
        # solver streams, and the first launch of a kernel with a large
        # scratch frame on ANOTHER queue pays that queue's scratch allocation
        # -- 8 ms once for configuration 2's two-stage fallback, which as a
        # third of a three-pass average made it the "dominant" launch)
        step.enqueue(iso_ev, serial=True)
        sync()
        for it in range(args.isolated_steps):
            step.enqueue(iso_ev, serial=True)
            sync()
            for k in range(nL):
                isolated_ms[k] += iso_ev[k][0].elapsed_ms(iso_ev[k][1])
        isolated_ms /= args.isolated_steps
    barrier()
    # the three phases of a sharded step on every rank (device time): what a
    # first multi-GPU run is read by -- slowest shard + collective + reassembly
    phases = None
    if sharded:
        mine = step.phase_ms(steps=5)
        if world > 1:
            every = [None] * world
            dist.all_gather_object(every, mine)
        else:
            every = [mine]
        phases = {k: [float(e[k]) for e in every] for k in mine}
        phases['note'] = ('per rank, HIP events on the null stream of 5 '
                          'synchronised steps: solver launches of the rank\'s '
                          'shard | all-gather of the packed slabs | device '
                          'reassembly into the column-major matrix')
    barrier()

    if rank != 0:
        if sharded:
            dist.destroy_process_group()
        return

    ms_per_step = 1e3 * elapsed / args.steps
    value = n_pairs / (elapsed / args.steps)
    rsize = np.dtype(real).itemsize
    mult = 2 if args.gradient else 1

    # ---- results of this rank's launches on the host ---------------------------
    if sharded:
        vals, grads = step.download()
        K = vals.reshape(n, n, order='F')
        dK = grads.reshape(n, n, nJ, order='F') if args.gradient else None
    else:
        got, ggot = backend.collect(plan)
        K = got.reshape(n, n, order='F')
        dK = ggot.reshape(n, n, nJ, order='F') if args.gradient else None

    sharded_check = None
    if sharded:
        from oracle import mgk
        K_host = shard.assemble(
            step.gathered.cpu().numpy().reshape(world, -1)[
                :, :shard.capacity].ravel())
        assert np.array_equal(K, K_host), 'device and host reassembly differ'
        rng = np.random.default_rng(1)
        probe = rng.choice(n_pairs, size=min(3000, n_pairs), replace=False)
        batch = mgk.TensorProductBatch(graphs, knode, kedge)
        ref, _ = batch.run(i[probe], j[probe], q=q, real='f64', tol=1e-13)
        sharded_check = {
            'max_rel_diff_vs_oracle': float(np.max(np.abs(
                K[i[probe], j[probe]] / ref - 1))),
            'symmetric': bool(np.count_nonzero(K - K.T) == 0),
            'collective': 'gloo/host' if host_collective else 'nccl(RCCL)',
            'ranks': world}

    # ---- per-launch algorithmic work ---------------------------------------------
    arena = plan.keep[0]
    iters_all = backend.iterations(plan).astype(np.int64)
    sbytes = survey_bytes_per_graph(graphs)
    per_kernel, tot = [], dict(bytes=0, flops=0, lds=0, image=0)
    for k, L in enumerate(plan.launches):
        ids = plan.order_host[L['offset']:L['offset'] + L['count']]
        lj = local_jobs[ids]
        lji, ljj = lj['i'].astype(np.int64), lj['j'].astype(np.int64)
        it_ = iters_all[ids]
        ab = int(algorithmic_bytes(arena, lji, ljj, rsize, n_cols).sum())
        sb = int((sbytes[lji] + sbytes[ljj] + rsize * n_cols).sum())
        af = int(algorithmic_flops(n_node, n_nz, lji, ljj, it_, Fv, Fe).sum()
                 * mult)
        al = int(algorithmic_lds_reals(n_node, n_nz, lji, ljj, it_).sum()
                 * rsize * mult)
        tot['bytes'] += sb
        tot['image'] += ab
        tot['flops'] += af
        tot['lds'] += al
        per_kernel.append({
            'kernel': backend.kernel_name(L['variant'], plan.C, False,
                                          L.get('tab', False)),
            'pairs': int(L['count']), 'grid': int(L['grid']),
            'avg_ms': float(kernel_ms[k]),
            'isolated_ms': float(isolated_ms[k]) if isolated_ms is not None
            else None,
            'algorithmic_bytes': sb, 'image_bytes': ab,
            'algorithmic_flops': af,
            'algorithmic_lds_bytes': al,
            'mean_cg_iterations': float(it_.mean()) if len(it_) else 0.0})

    # ---- roofline of the dominant kernel (by isolated duration) ------------------
    basis = isolated_ms if isolated_ms is not None else kernel_ms
    dom = int(np.argmax(basis))
    D = per_kernel[dom]
    dur = basis[dom] * 1e-3
    roofline = {
        'bound': 'hbm', 'kernel': D['kernel'],
        'achieved': D['algorithmic_bytes'] / dur / 1e9, 'peak': HBM_PEAK_GBS,
        'unit': 'GB/s',
        'frac': D['algorithmic_bytes'] / dur / 1e9 / HBM_PEAK_GBS,
        'traffic': None,
        'achieved_is': 'ALGORITHMIC bytes / launch duration (SURVEY.md 8d: '
                       'both graphs in the reference\'s device layout -- '
                       '32 B header, node records + 4 B degrees, edge '
                       'records, 32 B per octile -- plus the result), not a '
                       'measured rate: see achieved_measured_GBs',
        'achieved_measured_GBs': None,
        'algorithmic_bytes_per_launch': D['algorithmic_bytes'],
        'image_bytes_per_launch': D['image_bytes'],
        'image_bytes_note': 'what this build actually stages per pair: its '
                            'own packed images (CSR + label-class ids, fp64 '
                            'attributes in the fp64 build) + 2 x 64 B headers',
        'pairs_per_launch': D['pairs'],
        'avg_launch_ms': float(basis[dom]),
        'duration_basis': 'isolated: the launch alone on one stream, HIP '
                          'events, after the timed region (agrees with '
                          'rocprofv3 --kernel-trace of `bench.py --serial`)'
                          if isolated_ms is not None else
                          'timed region (launch streams overlap)',
        'avg_launch_ms_in_timed_region': float(kernel_ms[dom]),
        'note': 'the solver is LDS/VALU-bound by design (CG vectors and the '
                'product-graph operator live in LDS/registers; graph images '
                'are L2-resident): see compute / lds and step_aggregate',
    }
    # measured HBM traffic of that kernel, if a PMC profile of this command
    # has been committed (scripts/profile.sh + scripts/summarize_profile.py)
    try:
        with open(os.path.join(ROOT, 'profiles', 'traffic.json')) as f:
            # profiled commands: config 3 in both arithmetics, its fp64
            # gradient step, configuration 2 in fp32 (scripts/profile_all.sh)
            key = {(3, False): args.dtype, (3, True): 'grad' + args.dtype[1:],
                   (2, False): 'c2' if args.dtype == 'f32' else 'c2f64',
                   ('large', False): 'large' if args.dtype == 'f32'
                   else 'large64'}[(args.config, bool(args.gradient))]
            tr = json.load(f)[key]['kernels'].get(roofline['kernel'])
        if tr and world == 1:
            # the image staging is a 16-byte-per-lane coalesced read, which
            # FETCH_SIZE counts at half its bytes on gfx950
            # (MI355X_MICROARCH.md, HBM): 2 x FETCH_SIZE + WRITE_SIZE
            roofline['traffic'] = tr['hbm_bytes_per_launch_fetch_x2']
            roofline['achieved_measured_GBs'] = \
                tr['hbm_bytes_per_launch_fetch_x2'] / dur / 1e9
            roofline['traffic_source'] = 'profiles/traffic.json (rocprofv3 ' \
                '2 x FETCH_SIZE + WRITE_SIZE, separate --pmc passes)'
            # the other duration basis: the average of the same kernel in the
            # committed rocprofv3 --kernel-trace --stats summary of this
            # command (`bench.py --serial`): HIP events run 5-9 % below it
            if tr.get('rocprof_avg_launch_ms'):
                rp = tr['rocprof_avg_launch_ms']
                roofline['rocprof_avg_launch_ms'] = rp
                roofline['frac_rocprof'] = D['algorithmic_bytes'] / (
                    rp * 1e-3) / 1e9 / HBM_PEAK_GBS
                roofline['rocprof_source'] = 'profiles/traffic.json ' \
                    '(kernel trace of the profiled run, another box)'
    except (OSError, KeyError, ValueError):
        pass
    peak_tf, lds_peak = VALU_PEAK_TF[args.dtype], LDS_PEAK_TBS[args.dtype]
    compute = {
        'bound': 'valu', 'achieved': D['algorithmic_flops'] / dur / 1e12,
        'peak': peak_tf, 'unit': 'TFLOP/s',
        'frac': D['algorithmic_flops'] / dur / 1e12 / peak_tf,
        'algorithmic_flops_per_launch': D['algorithmic_flops'],
        'mean_cg_iterations': D['mean_cg_iterations']}
    lds = {'bound': 'lds', 'achieved': D['algorithmic_lds_bytes'] / dur / 1e12,
           'peak': lds_peak, 'unit': 'TB/s',
           'frac': D['algorithmic_lds_bytes'] / dur / 1e12 / lds_peak,
           'algorithmic_lds_bytes_per_launch': D['algorithmic_lds_bytes']}
    # the whole step: every launch of this rank against the step time
    st = ms_per_step * 1e-3
    step_aggregate = {
        'ms_per_step': ms_per_step, 'launches': nL,
        'pairs': int(sum(d['pairs'] for d in per_kernel)),
        'hbm': {'algorithmic_bytes': tot['bytes'],
                'image_bytes': tot['image'],
                'achieved_GBs': tot['bytes'] / st / 1e9,
                'frac_step': tot['bytes'] / st / 1e9 / HBM_PEAK_GBS},
        'compute': {'algorithmic_flops': tot['flops'],
                    'achieved_TFLOPs': tot['flops'] / st / 1e12,
                    'frac_step': tot['flops'] / st / 1e12 / peak_tf},
        'lds': {'algorithmic_bytes': tot['lds'],
                'achieved_TBs': tot['lds'] / st / 1e12,
                'frac_step': tot['lds'] / st / 1e12 / lds_peak},
        'sum_isolated_ms': float(isolated_ms.sum())
        if isolated_ms is not None else None}

    # (before the CPU baseline: its OpenMP team keeps spinning on every core
    # for a while after its last parallel region)
    api = None
    if world == 1 and not args.no_api and not sharded:
        api = measure_api(graphs, knode, kedge, q, real, local_rank,
                          args.gradient, n_pairs)

    # ---- CPU baseline (oracle, 1 core, bounded sample), N = 1 only -----------
    cpu = accuracy = conv = None
    if world == 1 and not args.no_cpu_baseline:
        from oracle import mgk
        batch = mgk.TensorProductBatch(graphs, knode, kedge)
        rng = np.random.default_rng(0)

        def run(sel, omp=False):
            if args.gradient:
                v, g, _ = batch.run_gradient(i[sel], j[sel], q=q,
                                             real=args.dtype, omp=omp)
                return v, g
            v, _ = batch.run(i[sel], j[sel], q=q, real=args.dtype, omp=omp)
            return v, None

        # (pairs of the large-graph configuration take ~0.1 s each on one
        # core: a probe of 500 would be a minute)
        n_probe = 16 if args.config == 'large' else 500
        probe = rng.choice(n_pairs, size=min(n_probe, n_pairs), replace=False)
        t1 = time.perf_counter()
        run(probe)
        rate = len(probe) / (time.perf_counter() - t1)
        size = int(min(n_pairs, max(n_probe, rate * args.cpu_seconds)))
        sample = rng.choice(n_pairs, size=size, replace=False)
        t1 = time.perf_counter()
        ref, gref = run(sample)
        dt = time.perf_counter() - t1
        fn = 'mgk_gram_tp_grad_' if args.gradient else 'mgk_gram_tp_'
        cpu = {'value': size / dt, 'unit': 'graph-pairs/s', 'cores': 1,
               'kind': 'port',
               'sample': f'{size} uniformly sampled pairs of the same '
                         f'{n}-graph set, oracle/mgk_oracle.c '
                         f'{fn}{args.dtype}, 1 thread'}
        # same restatement, OpenMP over the pairs (one work buffer per
        # thread, graphs packed outside the timed call), on every CPU this
        # process may use: the affinity mask capped by the container's CPU
        # quota -- threads beyond the quota only time-share
        try:
            n_aff, quota = effective_cpus()
            ncore = max(1, min(n_aff, int(quota + 0.5) if quota else n_aff))
            os.environ['OMP_NUM_THREADS'] = str(ncore)  # (read at load time)
            run(probe, omp=True)                        # threads are up
            t1 = time.perf_counter()
            run(probe, omp=True)
            rate_all = len(probe) / (time.perf_counter() - t1)
            # a sample of >= 5 s: the pair list repeated if it is too short
            # (the short probe under-estimates the steady rate: grow until
            # the timed call is long enough)
            size_all, dt_all = int(max(2000 if args.config != 'large' else
                                       4 * ncore, rate_all * 6.0)), 0.0
            for _ in range(4):
                sample_all = rng.choice(n_pairs, size=min(size_all, n_pairs),
                                        replace=False)
                sample_all = np.resize(sample_all, size_all)
                t1 = time.perf_counter()
                run(sample_all, omp=True)
                dt_all = time.perf_counter() - t1
                if dt_all >= 5.0:
                    break
                size_all = int(size_all * 6.5 / max(dt_all, 1e-3))
            cpu['all_cores'] = {
                'value': size_all / dt_all, 'unit': 'graph-pairs/s',
                'cores': ncore, 'affinity_cpus': n_aff,
                'cgroup_cpu_quota': quota, 'seconds': dt_all,
                'parallel_efficiency': size_all / dt_all / cpu['value']
                / ncore,
                'sample': f'{size_all} pairs ({min(size_all, n_pairs)} '
                          'distinct), OpenMP dynamic schedule, one work '
                          'buffer per thread'}
        except Exception as e:                      # no libgomp etc.
            cpu['all_cores'] = {'error': str(e)}
        # the reference's own Python CPU path cannot travel to this host; its
        # rate was recorded in the build container (provenance in the file)
        if args.config == 3 and not args.gradient:
            try:
                with open(os.path.join(ROOT, 'profiles',
                                       'r01_reference_python_cpu.json')) as f:
                    rp = json.load(f)
                cpu['reference_python'] = {
                    k: rp[k] for k in ('value', 'unit', 'cores', 'what',
                                       'where')}
            except (OSError, KeyError, ValueError):
                pass
        # the sample doubles as an on-line parity check of the timed result
        cpu['max_rel_diff_vs_gpu'] = float(np.max(np.abs(
            K[i[sample], j[sample]] / ref - 1)))
        # ... and EVERY value of the timed result against the same
        # restatement converged to 1e-13 N in double (OpenMP over the pairs):
        # what the stopping tolerance of the timed solve is worth
        try:
            t1 = time.perf_counter()
            conv, _ = batch.run(i, j, q=q, real='f64', tol=1e-13, omp=True)
            accuracy = {
                'max_rel_err_vs_converged_oracle': float(np.max(np.abs(
                    K[i, j] / conv - 1))),
                'pairs_checked': int(n_pairs),
                'oracle': 'oracle/mgk_oracle.c mgk_gram_tp_f64, tol 1e-13, '
                          'all pairs of the timed result',
                'seconds': time.perf_counter() - t1}
        except Exception as e:
            accuracy = {'error': str(e)}
        if args.gradient:
            mask = np.ones(nJ, dtype=bool)
            dg = dK[i[sample], j[sample], :]
            scale = np.abs(gref).max(axis=0, keepdims=True)
            rt, at = (2e-3, 2e-5) if args.dtype == 'f32' else (1e-6, 1e-9)
            cpu['gradient_max_violation_of_elementwise_bound'] = float(np.max(
                np.abs(dg - gref) / (rt * np.abs(gref) + at * scale)))
            cpu['gradient_bound'] = f'|d| <= {rt} |ref| + {at} colscale'
            cpu['gradient_max_diff_over_colscale'] = float(np.max(
                np.abs(dg - gref) / scale))

    other = converged = None
    if world == 1 and not args.no_f32 and not args.gradient and not sharded:
        other, K_other = measure_other_arithmetic(
            'f32' if args.dtype == 'f64' else 'f64', graphs, knode, kedge, q,
            all_jobs, starts, n, max(args.steps // 2, 3), args.warmup,
            local_rank)
        if conv is not None:
            other['max_rel_err_vs_converged_oracle'] = float(np.max(np.abs(
                K_other[i, j] / conv - 1)))
        if args.dtype == 'f64' and kernel.ftol > 1e-13:
            # the double solver run to convergence: the tolerance the fp64
            # parity statement (rel 1e-9 against the dense oracle) is made at
            converged, K_conv = measure_other_arithmetic(
                'f64', graphs, knode, kedge, q, all_jobs, starts, n,
                max(args.steps // 2, 3), args.warmup, local_rank,
                ftol=1e-13, note='the same step with the double solver run '
                'to convergence (ftol = 1e-13)')
            if conv is not None:
                converged['max_rel_err_vs_converged_oracle'] = float(np.max(
                    np.abs(K_conv[i, j] / conv - 1)))

    line = {
        'metric': 'graph-pairs/sec (Gram matrix)', 'value': value,
        'unit': 'graph-pairs/s', 'n_gpus': world, 'steps': args.steps,
        'warmup': args.warmup, 'ms_per_step': ms_per_step,
        'higher_is_better': True, 'scaling': 'strong',
        'vs_baseline': None, 'dtype': args.dtype, 'data': 'synthetic',
        'config': {
            'workload': workload_name + ', '
            + ('fp64' if args.dtype == 'f64' else 'fp32')
            + (', value + gradient' if args.gradient else ''),
            'graphs': n, 'pairs': n_pairs,
            'parallelism': f'pair-sharded x{world}' if sharded else 'single',
            # the value solve stops at sqrt(rTr) < ftol N (reference
            # marginalized_kernel.h:449; 1e-8 is the reference's default --
            # in double arithmetic that is ~1e-7 relative accuracy, see
            # `accuracy` and `fp64_converged`); value + gradient solves at
            # the reference's fixed 1e-10 * 2N (:769)
            'ftol': kernel.ftol,
            'stopping_rule': 'sqrt(rTr) < ftol*N' if not args.gradient
            else 'sqrt(rTr) < 1e-10*2N (compute_duo)',
        },
        'mean_cg_iterations': float(iters_all.mean()) if len(iters_all)
        else None,
        'accuracy': accuracy, 'fp64_converged': converged,
        'roofline': roofline, 'compute': compute, 'lds': lds,
        'step_aggregate': step_aggregate, 'kernels': per_kernel,
        'cpu_baseline': cpu, 'api_inclusive': api,
        'sharded_check': sharded_check, 'phases_per_rank': phases,
        'other_arithmetic': other,
        # host time to issue one step (launches, events, collective)
        'host_enqueue_ms': host_enqueue_ms,
    }
    # RCCL announces itself on C stdio ("Librccl path : ..."), which a pipe
    # would deliver after Python's buffer: flush it so that the JSON line is
    # the last line of stdout
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    emit(line)
    if sharded:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
