#!/usr/bin/env python
"""Times of KernelIsomap after the kernel matrix is in place: the fused chain
(csrc/device/knn.h for the lists, model/manifold/geodesic.h for the graph, the
blocked Floyd-Warshall rounds and B) against the torch chain
(`_geodesic.*_torch`: a mask for the graph, n broadcast passes over the (n, n)
matrix for the paths) on the same device tensors, for Gaussian-kernel matrices
of random points of the unit cube in float and in double: the lists, the graph,
the shortest paths, `finish`, the dense eigenpairs of `KernelPCA` on B, and a
whole `fit`.  For scale, scikit-learn's ``Isomap(metric='precomputed',
eigen_solver='dense')`` on the host on the same distances, once.  Host clocks
around work that ends in a device synchronise; medians of warm repeats, with
the smallest and the largest.

    python scripts/time_isomap.py [--sizes 1000 2000 4000] [--repeats 7]
        [--n-neighbors 10] [--no-sklearn] [--no-torch-paths-above N] [--out x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats, sync):
    """(median, min, max) in ms of `repeats` warm calls, and the last
    result."""
    ts = []
    for _ in range(repeats + 1):
        sync()
        t = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t)
    ts = 1e3 * np.array(ts[1:])
    return [float(np.median(ts)), float(ts.min()), float(ts.max())], out


def matrix(n, torch):
    """K = exp(-|a_i - a_j|^2 / 2) of n random points of the unit cube,
    float64 on the device."""
    A = torch.from_numpy(np.random.RandomState(n).rand(n, 3)).cuda()
    sq = torch.cdist(A, A) ** 2
    return torch.exp(-0.25 * (sq + sq.T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*',
                    default=[1000, 2000, 4000])
    ap.add_argument('--n-neighbors', type=int, default=10)
    ap.add_argument('--n-components', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--no-torch-paths-above', type=int, default=4000,
                    help='largest n whose paths the torch chain is timed on')
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.decomposition import KernelPCA
    from graphdot_amd.model.manifold import KernelIsomap, _geodesic
    from graphdot_amd.model.neighbors import device_lists
    if not torch.cuda.is_available():
        raise SystemExit('time_isomap.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    k, c, reps = args.n_neighbors, args.n_components, args.repeats
    out = {}
    for n in args.sizes:
        K64 = matrix(n, torch)
        for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            K = K64.to(dtype)
            diag = K.diagonal().to(torch.float64).contiguous()
            row = {'n': n, 'n_neighbors': k, 'rounds': _geodesic.rounds(n),
                   'matrix_MiB': K.numel() * K.element_size() / 2 ** 20}
            row['lists_fused_ms'], ((_, idx, _), fused) = timed(
                lambda: device_lists(K, diag, diag, k, exclude_self=True),
                reps, sync)
            assert fused
            row['graph_fused_ms'], W = timed(
                lambda: _geodesic.graph(K, diag, idx), reps, sync)
            row['graph_torch_ms'], Wt = timed(
                lambda: _geodesic.graph_torch(K, diag, idx), reps, sync)
            row['graph_equal'] = bool(torch.equal(W, Wt))
            del Wt
            row['paths_fused_ms'], G = timed(
                lambda: _geodesic.shortest_paths(W.clone()), reps, sync)
            row['clone_ms'] = timed(lambda: W.clone(), reps, sync)[0]
            if n <= args.no_torch_paths_above:
                row['paths_torch_ms'], Gt = timed(
                    lambda: _geodesic.shortest_paths_torch(W),
                    min(reps, 3), sync)
                row['paths_max_relative_difference'] = float(
                    ((G - Gt).abs() / Gt.clamp_min(1e-300)).max())
                del Gt
            row['finish_fused_ms'], (B, _, count) = timed(
                lambda: _geodesic.finish(G), reps, sync)
            row['finish_torch_ms'] = timed(
                lambda: _geodesic.finish_torch(G), reps, sync)[0]
            row['components'] = int(count.sum())
            row['eigenpairs_ms'] = timed(
                lambda: KernelPCA('precomputed', c, eigen_solver='dense',
                                  device='cuda').fit(B), reps, sync)[0]
            row['fit_fused_ms'], model = timed(
                lambda: KernelIsomap('precomputed', k, c).fit(K), reps, sync)
            row['fit_phases_ms'] = {p: 1e3 * model.last_timing[p]
                                    for p in ('paths', 'linalg')}
            row['eigenvalues'] = [float(w) for w in model.eigenvalues_]
            out[f'{n}_{name}'] = row
            print(f'{n}_{name}', json.dumps(row), flush=True)
            del K, W, G, B, model
        if not args.no_sklearn:
            from sklearn.manifold import Isomap
            d = K64.diagonal()
            D = torch.sqrt(torch.clamp_min(
                (d[:, None] + d[None, :]) - 2.0 * K64, 0.0))
            D.fill_diagonal_(0.0)
            D = D.cpu().numpy()
            t = time.perf_counter()
            sk = Isomap(n_neighbors=k, n_components=c, metric='precomputed',
                        eigen_solver='dense').fit(D)
            row = {'n': n, 'sklearn_fit_ms': 1e3 * (time.perf_counter() - t),
                   'reconstruction_error': float(sk.reconstruction_error())}
            out[f'{n}_sklearn'] = row
            print(f'{n}_sklearn', json.dumps(row), flush=True)
        del K64
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
