#!/usr/bin/env python
"""Times of KernelHDBSCAN after the kernel matrix is in place, on the matrices
of scripts/time_isomap.py (Gaussian-kernel matrices of random points of the
unit cube) in float and in double: the lists, the spanning tree in the HIP
chain (Boruvka rounds of model/clustering/mst.h on the implicit graph) and in
the torch chain (`_mst.*_torch`, which writes the (n, n) matrix of w2 once and
masks it every round) on the same device tensors, one row pass and one
hooking by themselves, the host part of a fit (hierarchy, condensing,
selection, labels), and a whole `fit`.  For scale, scikit-learn's
``HDBSCAN(metric='precomputed')`` on the host on the same distances, once.
Host clocks around work that ends in a device synchronise; medians of warm
repeats, with the smallest and the largest.

    python scripts/time_hdbscan.py [--sizes 1000 2000 4000] [--repeats 7]
        [--min-samples 5] [--min-cluster-size 5] [--no-sklearn] [--out x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from time_isomap import matrix, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*',
                    default=[1000, 2000, 4000])
    ap.add_argument('--min-samples', type=int, default=5)
    ap.add_argument('--min-cluster-size', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.clustering import KernelHDBSCAN, _mst
    from graphdot_amd.model.neighbors import device_lists
    if not torch.cuda.is_available():
        raise SystemExit('time_hdbscan.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    ms, size, reps = args.min_samples, args.min_cluster_size, args.repeats
    out = {}
    for n in args.sizes:
        K64 = matrix(n, torch)
        for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            K = K64.to(dtype)
            diag = K.diagonal().to(torch.float64).contiguous()
            row = {'n': n, 'min_samples': ms, 'min_cluster_size': size,
                   'parts': _mst.parts_for(n, n),
                   'matrix_MiB': K.numel() * K.element_size() / 2 ** 20}
            c2 = torch.zeros_like(diag)
            if ms > 1:
                row['lists_fused_ms'], ((d2, _, _), fused) = timed(
                    lambda: device_lists(K, diag, diag, ms - 1,
                                         exclude_self=True), reps, sync)
                assert fused
                c2 = d2[:, ms - 2].contiguous()
            comp = torch.arange(n, dtype=torch.int32, device='cuda')
            row['rows_fused_ms'], (w2, cand, _) = timed(
                lambda: _mst.rows(K, diag, c2, comp), reps, sync)
            row['hook_fused_ms'], (_, count) = timed(
                lambda: _mst.hook(w2, cand, comp,
                                  _mst.new_edges(n, K.device)), reps, sync)
            row['components_after_a_round'] = int(count.sum())
            row['tree_fused_ms'], tree = timed(
                lambda: _mst.spanning_tree(K, diag, c2, fused=True), reps,
                sync)
            row['tree_torch_ms'], plain = timed(
                lambda: _mst.spanning_tree(K, diag, c2, fused=False),
                min(reps, 3), sync)
            row['tree_equal'] = all(np.array_equal(x, y)
                                    for x, y in zip(tree[:3], plain[:3]))
            row['tied_edges'] = int(n - 1 - len(np.unique(tree[0])))
            row['fit_fused_ms'], model = timed(
                lambda: KernelHDBSCAN('precomputed', size, ms).fit(K), reps,
                sync)
            row['fit_phases_ms'] = {p: 1e3 * model.last_timing[p]
                                    for p in ('tree', 'host')}
            hosts = []
            for _ in range(reps):
                hosts.append(1e3 * KernelHDBSCAN(
                    'precomputed', size, ms).fit(K).last_timing['host'])
            row['host_ms'] = [float(np.median(hosts)), float(min(hosts)),
                              float(max(hosts))]
            row['n_clusters'] = model.n_clusters_
            row['noise'] = int((model.labels_ < 0).sum())
            out[f'{n}_{name}'] = row
            print(f'{n}_{name}', json.dumps(row), flush=True)
            del K, model
        if not args.no_sklearn:
            from sklearn.cluster import HDBSCAN
            d = K64.diagonal()
            D = torch.sqrt(torch.clamp_min(
                (d[:, None] + d[None, :]) - 2.0 * K64, 0.0))
            D.fill_diagonal_(0.0)
            D = D.cpu().numpy()
            t = time.perf_counter()
            sk = HDBSCAN(min_cluster_size=size, min_samples=ms,
                         metric='precomputed').fit(D)
            row = {'n': n, 'sklearn_fit_ms': 1e3 * (time.perf_counter() - t),
                   'n_clusters': int(sk.labels_.max()) + 1}
            out[f'{n}_sklearn'] = row
            print(f'{n}_sklearn', json.dumps(row), flush=True)
        del K64
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
