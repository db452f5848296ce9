#!/usr/bin/env python
"""Times of the nearest-neighbour search after the kernel matrix is in place:
the fused chain (csrc/device/knn.h: `knn_topk_*` and, where the columns are
split, `knn_merge`; the matrix read as it lies) against the torch chain
(`_knn.topk_torch`: the matrix of d2 in double and a stable sort) on the same
device tensors, for (b, n) matrices of random entries in float and in double,
row-major, at k = 5 and k = 64, with the peak device memory each chain takes
on top of its inputs; and one whole `fit` of `KernelLocalOutlierFactor` on a
precomputed RBF matrix on the device against the same steps through torch.
Host clocks around work that ends in a device synchronise; medians of warm
repeats, with the smallest and the largest.

    python scripts/time_neighbors.py [--shapes 1000x1000 1000x20000 64x100000]
        [--ks 5 64] [--parts P ...] [--lof 1000] [--repeats 7] [--out x.json]

--parts: time the fused search with these splits of the columns as well (the
same lists with every one), next to the split `_knn.parts_for` chooses.
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


def peak_extra(fn, torch):
    """Peak device memory in MiB above what is allocated before the call."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='*',
                    default=['1000x1000', '1000x20000', '64x100000'])
    ap.add_argument('--ks', type=int, nargs='*', default=[5, 64])
    ap.add_argument('--parts', type=int, nargs='*', default=[])
    ap.add_argument('--lof', type=int, default=1000)
    ap.add_argument('--lof-k', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.neighbors import KernelLocalOutlierFactor, _knn
    if not torch.cuda.is_available():
        raise SystemExit('time_neighbors.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    out = {}
    for shape in args.shapes:
        b, n = (int(x) for x in shape.split('x'))
        g = torch.Generator(device='cuda').manual_seed(b + n)
        K64 = torch.randn((b, n), dtype=torch.float64, device='cuda',
                          generator=g)
        dq = 3.0 + torch.rand(b, dtype=torch.float64, device='cuda',
                              generator=g)
        dt = 3.0 + torch.rand(n, dtype=torch.float64, device='cuda',
                              generator=g)
        for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            K = K64.to(dtype)
            for k in args.ks:
                row = {'b': b, 'n': n, 'k': k, 'parts': _knn.parts_for(b, n),
                       'matrix_MiB': K.numel() * K.element_size() / 2 ** 20}
                res = {}
                for chain, fn in (('fused', _knn.topk),
                                  ('torch', _knn.topk_torch)):
                    row[f'{chain}_ms'], res[chain] = timed(
                        lambda: fn(K, dq, dt, k), args.repeats, sync)
                    row[f'{chain}_peak_extra_MiB'] = peak_extra(
                        lambda: fn(K, dq, dt, k), torch)
                for p in args.parts:
                    row[f'fused_parts{p}_ms'] = timed(
                        lambda: _knn.topk(K, dq, dt, k, parts=p),
                        args.repeats, sync)[0]
                row['same_lists'] = bool(
                    torch.equal(res['fused'][1], res['torch'][1])
                    and torch.equal(res['fused'][0], res['torch'][0]))
                row['GB_per_s_fused'] = K.numel() * K.element_size() \
                    / (1e6 * row['fused_ms'][0])
                out[f'{shape}_{name}_k{k}'] = row
                print(f'{shape}_{name}_k{k}', json.dumps(row), flush=True)
                del res
            del K
        del K64
    if args.lof:
        n, k = args.lof, args.lof_k
        rng = np.random.default_rng(n)
        X = rng.normal(size=(n, 4))
        K = torch.from_numpy(np.exp(
            -0.05 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))).cuda()

        def fit():
            return KernelLocalOutlierFactor('precomputed', k).fit(
                K).negative_outlier_factor_

        def fit_torch():
            d = K.diagonal().to(torch.float64).clone()
            d2, idx, flag = _knn.topk_torch(K, d, d, k, exclude_self=True)
            kdist = torch.sqrt(d2[:, k - 1]).contiguous()
            own = _knn.lrd_torch(d2, idx, kdist)
            lof = _knn.ratio_torch(idx, own, own)
            return -torch.cat((lof, flag.to(lof.dtype))).cpu().numpy()[:-1]

        row = {'n': n, 'k': k}
        res = {}
        for chain, fn in (('fused', fit), ('torch', fit_torch)):
            row[f'{chain}_ms'], res[chain] = timed(fn, args.repeats, sync)
            row[f'{chain}_peak_extra_MiB'] = peak_extra(fn, torch)
        row['max_relative_difference'] = float(np.max(
            np.abs(res['fused'] - res['torch']) / np.abs(res['torch'])))
        out['lof_fit'] = row
        print('lof_fit', json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
