#!/usr/bin/env python
"""Times of the sums of the kernel two-sample test after the Gram matrix of
the pooled sample is in place: the fused chain (mmd.hip: three launches, the
matrix read as it lies) against the torch chain (`_mmd.forms_torch`) on the
same device tensors, for precomputed RBF matrices of N points in float and in
double and B permutations, with the peak device memory each chain takes on top
of its inputs; and one whole `fit` of `KernelTwoSampleTest` on QM7-like graphs
(tests/cases.py config 3) split into halves on the HIP backend, kernel
evaluation included.  Host clocks around work that ends in a device
synchronise; medians of warm repeats, with the smallest and the largest.

    python scripts/time_two_sample.py [--sizes 1000 2000 4000] [--b 9999]
        [--graphs 1000] [--repeats 7] [--out x.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


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
    ap.add_argument('--sizes', type=int, nargs='*', default=[1000, 2000, 4000])
    ap.add_argument('--b', type=int, default=9999)
    ap.add_argument('--graphs', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.two_sample import KernelTwoSampleTest, _mmd
    if not torch.cuda.is_available():
        raise SystemExit('time_two_sample.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    out = {'b': args.b}
    for n in args.sizes:
        rng = np.random.default_rng(n)
        X = rng.normal(size=(n, 4))
        X[: n // 2] += 0.1                     # (a slight shift of the first half)
        K64 = np.exp(-0.05 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
        z0 = np.arange(n) < n // 2
        Z = torch.from_numpy(_mmd.splits(z0, args.b, seed=0)).cuda()
        s = torch.from_numpy(np.where(z0, 1.0 / (n // 2),
                                      -1.0 / (n - n // 2))).cuda()
        for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            K = torch.from_numpy(K64).to(dtype).cuda()
            row = {'n': n, 'rows': int(Z.shape[0]), 'grid': _mmd.grid(n, len(Z))}
            res = {}
            for chain, fn in (('fused', _mmd.forms),
                              ('torch', _mmd.forms_torch)):
                row[f'{chain}_ms'], res[chain] = timed(
                    lambda: fn(K, Z, s), args.repeats, sync)
                row[f'{chain}_peak_extra_MiB'] = peak_extra(
                    lambda: fn(K, Z, s), torch)
            a, b = res['fused'][0], res['torch'][0]
            row['max_relative_difference'] = float(
                ((a - b).abs() / b.abs().clamp_min(1e-300)).max())
            row['fma_per_s_fused'] = 0.5 * n * n * len(Z) \
                / (1e-3 * row['fused_ms'][0])
            out[f'n{n}_{name}'] = row
            print(f'n{n}_{name}', json.dumps(row), flush=True)
            del K, res, a, b
    if args.graphs:
        import cases
        from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
        from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
        from graphdot_amd.kernel.fix import Normalization
        G = np.asarray(list(cases.config3_graphs(args.graphs)), dtype=object)
        knode, kedge, q = cases.config3_fit_kernels()
        kernel = Normalization(MarginalizedGraphKernel(
            knode, kedge, q=q, q_bounds=(1e-3, 0.5),
            backend=HIPBackend(real=np.float32)))
        half = args.graphs // 2
        fits = []
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for _ in range(3):
                test = KernelTwoSampleTest(kernel, n_permutations=args.b,
                                           random_state=0)
                t = time.perf_counter()
                test.fit(G[:half], G[half:])
                fits.append(1e3 * (time.perf_counter() - t))
        fit = {'graphs': args.graphs, 'ms': fits,
               'statistic': test.statistic_, 'pvalue': test.pvalue_,
               'last_timing': test.last_timing}
        out['fit'] = fit
        print('fit', json.dumps(fit), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
