#!/usr/bin/env python
"""Times of exact t-SNE after the kernel matrix is in place: the fused chain
(model/manifold/tsne.h: P recomputed per pair, two launches per step) against
the torch chain (`_tsne.*_torch`: the same arithmetic with the (n, n) matrix
of P stored) on the same device tensors, for RBF matrices of clustered points
in float and in double: the calibration, one step of the descent (the median
over repeats of the mean of `--steps` consecutive steps), one look, and a
whole `fit` from a random start, with the peak device memory each chain takes
on top of the matrix.  For scale, scikit-learn's `TSNE` on the host on the
same distances, `method='exact'` (up to `--sklearn-exact-most` samples: its
cost grows with n^2 per step) and `'barnes_hut'`, once each.  Host clocks
around work that ends in a device synchronise; medians of warm repeats, with
the smallest and the largest.

    python scripts/time_tsne.py [--sizes 1000 4000] [--repeats 7] [--fit-repeats R]
        [--steps 50] [--max-iter 1000] [--no-sklearn] [--out x.json]
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


def matrix(n, torch):
    """K = exp(-0.05 |a_i - a_j|^2) of n points around eight centres in six
    dimensions, float64 on the device."""
    rng = np.random.RandomState(n)
    c = 2 * rng.randn(8, 6)
    A = torch.from_numpy(c[rng.randint(0, 8, n)]
                         + 0.5 * rng.randn(n, 6)).cuda()
    sq = torch.cdist(A, A) ** 2
    return torch.exp(-0.05 * 0.5 * (sq + sq.T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[1000, 4000])
    ap.add_argument('--perplexity', type=float, default=30.0)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--fit-repeats', type=int,
                    help='repeats of a whole fit (default: --repeats)')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--max-iter', type=int, default=1000)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--sklearn-exact-most', type=int, default=1000)
    ap.add_argument('--out')
    args = ap.parse_args()
    fit_repeats = args.fit_repeats or args.repeats
    import torch
    from graphdot_amd.model.manifold import KernelTSNE, _tsne
    if not torch.cuda.is_available():
        raise SystemExit('time_tsne.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    out = {}
    for n in args.sizes:
        K64 = matrix(n, torch)
        lr = max(n / 12.0 / 4.0, 50.0)
        Y0 = 1e-4 * torch.randn((n, 2), dtype=torch.float64, device='cuda',
                                generator=torch.Generator(
                                    device='cuda').manual_seed(n))
        for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            K = K64.to(dtype)
            diag = K.diagonal().to(torch.float64).contiguous()
            row = {'n': n, 'parts': _tsne.parts_for(n),
                   'matrix_MiB': K.numel() * K.element_size() / 2 ** 20}
            cal = {}
            for chain, fn in (('fused', _tsne.calibrate),
                              ('torch', _tsne.calibrate_torch)):
                row[f'calibrate_{chain}_ms'], cal[chain] = timed(
                    lambda: fn(K, diag, args.perplexity), args.repeats, sync)
            row['calibrate_max_relative_difference'] = float(
                ((cal['fused'][0] - cal['torch'][0]).abs()
                 / cal['torch'][0]).max())
            beta, m, rZ, _, flag = cal['fused']
            P = _tsne._pairs_torch(K, diag, beta, m, rZ, Y0)[0]

            def steps(fused):
                state = _tsne.State(Y0)
                for _ in range(args.steps):
                    if fused:
                        _tsne.step(state, _tsne.forces(K, diag, beta, m, rZ,
                                                       state.Y),
                                   12.0, 0.5, lr)
                    else:
                        _tsne.step_torch(state, _tsne.forces_torch(
                            K, diag, beta, m, rZ, state.Y, P), 12.0, 0.5, lr)
                return state.Y

            def fit(fused):
                if fused:
                    return KernelTSNE('precomputed', init='random',
                                      perplexity=args.perplexity,
                                      max_iter=args.max_iter).fit(K)
                c = _tsne.calibrate_torch(K, diag, args.perplexity)
                return _tsne.descend(K, diag, *c[:3], c[4], Y0, args.max_iter,
                                     12.0, lr, 300, 1e-7, fused=False)

            res = {}
            for chain, fused in (('fused', True), ('torch', False)):
                t, res[chain] = timed(lambda: steps(fused), args.repeats,
                                      sync)
                row[f'step_{chain}_ms'] = [x / args.steps for x in t]
                row[f'look_{chain}_ms'] = timed(
                    lambda: (_tsne.objective if fused
                             else _tsne.objective_torch)(
                        K, diag, beta, m, rZ, Y0, 1.0)[0].cpu(),
                    args.repeats, sync)[0]
                row[f'fit_{chain}_ms'], f = timed(lambda: fit(fused),
                                                  fit_repeats, sync)
                row[f'fit_{chain}_kl'] = float(
                    f.kl_divergence_ if fused else f.kl)
                row[f'fit_{chain}_peak_extra_MiB'] = peak_extra(
                    lambda: fit(fused), torch)
            row['steps_max_difference'] = float(
                (res['fused'] - res['torch']).abs().max())
            out[f'{n}_{name}'] = row
            print(f'{n}_{name}', json.dumps(row), flush=True)
            del K, P, res, cal
        if not args.no_sklearn:
            from sklearn.manifold import TSNE
            d = K64.diagonal()
            D = torch.sqrt(torch.clamp_min(
                (d[:, None] + d[None, :]) - 2.0 * K64, 0.0))
            D.fill_diagonal_(0.0)
            D = D.cpu().numpy()
            row = {'n': n}
            for method in ('exact', 'barnes_hut'):
                if method == 'exact' and n > args.sklearn_exact_most:
                    continue
                t = time.perf_counter()
                sk = TSNE(perplexity=args.perplexity, method=method,
                          metric='precomputed', init='random',
                          max_iter=args.max_iter, random_state=0).fit(D)
                row[f'sklearn_{method}_ms'] = 1e3 * (time.perf_counter() - t)
                row[f'sklearn_{method}_kl'] = float(sk.kl_divergence_)
            out[f'{n}_sklearn'] = row
            print(f'{n}_sklearn', json.dumps(row), flush=True)
        del K64
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
