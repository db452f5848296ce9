#!/usr/bin/env python
"""Wall time of the active-learning selectors (model/active_learning) on a
kernel matrix in device memory, against the reference-style greedy loops on
the host: `DeterminantMaximizer` casts K to float32 and makes two N^2 passes
per pick (K @ v, K -= outer); `VarianceMinimizer` forms
K[i:, :i] @ inv @ K[:i, i:] again at every pick and grows the inverse by a
rank-one block update.

K: the RBF kernel of N random 3-D points, built on the GPU in fp32 and fp64.
Device times are whole calls of the selectors on the CUDA tensor (launches +
the one download), after one warm-up call.  Host loops: each is run for at
most --host-budget seconds; when it stops early its total is EXTRAPOLATED
from the steps it made (constant per-step cost for the determinant loop,
per-step cost linear in the step for the variance loop) and marked so.  The
host variance loop is not run at N = 30 000 (two float64 copies of K,
14 GB).

    python scripts/time_active_learning.py [--out profiles/x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_determinant(K, n, budget):
    K = K.astype(np.float32)
    chosen, times = [], []
    t0 = time.perf_counter()
    for _ in range(n):
        t = time.perf_counter()
        L = np.sum(K**2, axis=1)
        L[chosen] = -np.inf
        i = int(np.argmax(L))
        chosen.append(i)
        v = K[i, :] / np.linalg.norm(K[i, :])
        K -= np.outer(K @ v, v)
        times.append(time.perf_counter() - t)
        if time.perf_counter() - t0 > budget:
            break
    steps = len(times)
    total = float(np.mean(times) * n) if steps < n else float(sum(times))
    return dict(steps_measured=steps, total_s=total,
                extrapolated=steps < n)


def host_variance(K, n, alpha, budget):
    K = np.array(K, dtype=np.float64)
    K.flat[::len(K) + 1] += alpha
    index = np.arange(len(K))
    inv = np.zeros((0, 0))
    times = []
    t0 = time.perf_counter()
    for i in range(n):
        t = time.perf_counter()
        posterior = K[i:, i:] - K[i:, :i] @ inv @ K[:i, i:]
        j = i + int(np.argmax(np.sum(posterior, axis=1)))
        index[[i, j]] = index[[j, i]]
        K[[i, j], :] = K[[j, i], :]
        K[:, [i, j]] = K[:, [j, i]]
        if i < n - 1:
            w = inv @ K[:i, i]
            schur = K[i, i] - K[:i, i] @ w
            B = np.empty((i + 1, i + 1))
            B[:-1, :-1] = inv + np.outer(w, w) / schur
            B[-1, :-1] = B[:-1, -1] = -w / schur
            B[-1, -1] = 1 / schur
            inv = B
        times.append(time.perf_counter() - t)
        if time.perf_counter() - t0 > budget:
            break
    steps = len(times)
    if steps < n:
        # per-step cost a + b i fitted to the measured steps, summed to n
        if steps >= 3:
            b, a = np.polyfit(np.arange(steps), times, 1)
        else:
            a, b = float(np.mean(times)), 0.0
        total = float(sum(max(a + b * i, times[-1]) for i in range(n)))
    else:
        total = float(sum(times))
    return dict(steps_measured=steps, total_s=total, extrapolated=steps < n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='2000,10000,30000')
    ap.add_argument('--picks', default='100,500')
    ap.add_argument('--host-budget', type=float, default=8.0)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.active_learning import (
        DeterminantMaximizer, VarianceMinimizer)
    sizes = [int(s) for s in args.sizes.split(',')]
    picks = [int(s) for s in args.picks.split(',')]
    rows = []
    dm = DeterminantMaximizer('precomputed', device='cuda')
    vm = VarianceMinimizer('precomputed', device='cuda')
    for N in sizes:
        g = torch.Generator(device='cuda').manual_seed(N)
        X = torch.rand((N, 3), generator=g, device='cuda',
                       dtype=torch.float64) * 2 - 1
        K64 = torch.exp(-0.5 * torch.cdist(X, X)**2 / 0.3**2)
        for dtype, K in (('f64', K64), ('f32', K64.float())):
            for name, sel in (('determinant', dm), ('variance', vm)):
                sel(K, 5)                                     # warm-up
                for n in picks:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    out = sel(K, n)
                    dt = time.perf_counter() - t
                    assert len(set(out)) == n
                    row = dict(method=name, N=N, n=n, K=dtype,
                               where='device', total_s=dt,
                               per_pick_us=1e6 * dt / n)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            if dtype == 'f32':
                del K
        if not args.no_host:
            Kh = K64.cpu().numpy()
            for n in picks:
                r = host_determinant(Kh, n, args.host_budget)
                r.update(method='determinant', N=N, n=n, K='f32 (cast)',
                         where='host numpy, reference-style')
                rows.append(r)
                print(json.dumps(r), flush=True)
                if N <= 10000:
                    r = host_variance(Kh, n, 1e-6, args.host_budget)
                    r.update(method='variance', N=N, n=n, K='f64',
                             where='host numpy, reference-style')
                    rows.append(r)
                    print(json.dumps(r), flush=True)
            del Kh
        del K64
        torch.cuda.empty_cache()
    meta = dict(device=torch.cuda.get_device_name(0),
                host_threads=os.environ.get('OMP_NUM_THREADS'),
                kernel='RBF, length 0.3, N uniform 3-D points')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(dict(meta=meta, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
