#!/usr/bin/env python
"""Times of `KernelKMeans` on N QM7-like graphs (tests/cases.py config 3,
normalised kernel, float backend) after the Gram matrix is in place: the whole
`fit` (k-means++ seeding, all restarts, medoids) and the time per round of
the HIP chain (lloyd.hip: accumulate, assign, reduce) against the ``*_torch``
chain on the same device matrix and the same labels, then one `fit` of the
graphs through the public interface next to the Gram matrix alone.  Host
clocks around work that ends in a device synchronise; medians of warm repeats.

    python scripts/time_kkmeans.py [--n 1000] [--clusters 8] [--out x.json]
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
    ts = []
    for _ in range(repeats + 1):
        sync()
        t = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts[1:])) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000)
    ap.add_argument('--clusters', type=int, default=8)
    ap.add_argument('--n-init', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.clustering import KernelKMeans, _lloyd
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    if not torch.cuda.is_available():
        raise SystemExit('time_kkmeans.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    k, R = args.clusters, args.n_init
    G = np.asarray(list(cases.config3_graphs(args.n, seed=41)), dtype=object)
    knode, kedge, q = cases.config3_fit_kernels()
    kernel = Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, backend=HIPBackend(real=np.float32)))
    t_gram, Kd = timed(lambda: kernel.device_gram(G), 3, sync)
    # the matrix in place, as the model adopts it (a copy: the kernel's own
    # view dies at its next evaluation)
    K = torch.as_tensor(Kd, device='cuda').clone()
    out = {'n': args.n, 'k': k, 'n_init': R, 'gram_ms': t_gram,
           'matrix': str(K.dtype), 'strides': list(K.stride())}
    km = KernelKMeans('precomputed', k, n_init=R)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ms, _ = timed(lambda: km.fit(K), args.repeats, sync)
    out['fit'] = {'ms': ms, 'rounds': km.last_timing['rounds'],
                  'n_iter': km.n_iter_, 'inertia': km.inertia_,
                  'sizes': km.cluster_sizes_.tolist()}
    print(json.dumps(out['fit']), flush=True)

    # the rounds alone: both chains from the same start labels, no look
    u = np.random.default_rng(0).random((R, k))
    first = _lloyd.seed(K, k, 'k-means++', u)[1]
    K64 = K.to(torch.float64)         # (as `iterate` hands it to the torch chain)

    def chain(acc, asg, red, M):
        def run():
            lab = [first.clone(), torch.empty_like(first)]
            info = torch.zeros((R, 4), dtype=torch.float64, device='cuda')
            for it in range(1, args.rounds + 1):
                S, part = acc(M, lab[(it - 1) % 2], k)
                lab[it % 2], shares = asg(M, lab[(it - 1) % 2], S, part)
                red(shares, info, it)
            return lab[args.rounds % 2], info
        return run
    hip = chain(_lloyd.accumulate, _lloyd.assign, _lloyd.reduce, K)
    ref = chain(_lloyd.accumulate_torch, _lloyd.assign_torch,
                _lloyd.reduce_torch, K64)
    ms_hip, (lab_h, info_h) = timed(hip, args.repeats, sync)
    ms_ref, (lab_t, info_t) = timed(ref, args.repeats, sync)
    out['round'] = {
        'rounds': args.rounds, 'hip_ms': ms_hip / args.rounds,
        'torch_ms': ms_ref / args.rounds,
        'same_labels': bool(torch.equal(lab_h, lab_t)),
        'inertia_difference': float((info_h[:, 1] - info_t[:, 1]).abs().max()
                                    / info_t[:, 1].abs().max())}
    print(json.dumps(out['round']), flush=True)
    km = KernelKMeans(kernel, k, n_init=R)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ms, _ = timed(lambda: km.fit(G), 3, sync)
    out['fit_graphs'] = {'ms': ms, 'timing': km.last_timing}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
