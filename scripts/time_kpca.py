#!/usr/bin/env python
"""Times of `KernelPCA` on N QM7-like graphs (tests/cases.py config 3,
normalised kernel, float backend): the eigen-solve of `fit` after the Gram
matrix is in place -- `eigen_solver='subspace'` (subspace.hip) against
`'dense'` (`torch.linalg.eigh` of the explicitly centred matrix) on the same
device matrix, for each k -- then one `fit_transform` of the graphs through
the public interface next to the Gram matrix alone.  Host clocks around work
that ends in a device synchronise; medians of warm repeats.

    python scripts/time_kpca.py [--n 1000] [--components 2,16] [--out x.json]
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
    ap.add_argument('--components', default='2,16')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.decomposition import KernelPCA
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    if not torch.cuda.is_available():
        raise SystemExit('time_kpca.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    G = np.asarray(list(cases.config3_graphs(args.n, seed=41)), dtype=object)
    knode, kedge, q = cases.config3_fit_kernels()
    kernel = Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, backend=HIPBackend(real=np.float32)))
    t_gram, Kd = timed(lambda: kernel.device_gram(G), 3, sync)
    # the matrix in place, as the model adopts it (a copy: the kernel's own
    # view dies at its next evaluation)
    K = torch.as_tensor(Kd, device='cuda').clone()
    out = {'n': args.n, 'gram_ms': t_gram, 'matrix': str(K.dtype),
           'strides': list(K.stride()), 'solve': []}
    for k in map(int, args.components.split(',')):
        row = {'k': k}
        for solver in ('subspace', 'dense'):
            pca = KernelPCA('precomputed', k, eigen_solver=solver)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                ms, _ = timed(lambda: pca.fit(K), args.repeats, sync)
            row[f'{solver}_ms'] = ms
            row[f'{solver}_ran'] = pca.eigen_solver_
            if solver == 'subspace':
                row['iterations'] = pca.n_iter_
            row[f'{solver}_eigenvalues'] = pca.eigenvalues_[:2].tolist()
        out['solve'].append(row)
        print(json.dumps(row), flush=True)
    k = int(args.components.split(',')[0])
    pca = KernelPCA(kernel, k)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ms, xy = timed(lambda: pca.fit_transform(G), 3, sync)
    out['fit_transform'] = {'k': k, 'ms': ms, 'solver': pca.eigen_solver_,
                            'iterations': pca.n_iter_,
                            'timing': pca.last_timing, 'shape': xy.shape}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
