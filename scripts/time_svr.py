#!/usr/bin/env python
"""Times of `KernelSVR` on N QM7-like graphs (tests/cases.py config 3,
normalised kernel, float backend) after the Gram matrix is in place: (a) a
`fit`, (b) `cross_val_score` with 8 values of C x 4 of epsilon x 5 folds (160
problems) -- each on the fused path (svr.hip) and through `smo2_torch` on the
same device matrix, in microseconds per SMO step, and beside them
scikit-learn's ``SVR(kernel='precomputed')`` on the downloaded matrix on the
host; and a `fit` of `KernelOneClassSVM` the same three ways.  Host clocks
around work that ends in a device synchronise; medians of warm repeats.

    python scripts/time_svr.py [--n 1000] [--repeats 7] [--out x.json]
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
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--torch-repeats', type=int, default=1)
    ap.add_argument('--C', type=float, default=10.0)
    ap.add_argument('--epsilon', type=float, default=0.1)
    ap.add_argument('--nu', type=float, default=0.2)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.svm import KernelOneClassSVM, KernelSVR, _smo
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    if not torch.cuda.is_available():
        raise SystemExit('time_svr.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    n = args.n
    G = np.asarray(list(cases.config3_graphs(n, seed=41)), dtype=object)
    knode, kedge, q = cases.config3_fit_kernels()
    kernel = Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, backend=HIPBackend(real=np.float32)))
    t_gram, Kd = timed(lambda: kernel.device_gram(G), 3, sync)
    # the matrix in place, as the model adopts it (a copy: the kernel's own
    # view dies at its next evaluation)
    K = torch.as_tensor(Kd, device='cuda').clone()
    Kh = K.cpu().numpy().astype(np.float64)
    # a target the kernel can learn: the number of atoms, standardised, with
    # a little noise
    size = np.array([float(len(g.nodes)) for g in G])
    z = (size - size.mean()) / size.std() \
        + 0.1 * np.random.default_rng(0).normal(size=n)
    Cs = [0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    es = [0.025, 0.05, 0.1, 0.2]
    out = {'n': n, 'gram_ms': t_gram, 'matrix': str(K.dtype),
           'strides': list(K.stride()), 'C': args.C, 'epsilon': args.epsilon,
           'nu': args.nu}

    def through_torch(fn):
        """`fn` with the fused paths switched off: the torch restatements on
        the same device matrix."""
        saved = _smo.NMAX, _smo.NMAX2
        _smo.NMAX = _smo.NMAX2 = 0
        try:
            return fn()
        finally:
            _smo.NMAX, _smo.NMAX2 = saved

    def measure(name, run, steps, sk):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ms, m = timed(run, args.repeats, sync)
            s = steps(m)
            # (steps: those of all problems of the batch, added up)
            row = {'fused_ms': ms, 'steps': s,
                   'fused_us_per_step': 1e3 * ms / max(s, 1),
                   'slices': m.last_timing['slices']}
            assert m.last_timing['fused']
            ms_t, mt = through_torch(
                lambda: timed(run, args.torch_repeats, sync))
            assert not mt.last_timing['fused']
            row.update(torch_ms=ms_t, torch_steps=steps(mt),
                       torch_us_per_step=1e3 * ms_t / max(steps(mt), 1))
            if sk is not None:
                row['sklearn_ms'] = timed(sk, 3, lambda: None)[0]
        out[name] = row
        print(name, json.dumps(row), flush=True)

    def fit():
        return KernelSVR('precomputed', C=args.C,
                         epsilon=args.epsilon).fit(K, z)

    def cv():
        m = KernelSVR('precomputed')
        m.scores = m.cross_val_score(K, z, Cs, es, cv=5)
        return m

    def one():
        return KernelOneClassSVM('precomputed', nu=args.nu).fit(K)

    try:
        from sklearn.svm import SVR, OneClassSVM
        from sklearn.model_selection import KFold, cross_val_score

        def sk_fit():
            return SVR(C=args.C, epsilon=args.epsilon, kernel='precomputed',
                       cache_size=1000).fit(Kh, z)

        def sk_cv():
            folds = KFold(5, shuffle=True, random_state=0)
            return [cross_val_score(SVR(C=C, epsilon=e, kernel='precomputed',
                                        cache_size=1000), Kh, z, cv=folds)
                    for C in Cs for e in es]

        def sk_one():
            return OneClassSVM(nu=args.nu, kernel='precomputed',
                               cache_size=1000).fit(Kh)
    except ImportError:
        sk_fit = sk_cv = sk_one = None
    measure('fit', fit, lambda m: m.n_iter_, sk_fit)
    measure('cross_val_8x4x5', cv, lambda m: m.last_timing['steps'], sk_cv)
    measure('one_class_fit', one, lambda m: m.n_iter_, sk_one)
    m = KernelSVR(kernel, C=args.C, epsilon=args.epsilon)
    ms, _ = timed(lambda: m.fit(G, z), 3, sync)
    out['fit_graphs'] = {'ms': ms, 'timing': m.last_timing}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
