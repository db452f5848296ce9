#!/usr/bin/env python
"""Times of `KernelSVC` on N QM7-like graphs (tests/cases.py config 3,
normalised kernel, float backend) after the Gram matrix is in place: (a) a
binary `fit`, (b) a 10-class `fit` (45 one-vs-one problems), (c)
`cross_val_score` with 8 values of C x 5 folds -- each on the fused path
(smo.hip) and through `smo_torch` on the same device matrix, in microseconds
per SMO step, and beside them scikit-learn's ``SVC(kernel='precomputed')`` on
the downloaded matrix on the host.  Host clocks around work that ends in a
device synchronise; medians of warm repeats.

    python scripts/time_svc.py [--n 1000] [--repeats 7] [--out x.json]
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
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.svm import KernelSVC, _smo
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    if not torch.cuda.is_available():
        raise SystemExit('time_svc.py measures on a GPU; none found')
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
    # labels the kernel can learn: the number of atoms, in 2 and in 10 bins
    size = np.array([len(g.nodes) for g in G]) \
        + np.random.default_rng(0).random(n)
    lab2 = np.searchsorted(np.quantile(size, [0.5]), size)
    lab10 = np.searchsorted(np.quantile(size, np.arange(1, 10) / 10), size)
    Cs = [0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    out = {'n': n, 'gram_ms': t_gram, 'matrix': str(K.dtype),
           'strides': list(K.stride()), 'C': args.C}

    def through_torch(fn):
        """`fn` with the fused path switched off: `smo_torch` on the same
        device matrix."""
        nmax, _smo.NMAX = _smo.NMAX, 0
        try:
            return fn()
        finally:
            _smo.NMAX = nmax

    def measure(name, run, steps, sk):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ms, m = timed(run, args.repeats, sync)
            s = steps(m)
            # (steps: those of all problems of the batch, added up)
            row = {'fused_ms': ms, 'steps': s,
                   'fused_us_per_step': 1e3 * ms / s,
                   'slices': m.last_timing['slices']}
            assert m.last_timing['fused']
            ms_t, mt = through_torch(
                lambda: timed(run, args.torch_repeats, sync))
            assert not mt.last_timing['fused']
            row.update(torch_ms=ms_t, torch_steps=steps(mt),
                       torch_us_per_step=1e3 * ms_t / steps(mt))
            if sk is not None:
                row['sklearn_ms'] = timed(sk, 3, lambda: None)[0]
        out[name] = row
        print(name, json.dumps(row), flush=True)

    def fit(lab):
        return lambda: KernelSVC('precomputed', C=args.C).fit(K, lab)

    def cv():
        m = KernelSVC('precomputed')
        m.scores = m.cross_val_score(K, lab2, Cs, cv=5)
        return m

    try:
        from sklearn.svm import SVC
        from sklearn.model_selection import StratifiedKFold, cross_val_score

        def sk_fit(lab):
            return lambda: SVC(C=args.C, kernel='precomputed',
                               cache_size=1000).fit(Kh, lab)

        def sk_cv():
            folds = StratifiedKFold(5, shuffle=True, random_state=0)
            return [cross_val_score(SVC(C=C, kernel='precomputed',
                                        cache_size=1000), Kh, lab2, cv=folds)
                    for C in Cs]
    except ImportError:
        sk_fit = lambda lab: None  # noqa: E731
        sk_cv = None
    measure('binary_fit', fit(lab2), lambda m: int(m.n_iter_.sum()),
            sk_fit(lab2))
    measure('ten_class_fit', fit(lab10), lambda m: int(m.n_iter_.sum()),
            sk_fit(lab10))
    measure('cross_val_8x5', cv, lambda m: m.last_timing['steps'], sk_cv)
    m = KernelSVC(kernel, C=args.C)
    ms, _ = timed(lambda: m.fit(G, lab2), 3, sync)
    out['fit_graphs'] = {'ms': ms, 'timing': m.last_timing}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
