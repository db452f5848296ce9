#!/usr/bin/env python
"""Wall time of the Nystrom regressor (LowRankApproximateGPR) on the GPU.

1. One likelihood + gradient step, ``log_marginal_likelihood(
   eval_gradient=True)``, of `Normalization(MarginalizedGraphKernel)` on
   QM7-like graphs (tests/cases.py config 3) for N training graphs and m core
   graphs, with the solver in float32 and float64.  Split as the model
   records it (`last_timing`): 'kernel' = the device evaluations (Kxc, Kcc
   and the two diagonals, up to a device synchronise), 'linalg' = the float64
   algebra on the GPU, the two gradient contractions and the one download.
   One warm-up step per shape, then the median of --repeat steps.

2. The gradient contraction ``out[k] = sum_ic W[i, c] P[i, c, k]`` of
   lowrank.hip against the torch route (the planes converted to float64,
   then one matrix-vector product), on random column-major planes, timed
   with device events (median of --repeat after a warm-up).  Bytes: the
   planes once plus W once, over the kernel's time.

    python scripts/time_nystrom.py [--out profiles/x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(ROOT)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def step_times(Ns, ms, repeat):
    import cases
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.model.gaussian_process import LowRankApproximateGPR
    t = time.perf_counter()
    G = cases.config3_graphs(max(Ns) + max(ms), seed=31)
    print(f'{len(G)} graphs in {time.perf_counter() - t:.1f} s', flush=True)
    rng = np.random.default_rng(0)
    out = []
    for real in ('f32', 'f64'):
        backend = HIPBackend(real=np.float64) if real == 'f64' \
            else HIPBackend()
        kn, ke, _ = cases.config3_kernels()
        kernel = Normalization(MarginalizedGraphKernel(kn, ke, q=0.05,
                                                       backend=backend))
        for N in Ns:
            X = G[:N]
            y = np.array([len(g.nodes) for g in X], float) \
                + 0.1 * rng.normal(size=N)
            for m in ms:
                C = G[-m:]
                model = LowRankApproximateGPR(kernel, alpha=1e-6,
                                              device='cuda')
                model.C, model.X, model.y = C, X, y
                model.log_marginal_likelihood(eval_gradient=True)
                rows = []
                for _ in range(repeat):
                    t = time.perf_counter()
                    value, grad = model.log_marginal_likelihood(
                        eval_gradient=True)
                    total = time.perf_counter() - t
                    rows.append((total, model.last_timing['kernel'],
                                 model.last_timing['linalg']))
                total, kern, lin = np.median(np.array(rows), axis=0)
                rec = dict(solver=real, N=N, m=m, pairs=N * m + m * m,
                           step_ms=1e3 * total, kernel_ms=1e3 * kern,
                           algebra_ms=1e3 * lin, value=float(value),
                           grad_norm=float(np.linalg.norm(grad)),
                           steps=repeat)
                print(json.dumps(rec), flush=True)
                out.append(rec)
    return out


def contraction_times(shapes, repeat):
    import torch
    from graphdot_amd.model.gaussian_process import _lowrank
    out = []
    for N, M, nt in shapes:
        for dtype in (torch.float32, torch.float64):
            P = torch.empty((nt, M, N), dtype=dtype, device='cuda')
            P.normal_()
            P = P.permute(2, 1, 0)
            W = torch.randn((N, M), dtype=torch.float64, device='cuda')
            routes = dict(hip=lambda: _lowrank.contract(P, W),
                          torch=lambda: _lowrank.contract_torch(P, W))
            rec = dict(N=N, m=M, n_theta=nt, planes=str(dtype)[6:])
            res = {}
            for name, f in routes.items():
                res[name] = f()
                ms = []
                for _ in range(repeat):
                    a = torch.cuda.Event(enable_timing=True)
                    b = torch.cuda.Event(enable_timing=True)
                    a.record()
                    f()
                    b.record()
                    b.synchronize()
                    ms.append(a.elapsed_time(b))
                rec[f'{name}_ms'] = float(np.median(ms))
            nbytes = N * M * nt * P.element_size() + N * M * 8
            rec['bytes'] = nbytes
            rec['hip_TBps'] = nbytes / rec['hip_ms'] / 1e9
            rec['torch_TBps'] = nbytes / rec['torch_ms'] / 1e9
            rec['max_rel_diff'] = float(
                ((res['hip'] - res['torch']).abs()
                 / res['torch'].abs().clamp(min=1e-300)).max())
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del P, W, res
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--N', type=int, nargs='+', default=[2000, 20000])
    ap.add_argument('--m', type=int, nargs='+', default=[100, 500])
    ap.add_argument('--skip-steps', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_nystrom.py needs a GPU')
    res = dict(device=torch.cuda.get_device_name(0))
    res['contraction'] = contraction_times(
        [(20000, 500, 7), (100000, 1000, 8)], max(args.repeat, 5))
    if not args.skip_steps:
        res['likelihood_step'] = step_times(args.N, args.m, args.repeat)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
