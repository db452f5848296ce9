#!/usr/bin/env python
"""Times of the centred kernel-target alignment and its gradient on N QM7-like
graphs (tests/cases.py config 3, labels "energy above the median") after the
Gram matrix and the gradient planes are in place: the fused chain
(alignment.hip: three launches, one download of 2 + 2 m doubles) against the
torch chain (`_align.alignment_torch`) on the same device matrix and planes --
for the plain kernel on the float backend (float matrix and planes, all the
kernel's columns, the active ones read) and for the normalised kernel (double,
as `Normalization.device_gram` leaves them) -- and one whole `fit` of
`KernelTargetAlignment` with the optimizer, kernel evaluations included.  Host
clocks around work that ends in the download; medians of warm repeats.

    python scripts/time_alignment.py [--n 1000] [--repeats 7] [--out x.json]
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
    ap.add_argument('--tol', type=float, default=1e-5)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from graphdot_amd.model.alignment import KernelTargetAlignment, _align
    from graphdot_amd.model._device_kernel import active_planes
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    if not torch.cuda.is_available():
        raise SystemExit('time_alignment.py measures on a GPU; none found')
    sync = torch.cuda.synchronize
    n = args.n
    G = np.asarray(list(cases.config3_graphs(n)), dtype=object)
    e = cases.synthetic_energies(list(G))
    y = (e > np.median(e)).astype(int)
    T = np.eye(2)[y]
    Tc = torch.from_numpy(np.ascontiguousarray(T - T.mean(0))).cuda()
    Lnorm = float(np.linalg.norm((T - T.mean(0)).T @ (T - T.mean(0))))
    knode, kedge, q = cases.config3_fit_kernels()
    plain = MarginalizedGraphKernel(knode, kedge, q=q, q_bounds=(1e-3, 0.5),
                                    backend=HIPBackend(real=np.float32))
    out = {'n': n}
    for name, kernel in (('plain_f32', plain),
                         ('normalized', Normalization(plain))):
        t_gram, (Kd, dKd) = timed(
            lambda: kernel.device_gram(G, eval_gradient=True), 3, sync)
        # the matrix and the planes in place, as the model adopts them
        # (copies in the same layout: the kernel's own views die at its next
        # evaluation)
        K = torch.as_tensor(Kd, device='cuda')
        P = torch.as_tensor(dKd, device='cuda')
        K = torch.empty_strided(K.shape, K.stride(), dtype=K.dtype,
                                device='cuda').copy_(K)
        P = torch.empty_strided(P.shape, P.stride(), dtype=P.dtype,
                                device='cuda').copy_(P)
        planes = active_planes(kernel, P.shape[2])
        row = {'gram_and_gradient_ms': t_gram, 'matrix': str(K.dtype),
               'strides': list(K.stride()), 'plane_strides': list(P.stride()),
               'columns': int(P.shape[2]), 'planes': int(len(planes))}
        for chain, fn in (('fused', _align.alignment),
                          ('torch', _align.alignment_torch)):
            row[f'{chain}_value_ms'], v = timed(
                lambda: fn(K, Tc).cpu(), args.repeats, sync)
            row[f'{chain}_value_gradient_ms'], s = timed(
                lambda: fn(K, Tc, P, planes).cpu(), args.repeats, sync)
            m = len(planes)
            A, grad = _align.value_and_gradient(
                s[0], s[1], s[2:2 + m], s[2 + m:], Lnorm)
            row[f'{chain}_alignment'] = A
            row[f'{chain}_gradient_norm'] = float(np.linalg.norm(grad))
        out[name] = row
        print(name, json.dumps(row), flush=True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            kta = KernelTargetAlignment(kernel, optimizer=True)
            t = time.perf_counter()
            kta.fit(G, y, tol=args.tol)
            ms = 1e3 * (time.perf_counter() - t)
        res = kta.optimization_result
        fit = {'ms': ms, 'evaluations': int(res.nfev),
               'iterations': int(res.nit), 'converged': bool(res.success),
               'alignment_start': float(kta.alignment(kernel.theta)),
               'alignment': float(kta.alignment_),
               'last_timing': kta.last_timing}
        out[f'{name}_fit'] = fit
        print(f'{name}_fit', json.dumps(fit), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
