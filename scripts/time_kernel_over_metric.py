#!/usr/bin/env python
"""Step times of KernelOverMetric(MaxiMin) in a Gaussian process on
QM7-like graphs (tests/cases.py config 3): one
`log_marginal_likelihood(eval_gradient=True)` on the device path and with
device='cpu' (the host path: the distance and its gradient downloaded, the
formula evaluated by numpy, K and the planes uploaded for nothing -- the
algebra runs on the CPU there); the device step split into the Maximin solve
(`MaxiMin.device_distance`), the map (kernel_over_metric.hip, between device
events, with the bytes it must move and the rate that gives) and the
algebra (the rest).  Medians of --repeat after a warm-up.

    python scripts/time_kernel_over_metric.py [--out profiles/x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

EXPR = 'v * exp(-d^2 / ell^2)'


def _median(f, repeat, events=False):
    import torch
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        t = time.perf_counter()
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 if events
                  else time.perf_counter() - t)
    return float(np.median(ts))


def one(N, repeat):
    import torch
    import cases
    from graphdot_amd.kernel import KernelOverMetric
    from graphdot_amd.metric.maximin import MaxiMin
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    G = cases.config3_graphs(N)
    y = cases.synthetic_energies(G)
    y = (y - y.mean()) / y.std()
    knode, kedge, q = cases.config3_kernels()
    mm = MaxiMin(knode, kedge, q=q, backend='hip')
    k = KernelOverMetric(mm, EXPR, 'd', v=(1.0, (1e-2, 1e2)),
                         ell=(0.5, (1e-2, 1e2)))
    out = {'N': N, 'expr': EXPR, 'distance_columns': len(mm.theta)}
    dev = GaussianProcessRegressor(k, alpha=1e-2, device='cuda')
    dev.X, dev.y = G, y
    out['step_device_s'] = _median(
        lambda: dev.log_marginal_likelihood(eval_gradient=True), repeat)
    host = GaussianProcessRegressor(k, alpha=1e-2, device='cpu')
    host.X, host.y = G, y
    out['step_host_s'] = _median(
        lambda: host.log_marginal_likelihood(eval_gradient=True),
        max(1, repeat // 2))
    # the pieces of the device step
    out['maximin_s'] = _median(
        lambda: mm.device_distance(G, eval_gradient=True), repeat)
    D, dD = mm.device_distance(G, eval_gradient=True)
    D = torch.as_tensor(D, device='cuda')
    dD = torch.as_tensor(dD, device='cuda')
    planes = np.flatnonzero(mm.active_theta_mask)
    dmap = k._map()
    h = k._h()
    out['map_s'] = _median(lambda: dmap(D, h, dD, planes, form='dense'),
                           repeat, events=True)
    n_h = len(h)
    nbytes = N * N * (D.element_size() + len(planes) * dD.element_size()
                      + 8 * (1 + n_h + len(planes)))
    out['map_bytes'] = int(nbytes)
    out['map_TBps'] = nbytes / out['map_s'] / 1e12
    out['algebra_s'] = out['step_device_s'] - out['maximin_s'] - out['map_s']
    out['avoided_transfer_numbers'] = int((1 + len(k.theta)) * N * N)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1000])
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import graphdot_amd.model.gaussian_process  # noqa: F401 (torch first)
    rec = {'device': torch.cuda.get_device_name(0), 'steps': []}
    for N in a.sizes:
        r = one(N, a.repeat)
        print(json.dumps(r), flush=True)
        rec['steps'].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
