#!/usr/bin/env python
"""Times of one objective + gradient evaluation and of one `predict_proba` of
10 candidates of `GaussianProcessClassifier` on N QM7-like training graphs
(tests/cases.py config 3, normalised kernel, labels "energy above the
median"): the device path (laplace.hip around potrf.hip, the planes read
where the solver left them) against the class's own host path (`device =
'cpu'`: the same chain through torch on the CPU, the kernel evaluated on the
GPU and brought to the host).  Each evaluation is split into the kernel and
the algebra behind it (`last_timing`); on the device path the launches of one
evaluation are also timed between device events, one kind at a time.  Every
process reports medians after a warm-up; the parent starts --processes of
them one after the other and reports the median of their medians.

    python scripts/time_gpc.py [--sizes 250,1000,4000] [--out x.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
CANDIDATES = 10


def launches(kernel, G, y):
    """ms between device events of each kind of launch (medians of 5 after a
    warm-up), on the kernel's own device matrices and the first Newton step
    from f = 0: the times depend on the shapes, not on the values.  Only the
    device-path protocol and the launch functions are used, as the
    classifier uses them."""
    import torch
    from graphdot_amd.model._device_kernel import (device_call, as_float64,
                                                   active_planes)
    from graphdot_amd.model.gaussian_process import _laplace, _potrf
    dev = torch.device('cuda')
    Kd, dKd = device_call(kernel, 'device_gram', G, eval_gradient=True)
    K = as_float64(Kd, dev).contiguous()
    P = torch.as_tensor(dKd, device=dev)
    planes = active_planes(kernel, P.shape[2])
    n = K.shape[0]
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64), device=dev)
    f0 = torch.zeros(n, dtype=torch.float64, device=dev)
    B, vec, _ = _laplace.build(K, f0, yt, f0)
    Binv = _potrf.factor_inverse_(B)[0]
    a = _laplace.solve(Binv, vec)
    f = _laplace.apply(K, a)
    s, g = vec[n:2 * n], vec[3 * n:4 * n]
    u = _laplace.third_order(K, Binv, vec)

    def potrf():
        _laplace.build(K, f, yt, a, B)
        return lambda: _potrf.factor_inverse_(B)
    kinds = {
        'lp_build': lambda: lambda: _laplace.build(K, f, yt, a, B),
        'potrf': potrf,
        'lp_solve': lambda: lambda: _laplace.solve(Binv, vec),
        'lp_apply': lambda: lambda: _laplace.apply(K, a),
        'third_order_torch': lambda: lambda: _laplace.third_order(
            K, Binv, vec),
        'lp_planes_reduce': lambda: lambda: _laplace.contract(
            P, planes, Binv, s, a, u, g),
    }
    out = {'planes': int(len(planes)), 'plane_dtype': str(P.dtype)}
    for name, prepare in kinds.items():
        ts = []
        for _ in range(6):
            run = prepare()
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        out[f'{name}_ms'] = float(np.median(ts[1:]))
    return out


def one(N, repeat, pool):
    import cases
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.model.gaussian_process import GaussianProcessClassifier
    G = np.asarray(cases.config3_graphs(N), dtype=object)
    e = cases.synthetic_energies(list(G))
    y = (e > np.median(e)).astype(int)
    knode, kedge, q = cases.config3_kernels()
    kernel = Normalization(MarginalizedGraphKernel(knode, kedge, q=q,
                                                   backend='hip'))
    row = {'N': N}
    cursor = 0
    for name, device in (('device', 'cuda'), ('host', 'cpu')):
        m = GaussianProcessClassifier(kernel)
        m.device = device
        m.fit(G, y)
        # (the host algebra at N = 4000 takes seconds per Newton step)
        reps = repeat if name == 'device' else min(repeat, 3)
        total, kern, alg = [], [], []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            m.log_marginal_likelihood(kernel.theta, eval_gradient=True)
            total.append(time.perf_counter() - t0)
            kern.append(m.last_timing['kernel'])
            alg.append(m.last_timing['linalg'])
        assert m.last_timing['fused'] is (name == 'device')
        row[f'{name}_objective_ms'] = 1e3 * float(np.median(total[1:]))
        row[f'{name}_objective_kernel_ms'] = 1e3 * float(np.median(kern[1:]))
        row[f'{name}_objective_algebra_ms'] = 1e3 * float(np.median(alg[1:]))
        row[f'{name}_newton_steps'] = m.last_timing['newton_steps']
        ts = []
        for k in range(reps + 1):
            Z = pool[cursor:cursor + CANDIDATES]     # (candidates not seen)
            cursor = (cursor + CANDIDATES) % (len(pool) - CANDIDATES)
            t0 = time.perf_counter()
            m.predict_proba(Z)
            ts.append(time.perf_counter() - t0)
        row[f'{name}_predict_proba_ms'] = 1e3 * float(np.median(ts[1:]))
        if name == 'device':
            row['launches'] = launches(kernel, G, y)
    return row


def child(a):
    import torch
    import graphdot_amd.model.gaussian_process  # noqa: F401 (torch first)
    if not torch.cuda.is_available():
        raise SystemExit('time_gpc.py measures on a GPU; none found')
    import cases
    pool = np.asarray(cases.config3_graphs(400, seed=99), dtype=object)
    for N in map(int, a.sizes.split(',')):
        print(json.dumps(one(N, a.repeat, pool)), flush=True)


def merge(rows):
    """Median over the processes of every number of a row."""
    out = {}
    for key, first in rows[0].items():
        if isinstance(first, dict):
            out[key] = merge([r[key] for r in rows])
        elif isinstance(first, (int, float)) and key != 'N':
            out[key] = float(np.median([r[key] for r in rows]))
        else:
            out[key] = first
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='250,1000,4000')
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--processes', type=int, default=3)
    ap.add_argument('--timeout', type=float, default=900.0,
                    help='seconds one process may take')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.processes):
        out = subprocess.run(
            [sys.executable, os.path.abspath(__file__), '--child', '--sizes',
             a.sizes, '--repeat', str(a.repeat)],
            stdout=subprocess.PIPE, text=True, check=True,
            timeout=a.timeout)
        runs.append([json.loads(line) for line in out.stdout.splitlines()
                     if line.startswith('{')])
        print(f'process {len(runs)} of {a.processes} done', flush=True)
    rows = [merge([run[k] for run in runs]) for k in range(len(runs[0]))]
    for row in rows:
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'processes': a.processes, 'rows': rows,
                       'per_process': runs}, f, indent=1)


if __name__ == '__main__':
    main()
