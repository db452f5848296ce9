#!/usr/bin/env python
"""Step times of one likelihood + gradient evaluation of the outlier
detector's fused device path on QM7-like graphs (tests/cases.py config 3):
N graphs, f32/f64 solver, raw and normalised kernel.  kernel = one device
evaluation with the gradient; potrf = factor_inverse; certificate_B =
cholesky_ of the shifted matrix; eigh = torch.linalg.eigh plus the
reconstruction of the clamped inverse (forced); epilogue = outlier.hip's
three launches between device events, with the bytes it reads over that
time; evaluation = the whole `log_marginal_likelihood` on the device and
with device='cpu' (the host baseline).  Medians of --repeat after a
warm-up.  Then one seeded `fit` with shifted targets: evaluations, the
share of each inverse path, total time and whether the shifted samples were
flagged.

    python scripts/time_outlier_detector.py [--out profiles/x.json]
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

HBM = 6.3e12


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


def _kernel(real, normalized):
    import cases
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    knode, kedge, q = cases.config3_fit_kernels()
    k = MarginalizedGraphKernel(knode, kedge, q=q, backend=HIPBackend(
        real=real), ftol=1e-13 if real is np.float64 else 1e-8)
    return Normalization(k) if normalized else k


def one(N, real, normalized, repeat):
    import torch
    import cases
    from graphdot_amd.model.gaussian_process import GPROutlierDetector
    from graphdot_amd.model.gaussian_process import _outlier
    from graphdot_amd.model.gaussian_process._potrf import (factor_inverse,
                                                            cholesky_)
    from graphdot_amd.model.gaussian_process.outlier_detector import _Inverse
    G = np.asarray(cases.config3_graphs(N), dtype=object)
    y = cases.synthetic_energies(list(G))
    y = (y - y.mean()) / y.std()
    k = _kernel(real, normalized)
    m = GPROutlierDetector(k, device='cuda')
    la = m._dense()
    sigma2 = np.full(N, 0.05)
    Ks, P, planes = m._device_inputs(la, k, list(G), True)
    Ks.diagonal().add_(torch.as_tensor(sigma2, device='cuda'))
    Kinv = factor_inverse(Ks)[0]
    yt = torch.as_tensor(y, device='cuda')
    out = {'N': N, 'real': np.dtype(real).name, 'normalized': normalized,
           'planes': len(planes), 'plane_dtype': str(P.dtype)[6:]}
    out['kernel_s'] = _median(
        lambda: m._device_inputs(la, k, list(G), True), repeat)
    out['potrf_s'] = _median(lambda: factor_inverse(Ks), repeat, True)

    def cert_b():
        B = Ks.clone()
        B.diagonal().sub_(1e-8)
        cholesky_(B)
    out['certificate_B_s'] = _median(cert_b, repeat, True)
    out['eigh_s'] = _median(lambda: _Inverse.clamp(Ks, 1e-8), repeat, True)
    out['epilogue_events_s'] = t = _median(
        lambda: _outlier.epilogue(Kinv, Ks, yt, sigma2, P, planes), repeat,
        True)
    # Kinv and Ks once (stage A), the planes' upper tiles and Kinv again
    # (stage B), the small vectors neglected
    tri = N * (N + 1) / 2
    nbytes = 2 * 8 * N * N + tri * (len(planes) * P.element_size() + 8)
    out['epilogue_bytes'] = int(nbytes)
    out['epilogue_TBps'] = round(nbytes / t / 1e12, 4)
    theta_ext = np.concatenate((k.theta, 0.5 * np.log(sigma2)))
    out['evaluation_s'] = _median(
        lambda: m.log_marginal_likelihood(theta_ext, X=G, y=y,
                                          eval_gradient=True), repeat)
    out['path'] = m.last_timing['path']
    host = GPROutlierDetector(k, device='cpu')
    out['evaluation_cpu_s'] = _median(
        lambda: host.log_marginal_likelihood(theta_ext, X=G, y=y,
                                             eval_gradient=True),
        max(1, repeat // 5))
    return {key: (float('%.4g' % v) if isinstance(v, float) else v)
            for key, v in out.items()}


def fit(N, shifted):
    import cases
    from graphdot_amd.model.gaussian_process import GPROutlierDetector
    G = np.asarray(cases.config3_graphs(N, seed=29), dtype=object)
    y = cases.synthetic_energies(list(G))
    y[shifted] += 3.0 * y.std() * np.array([1, -1, 1, -1, 1])[:len(shifted)]
    m = GPROutlierDetector(_kernel(np.float64, True), normalize_y=True,
                           device='cuda')
    paths = []
    lml = m.log_marginal_likelihood

    def counted(*args, **kwargs):
        r = lml(*args, **kwargs)
        paths.append(m.last_timing['path'])
        return r
    m.log_marginal_likelihood = counted
    np.random.seed(0)
    t = time.perf_counter()
    m.fit(G, y, w=0.3, repeat=1)
    total = time.perf_counter() - t
    u = m.y_uncertainty
    top = sorted(int(i) for i in np.argsort(u)[-len(shifted):])
    return {'N': N, 'real': 'float64', 'normalized': True,
            'shifted': shifted, 'evaluations': len(paths),
            'path_share': {p: round(paths.count(p) / len(paths), 4)
                           for p in ('A', 'B', 'eigh')},
            'total_s': round(total, 2),
            'per_evaluation_s': round(total / max(len(paths), 1), 5),
            'top_uncertainty': top, 'flagged': top == sorted(shifted),
            'u_shifted_min': float(u[shifted].min()),
            'u_others_max': float(np.delete(u, shifted).max())}


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument('--out')
    p.add_argument('--repeat', type=int, default=10)
    p.add_argument('--sizes', default='1000,2000')
    p.add_argument('--fit-size', type=int, default=1000)
    a = p.parse_args()
    rows = []
    for N in map(int, a.sizes.split(',')):
        for real in (np.float32, np.float64):
            for normalized in (False, True):
                rows.append(one(N, real, normalized, a.repeat))
                print(json.dumps(rows[-1]), flush=True)
    f = fit(a.fit_size, [3, 170, 401, 655, 902])
    print(json.dumps(f), flush=True)
    res = {'device': torch.cuda.get_device_name(0), 'hbm_Bps': HBM,
           'hbm_note': '6.3 TB/s: assumed achievable HBM rate, not measured',
           'steps': rows, 'fit': f}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('{\n "device": %s,\n "hbm_Bps": %s,\n "hbm_note": %s,\n'
                     ' "steps": [\n%s\n ],\n "fit": %s\n}\n' % (
                         json.dumps(res['device']), HBM,
                         json.dumps(res['hbm_note']),
                         ',\n'.join('  ' + json.dumps(r) for r in rows),
                         json.dumps(f)))


if __name__ == '__main__':
    main()
