#!/usr/bin/env python
"""Step times of one ALE + gradient evaluation of the Gaussian field
regressor's fused device path on QM7-like graphs (tests/cases.py config 3):
N graphs, a labelled fraction, f32/f64 solver, raw and normalised kernel.
kernel = the device evaluations (one, to a synchronise; the first config
also pays the JIT load); rowsums, factor (cholesky_ex), solves (two
cholesky_solve), contract (gf_contract of both blocks) = median of --repeat
after a warm-up; the contraction also between device events, with its bytes
(K and the selected planes, read once) over that time.

    python scripts/time_gaussian_field.py [--out profiles/x.json]
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


def one(N, frac, real, normalized, repeat):
    import torch
    import cases
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.metric import KernelInducedDistance
    from graphdot_amd.model.gaussian_field import (GaussianFieldRegressor,
                                                   RBFOverDistance)
    G = np.asarray(cases.config3_graphs(N))
    rng = np.random.default_rng(0)
    y = (rng.uniform(size=N) > 0.5).astype(float)
    lab = np.zeros(N, bool)
    lab[rng.choice(N, int(frac * N), replace=False)] = True
    y[~lab] = np.nan
    knode, kedge, q = cases.config3_kernels()
    k = MarginalizedGraphKernel(knode, kedge, q=q,
                                backend=HIPBackend(real=real))
    if normalized:
        k = Normalization(k)
    g = GaussianFieldRegressor(
        RBFOverDistance(KernelInducedDistance(k), 0.3 if normalized else 5.0),
        device='cuda')
    rec = dict(N=N, labelled=int(lab.sum()), real=np.dtype(real).name,
               normalized=normalized)

    torch.cuda.synchronize()
    t = time.perf_counter()
    ul = g._cross_block(k, G[~lab], G[lab], True)
    uu = g._self_block(k, G[~lab], True)
    torch.cuda.synchronize()
    rec['kernel_s'] = time.perf_counter() - t

    f_l = torch.as_tensor(y[lab], dtype=torch.float64, device='cuda')
    state = {}

    def rowsums():
        state['ul'] = g._rowsums(ul, y=f_l)
        state['uu'] = g._rowsums(uu, write=True)

    def factor():
        s_ul = state['ul'][0]
        s_uu, _, W = state['uu']
        L = -W
        L.diagonal().add_(s_uu + s_ul)
        state['C'] = torch.linalg.cholesky_ex(L)[0]

    def solves():
        f_u = torch.cholesky_solve(state['ul'][1][:, None], state['C'])[:, 0]
        z = f_u.clamp(1e-7, 1 - 1e-7)
        gr = -(z.log() - (1 - z).log()) / len(z)
        state['f_u'] = f_u
        state['v'] = torch.cholesky_solve(gr[:, None], state['C'])[:, 0]

    def contract():
        v, f_u = state['v'], state['f_u']
        a = -v * f_u
        state['grad'] = g._contract(uu, a, v, f_u) + g._contract(ul, a, v,
                                                                 f_l)

    for name, f in (('rowsums', rowsums), ('factor', factor),
                    ('solves', solves), ('contract', contract)):
        rec[name + '_s'] = _median(f, repeat)
    rec['contract_events_s'] = _median(contract, repeat, events=True)
    n = len(uu['planes'])
    nbytes = 0
    for b in (uu, ul):
        Nr, Nc = b['K'].shape
        nbytes += Nr * Nc * (b['K'].element_size()
                             + n * b['P'].element_size())
    rec['contract_bytes'] = nbytes
    rec['contract_TBps'] = nbytes / rec['contract_events_s'] / 1e12
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--N', type=int, nargs='+', default=[1000, 4000])
    ap.add_argument('--frac', type=float, nargs='+', default=[0.1, 0.5])
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    import graphdot_amd.model.gaussian_field   # noqa: F401 (torch first)
    res = dict(device=torch.cuda.get_device_name(0), hbm_Bps=HBM,
               hbm_note='6.3 TB/s: assumed achievable HBM rate, not measured',
               steps=[])
    for N in args.N:
        for frac in args.frac:
            for real in (np.float32, np.float64):
                for normalized in (False, True):
                    rec = {k: float('%.4g' % v) if isinstance(v, float) else v
                           for k, v in one(N, frac, real, normalized,
                                           args.repeat).items()}
                    print(json.dumps(rec), flush=True)
                    res['steps'].append(json.dumps(rec))
    if args.out:
        head = ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(v))
                           for k, v in res.items() if k != 'steps')
        with open(args.out, 'w') as f:      # (one line per step)
            f.write('{\n%s,\n "steps": [\n  %s\n ]\n}\n' % (
                head, ',\n  '.join(res['steps'])))


if __name__ == '__main__':
    main()
