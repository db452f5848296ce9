#!/usr/bin/env python
"""Times of one prediction of b candidates and of one tree-search iteration
against N QM7-like training graphs (tests/cases.py config 3): the device path
(`DevicePosterior`: cross kernel left on the device, posterior.hip, one
download of 2 b numbers) against the host path of the same commit
(`GaussianProcessRegressor.predict`).  Every call gets candidates it has not
seen.  The device prediction is split into the solver (`device_cross_gram` +
`device_diag`, of which the assembly and upload of the graph arena of all
N + b graphs is timed separately), the fused kernel (between device events,
with the bytes of the inverse it must stream and the rate that gives) and the
rest (adoption, regularisation, download); the host prediction into the
kernel evaluation and the numpy algebra.  The parts are timed inside one and
the same call as their total, so they add up to it; the whole predictions and
the iterations alternate between the two paths.  Medians (and quartiles) of
--repeat after a warm-up; host clocks around work that ends in a
synchronisation.  Run it several times to see the spread between processes.

    python scripts/time_tree_search.py [--sizes 250,1000,4000] [--out x.json]
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


class PoolDraws:
    def __init__(self, pool, b):
        self.pool, self.b = pool, b

    def __call__(self, node, rng):
        return [self.pool[i] for i in rng.choice(len(self.pool), size=self.b,
                                                 replace=False)]


def one(N, bs, repeat, pool):
    import torch
    import cases
    from graphdot_amd.hip import runtime
    from graphdot_amd.kernel.fix import Normalization
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.model.gaussian_process import (
        GaussianProcessRegressor, DevicePosterior, _posterior)
    from graphdot_amd.model.tree_search import MCTSGraphTransformer
    G = np.asarray(cases.config3_graphs(N), dtype=object)
    y = cases.synthetic_energies(list(G))
    knode, kedge, q = cases.config3_kernels()
    mgk = MarginalizedGraphKernel(knode, kedge, q=q, backend='hip')
    gpr = GaussianProcessRegressor(Normalization(mgk), alpha=1e-2,
                                   normalize_y=True, device='cuda')
    t = time.perf_counter()
    gpr.fit(G, y)
    rows = [{'N': N, 'fit_s': time.perf_counter() - t}]
    post = DevicePosterior(gpr)
    assert post.available
    backend = mgk.backend
    arena_s, arena_bytes = [], []
    inner_arena, upload = backend._arena, runtime.DeviceBuffer.upload

    def timed_arena(*a, **k):
        t0 = time.perf_counter()
        out = inner_arena(*a, **k)
        arena_s.append(time.perf_counter() - t0)
        return out

    def counting(self, array, *a, **k):
        arena_bytes.append(np.asarray(array).nbytes)
        return upload(self, array, *a, **k)
    backend._arena = timed_arena
    runtime.DeviceBuffer.upload = counting
    cursor = [0]

    def fresh(b):
        k = cursor[0]
        cursor[0] = (k + b) % (len(pool) - b)
        return list(pool[k:k + b])

    def stats(ts):
        q1, med, q3 = np.percentile(ts, [25, 50, 75])
        return 1e3 * float(med), [1e3 * float(q1), 1e3 * float(q3)]

    kernel = gpr.kernel
    for b in bs:
        row = {'N': N, 'b': b}
        # whole predictions, the two paths alternating
        whole = {'device': [], 'host': []}
        paths = (('device', post.predict), ('host', gpr.predict))
        for _, f in paths:
            f(fresh(b), return_std=True)
        torch.cuda.synchronize()
        for _ in range(repeat):
            for name, f in paths:
                Z = fresh(b)
                t0 = time.perf_counter()
                f(Z, return_std=True)
                whole[name].append(time.perf_counter() - t0)
        for name in whole:
            row[f'{name}_predict_ms'], row[f'{name}_predict_iqr_ms'] = \
                stats(whole[name])
        # the device path in parts, timed inside one and the same call: the
        # steps of DevicePosterior.predict with a synchronisation after the
        # solver, so total = solver + fused + rest
        total, solver, arena, sent, fused = [], [], [], [], []
        for _ in range(repeat):
            Z = fresh(b)
            del arena_s[:], arena_bytes[:]
            t0 = time.perf_counter()
            Ks = torch.as_tensor(kernel.device_cross_gram(Z, post.X),
                                 device='cuda')
            kss = torch.as_tensor(kernel.device_diag(Z), device='cuda')
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            kss = gpr._regularize(kss.to(torch.float64), gpr.alpha)
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            out, _ = _posterior.posterior(post.Kinv, Ks, post.Ky, kss,
                                          gpr._ymean, gpr._ystd)
            e1.record()
            out.cpu()
            t2 = time.perf_counter()
            total.append(t2 - t0)
            solver.append(t1 - t0)
            arena.append(sum(arena_s))
            sent.append(sum(arena_bytes))
            fused.append(e0.elapsed_time(e1) * 1e-3)
        total, solver, fused = map(np.asarray, (total, solver, fused))
        row['device_parts_total_ms'] = stats(total)[0]
        row['device_solver_ms'] = stats(solver)[0]
        row['device_arena_ms'] = stats(arena)[0]
        row['device_arena_share'] = float(np.median(np.asarray(arena) / total))
        row['device_uploaded_bytes'] = float(np.median(sent))
        row['device_fused_ms'] = stats(fused)[0]
        row['device_rest_ms'] = stats(total - solver - fused)[0]
        row['kinv_bytes'] = 8 * N * N
        row['fused_GBps'] = 8 * N * N / (row['device_fused_ms'] * 1e-3) / 1e9
        # the host path in parts, likewise inside one call: the statements of
        # GaussianProcessRegressor.predict(return_std=True)
        total, kern = [], []
        for _ in range(repeat):
            Z = fresh(b)
            t0 = time.perf_counter()
            Ks = np.asarray(gpr._gramian(None, Z, gpr._X),
                            dtype=np.float64)[:, gpr._y_mask]
            Kss = gpr._gramian(gpr.alpha, Z, diag=True)
            t1 = time.perf_counter()
            mean = (Ks @ gpr.Ky) * gpr._ystd + gpr._ymean
            var = Kss - np.einsum('ij,jk,ik->i', Ks, gpr.Kinv, Ks)
            std = np.sqrt(np.maximum(0, var)) * gpr._ystd
            t2 = time.perf_counter()
            total.append(t2 - t0)
            kern.append(t1 - t0)
        total, kern = np.asarray(total), np.asarray(kern)
        row['host_parts_total_ms'] = stats(total)[0]
        row['host_kernel_ms'] = stats(kern)[0]
        row['host_algebra_ms'] = stats(total - kern)[0]
        # tree-search iterations, the two paths alternating
        its = {'cuda': [], 'cpu': []}
        ts = {d: MCTSGraphTransformer(PoolDraws(pool, b), gpr, device=d,
                                      precision=0.5) for d in its}
        for d in its:
            ts[d].seek(pool[0], float(np.median(y)), maxiter=2,
                       random_state=0)
        for k in range(5):
            for d in its:
                t0 = time.perf_counter()
                ts[d].seek(pool[0], float(np.median(y)), maxiter=6,
                           random_state=k)
                its[d].append((time.perf_counter() - t0) / 7)
        for d in its:
            row[f'{d}_iteration_ms'], row[f'{d}_iteration_iqr_ms'] = \
                stats(its[d])
        print(json.dumps(row), flush=True)
        rows.append(row)
    backend._arena = inner_arena
    runtime.DeviceBuffer.upload = upload
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='250,1000,4000')
    ap.add_argument('--candidates', default='1,5,10')
    ap.add_argument('--repeat', type=int, default=15)
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    import graphdot_amd.model.gaussian_process  # noqa: F401 (torch first)
    if not torch.cuda.is_available():
        raise SystemExit('time_tree_search.py measures on a GPU; none found')
    import cases
    pool = np.asarray(cases.config3_graphs(400, seed=99), dtype=object)
    rows = []
    for N in map(int, a.sizes.split(',')):
        rows += one(N, list(map(int, a.candidates.split(','))), a.repeat, pool)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
