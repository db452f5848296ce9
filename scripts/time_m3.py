#!/usr/bin/env python3
"""Timing of M3 (graphdot_amd.experimental.metric.m3) on one GPU: pairwise M3
over `cases.tang2019_graphs()` in double, fused epilogue against the host
composition, and Graph.from_ase over generated structures (host work).

    python scripts/time_m3.py [--graphs 256] [--structures 1000] [--repeat 3]

Prints one JSON object: milliseconds (best of --repeat, after one warm-up
call that includes compilation) and pairs / structures per second.
"""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'tests'))
import numpy as np                                                  # noqa: E402


class Atoms:
    def __init__(self, numbers, positions):
        self.numbers, self.positions = numbers, positions
        self.cell, self.pbc = np.zeros((3, 3)), np.zeros(3, dtype=bool)

    def __len__(self):
        return len(self.numbers)

    def get_atomic_numbers(self):
        return self.numbers

    def get_positions(self):
        return self.positions


def structures(n, seed=0):
    """Random molecules of 8-24 atoms (C, H, N, O, S) on a jittered grid."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(8, 25))
        grid = np.stack(np.meshgrid(*[np.arange(3)] * 3), -1).reshape(-1, 3)
        pos = 1.3 * grid[rng.permutation(len(grid))[:k]] + \
            0.1 * rng.normal(size=(k, 3))
        z = rng.choice([1, 1, 1, 6, 6, 7, 8, 16], size=k)
        out.append(Atoms(z, pos))
    return out


def best(f, repeat):
    f()
    times = []
    for _ in range(repeat):
        t = time.perf_counter()
        f()
        times.append(time.perf_counter() - t)
    return 1e3 * min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=256)
    ap.add_argument('--structures', type=int, default=1000)
    ap.add_argument('--repeat', type=int, default=3)
    a = ap.parse_args()
    import cases
    from graphdot_amd.graph import Graph
    from graphdot_amd.experimental.metric import M3

    G = cases.tang2019_graphs(a.graphs)
    m = M3()
    GX, _, _ = m._graphs(G, None)
    pairs = a.graphs * (a.graphs + 1) // 2
    fused = best(lambda: m._fused(GX, None), a.repeat)
    comp = best(lambda: m._composition(GX, None), a.repeat)
    D1, D2 = m._fused(GX, None), m._composition(GX, None)
    S = structures(a.structures)
    imp = best(lambda: [Graph.from_ase(s) for s in S], a.repeat)
    print(json.dumps(dict(
        graphs=a.graphs, pairs=pairs,
        fused_ms=round(fused, 2), fused_pairs_per_s=round(pairs / fused * 1e3),
        composition_ms=round(comp, 2),
        composition_pairs_per_s=round(pairs / comp * 1e3),
        max_abs_diff=float(np.abs(D1 - D2).max()),
        structures=a.structures, from_ase_ms=round(imp, 2),
        from_ase_per_s=round(a.structures / imp * 1e3))))


if __name__ == '__main__':
    main()
