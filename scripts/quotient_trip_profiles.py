#!/usr/bin/env python3
"""Trip profiles of the twin-leaf quotient pairs of the QM7-like set (DESIGN.md
section 4a): for every pair the degree product of the first row of each
64-row batch (HIPBackend.oc_trips), counted over all pairs -- what a static
layout of mgk_oc.h has to dominate -- and, for the menu in use, the pairs of
every static layout and the mean slots per lane (profiles: the lower bound of
any menu).  Host only.

    python scripts/quotient_trip_profiles.py [n_graphs]
"""
import os
import sys
from collections import Counter
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import cases                                                   # noqa: E402
from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend  # noqa: E402
from graphdot_amd.kernel.marginalized._devicegraph import (    # noqa: E402
    pack_many, quotient_graph)


def menu_table(backend, gs):
    """{layout: pairs} of the symmetric call on the images `gs` before small
    launches are merged, and the mean slots per lane."""
    i, j = np.triu_indices(len(gs))
    choice = backend.classify(i, j, gs, 1)[0]
    pairs = Counter(backend.variants[k] for k in choice.tolist())
    slots = sum(v.S * c for v, c in pairs.items()) / len(choice)
    return pairs, slots


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    dgs = pack_many(cases.config3_graphs(n), real=np.float64)
    backend = HIPBackend(real=np.float64)
    for name, gs in (('full', dgs), ('quotient', [quotient_graph(g) for g in dgs])):
        hist = np.array([np.bincount(g.adjacency_count, minlength=5)[:5]
                         for g in gs])
        H, hid = np.unique(hist, axis=0, return_inverse=True)
        hid = hid.reshape(-1)
        i, j = np.triu_indices(len(gs))
        pk = hid[i] * len(H) + hid[j]
        upk, count = np.unique(pk, return_counts=True)
        trips = HIPBackend.oc_trips(H[upk // len(H)], H[upk % len(H)], 4, 12)
        prof = Counter()
        for t, c in zip(trips, count):
            prof[tuple(int(x) for x in t if x)] += int(c)
        total = sum(prof.values())
        slots = sum(sum(k) * v for k, v in prof.items()) / total
        print(f'{name}: {len(prof)} profiles over {total} pairs, '
              f'{slots:.2f} slots per lane on average')
        for k, v in prof.most_common(12):
            print(f'  {v / total:6.1%}  {k}')
        pairs, slots = menu_table(backend, gs)
        print(f'  menu in use: {slots:.2f} slots per lane on average')
        for v, c in sorted(pairs.items(), key=lambda t: -t[1]):
            print(f'  {c:8d}  {v.L if getattr(v, "L", None) else tuple(v)}')


if __name__ == '__main__':
    main()
