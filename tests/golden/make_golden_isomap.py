"""Records tests/golden/isomap_bands.json: per shape of tests/test_isomap.py
(double storage), how far the numpy definition of KernelIsomap in that file is
from scikit-learn's ``Isomap(metric='precomputed', eigen_solver='dense')`` on
the CPU -- the largest differences of the embedding and of `transform` up to
the signs of the columns, whether the geodesics agree within the path bound,
scikit-learn's reconstruction error and the scale of the embedding.  The tests
allow the model 100 times the recorded differences.  Recorded numbers only.

    python tests/golden/make_golden_isomap.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    sys.path.insert(0, p)


def main():
    import sklearn
    import test_isomap as t
    cases = {}
    for n, k in t.SHAPES:
        c = t.case(n, k, np.float64)
        cases[f'{n}-{k}'] = dict(
            t.sklearn_differences(c), n_components=c.c, seed=t.SEEDS[n],
            eigenvalues=[float(w) for w in np.linalg.eigvalsh(
                t.centre(c.B))[::-1][:c.c + 1]])
    out = {'sklearn': sklearn.__version__, 'numpy': np.__version__,
           'cases': cases}
    with open(os.path.join(HERE, 'isomap_bands.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
