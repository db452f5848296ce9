"""Records tests/golden/tsne_bands.json: trustworthiness and KL divergence of
scikit-learn's exact t-SNE on the distances of `test_tsne.points(130, 5)`
under the kernel of test_tsne.py at perplexity 10, from the five starts ``1e-4
RandomState(s).standard_normal((130, 2))``, s = 0..4.  Runs from equal starts
diverge between implementations, so tests/test_tsne.py compares no trajectory:
a `KernelTSNE.fit` from other starts must land within scikit-learn's own
spread over starts.  Recorded numbers only.

    python tests/golden/make_golden_tsne.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    sys.path.insert(0, p)

N, SEED, PERPLEXITY, NEIGHBORS = 130, 5, 10.0, 5


def main():
    import sklearn
    from sklearn.manifold import TSNE, trustworthiness
    import test_tsne as t
    K = t.kernel_matrix(t.points(N, SEED))
    D = np.sqrt(t.define_d2(K))
    trust, kl = [], []
    for s in range(5):
        init = 1e-4 * np.random.RandomState(s).standard_normal((N, 2))
        m = TSNE(n_components=2, perplexity=PERPLEXITY, method='exact',
                 metric='precomputed', init=init)
        Y = m.fit_transform(D)
        trust.append(float(trustworthiness(D, Y, n_neighbors=NEIGHBORS,
                                           metric='precomputed')))
        kl.append(float(m.kl_divergence_))
    out = {'n': N, 'seed': SEED, 'perplexity': PERPLEXITY,
           'n_neighbors': NEIGHBORS, 'inits': list(range(5)),
           'sklearn': sklearn.__version__,
           'trustworthiness': trust, 'kl_divergence': kl}
    with open(os.path.join(HERE, 'tsne_bands.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(out)


if __name__ == '__main__':
    main()
