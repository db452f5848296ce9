"""graphdot_amd.model.tree_search and DevicePosterior without a GPU: the
rewriter against facts that follow from its definition, the transformer
against trees the reference built (tests/golden/tree_search.json, written by
tests/golden/make_golden_tree_search.py), the device posterior's algebra
through its torch restatement."""
import io
import os
import sys

import numpy as np
import pytest

from _fixtures import load, GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden_tree_search as problems      # noqa: E402
sys.path.remove(GOLDEN)

from graphdot_amd.model.tree_search import (     # noqa: E402
    MCTSGraphTransformer, AbstractRewriter, LookAheadSequenceRewriter)
from graphdot_amd.model.gaussian_process import (  # noqa: E402
    GaussianProcessRegressor, DevicePosterior)


def trie(rw):
    """{context + symbol as a tuple: (count, freq)} of a fitted rewriter."""
    t, out = rw.tree, {}

    def visit(nid, path):
        for c in t.children(nid):
            out[path + (c.tag,)] = (c.data.count, c.data.freq)
            visit(c.identifier, path + (c.tag,))
    visit(t.root, ())
    return out


# -- the rewriter ------------------------------------------------------------------
@pytest.mark.parametrize('n, X, expected', [
    (0, ['A'], {('A',): (1, 1.0)}),
    (1, ['A'], {('A',): (1, 1.0)}),
    (0, ['A', 'B'], {('A',): (1, 0.5), ('B',): (1, 0.5)}),
    (1, ['A', 'B'], {('A',): (1, 0.5), ('B',): (1, 0.5)}),
    (0, ['AA', 'BB'], {('A',): (2, 0.5), ('B',): (2, 0.5)}),
    (0, ['ABCDE'], {(c,): (1, 0.2) for c in 'ABCDE'}),
    (0, ['AABBB'], {('A',): (2, 0.4), ('B',): (3, 0.6)}),
    (1, ['AABBB'], {('A',): (2, 0.4), ('B',): (3, 0.6),
                    ('A', 'A'): (1, 0.5), ('A', 'B'): (1, 0.5),
                    ('B', 'B'): (2, 1.0)}),
    (1, ['AA', 'BB'], {('A',): (2, 0.5), ('B',): (2, 0.5),
                       ('A', 'A'): (1, 1.0), ('B', 'B'): (1, 1.0)}),
    (1, ['ABCDE'], dict(
        [((c,), (1, 0.2)) for c in 'ABCDE']
        + [((a, b), (1, 1.0)) for a, b in zip('ABCD', 'BCDE')])),
])
def test_trie_counts_and_frequencies(n, X, expected):
    rw = LookAheadSequenceRewriter(n=n)
    rw.fit(X)
    got = trie(rw)
    assert set(got) == set(expected)
    for key, (count, freq) in expected.items():
        assert got[key][0] == count
        assert got[key][1] == pytest.approx(freq, rel=1e-15)


def test_trie_interface():
    rw = LookAheadSequenceRewriter(n=1)
    rw.fit(['AB', 'AC'])
    t = rw.tree
    root = t[t.root]
    assert root.tag == '$' and root.identifier == t.root
    assert t.parent(t.root) is None
    a, b, c = t.children(t.root)            # insertion order
    assert [x.tag for x in (a, b, c)] == ['A', 'B', 'C']
    assert [x.tag for x in t.children(a.identifier)] == ['B', 'C']
    assert t.parent(b.identifier) is root
    assert set(t.nodes) == {n.identifier for n in t.nodes.values()}
    assert len(t.nodes) == 6
    buf = io.StringIO()
    t.show(file=buf)
    assert buf.getvalue().count('\n') == 6


def test_tree_before_fit_raises():
    with pytest.raises(RuntimeError):
        LookAheadSequenceRewriter().tree


def test_match_context_falls_back_to_the_longest_match():
    rw = LookAheadSequenceRewriter(n=2)
    rw.fit(['ABC', 'BD'])
    t = rw.tree
    path = lambda node: (path(t.parent(node.identifier))      # noqa: E731
                         + (node.tag,)) if node.identifier != t.root else ()
    match = lambda s, k: path(rw._match_context(t, s, k, 2))  # noqa: E731
    assert match('ABC', 2) == ('A', 'B')       # the full 2-gram was seen
    assert match('XAB', 3) == ('A', 'B')
    assert match('CB', 2) == ('B',)            # 'CB' never seen: 1-gram 'B'
    assert match('ABC', 1) == ('A',)           # only one symbol in front
    assert match('ABC', 0) == ()               # nothing in front: the root
    assert match('BC', 2) == ()                # 'C' has no successor at all
    assert match('ZZ', 2) == ()                # unseen symbols


def test_forced_edits():
    rw = LookAheadSequenceRewriter(n=0, random_state=0)
    rw.fit(['XXX'])                            # the only proposal is 'X'
    s = 'abc'
    for k in range(len(s)):
        assert rw._insert(s, k) == s[:k] + 'X' + s[k:]
        assert rw._mutate(s, k) == s[:k] + 'X' + s[k + 1:]
        assert rw._delete(s, k) == s[:k] + s[k + 1:]
    # context-sensitive: after 'A' always 'B', after 'B' always 'A'
    rw = LookAheadSequenceRewriter(n=1, random_state=0)
    rw.fit(['ABABAB'])
    assert rw._insert('AA', 1) == 'ABA'
    assert rw._mutate('BBB', 1) == 'BAB'
    assert rw._insert(('A', 'A'), 1) == ('A', 'B', 'A')


def test_proposal_frequencies():
    rw = LookAheadSequenceRewriter(n=0, random_state=12345)
    rw.fit(['AB'])
    draws = [rw._propose('AB', 1) for _ in range(10000)]
    share = draws.count('A') / len(draws)
    print('share of A in 10000 draws:', share)
    assert set(draws) == {'A', 'B'}
    # five standard deviations of a fair coin at 10 000 draws
    assert abs(share - 0.5) <= 0.025


def test_offspring():
    rw = LookAheadSequenceRewriter(n=1, b=5, random_state=3)
    rw.fit(['AABBB', 'ABAB', 'BBA'])
    for s in ('AB', 'ABBA', 'BBBB'):
        T = rw(s)
        assert len(T) <= 5 and s not in T and len(set(T)) == len(T)
    a = LookAheadSequenceRewriter(n=1, b=5, random_state=7).fit(['AABBB'])
    b = LookAheadSequenceRewriter(n=1, b=5, random_state=7).fit(['AABBB'])
    assert a('ABAB') == b('ABAB')
    # a passed generator takes the place of the internal one
    g = lambda: np.random.Generator(np.random.PCG64(5))       # noqa: E731
    assert a('ABAB', g()) == b('ABAB', g())
    assert issubclass(LookAheadSequenceRewriter, AbstractRewriter)


def test_rewriter_takes_a_node_view():
    from graphdot_amd.model.tree_search._tree import Tree
    tree = Tree(parent=[None], children=[None], g=['ABAB'],
                visits=np.zeros(1, dtype=int))
    node = next(tree.iternodes())
    a = LookAheadSequenceRewriter(n=1, random_state=7).fit(['AABBB'])
    b = LookAheadSequenceRewriter(n=1, random_state=7).fit(['AABBB'])
    assert a(node) == b('ABAB')


def test_tree_does_not_share_a_default():
    from graphdot_amd.model.tree_search._tree import Tree
    Tree(g=[1, 2])
    assert Tree().columns == []
    t = Tree(parent=[None, None], children=[None, None], g=[1, 2],
             visits=np.zeros(2, dtype=int))
    n = list(t.iternodes())[1]
    n.visits += 3
    assert t.visits[1] == 3 and n.g == 2
    with pytest.raises(AttributeError):
        n.no_such_column
    assert t.flat.columns == ['level', 'g', 'visits']
    assert 'visits' in str(t)


# -- the transformer against the reference ---------------------------------------------
GOLD = load('tree_search.json')


def test_golden_file_is_sound():
    kinds = [c['kind'] for c in GOLD['cases']]
    assert kinds.count('scalar') >= 4 and kinds.count('graph') >= 2
    assert GOLD['observed_disagreement'] * 1e3 < GOLD['MIN_GAP']
    for c in GOLD['cases']:
        assert c['min_gap'] >= GOLD['MIN_GAP']
        assert min(r['tree_std'] for r in c['rows']) > 0


@pytest.fixture(scope='module')
def pool_kernel():
    from oracle import mgk
    mgk.build()
    return problems.PoolKernel(problems.graph_pool())


@pytest.mark.parametrize('k', range(len(GOLD['cases'])))
def test_transformer_builds_the_reference_tree(k, pool_kernel):
    case = GOLD['cases'][k]
    if case['kind'] == 'scalar':
        X, y = problems.scalar_problem()
        kernel = problems.RBF(0.5)
        rewriter = problems.NormalSteps(case['b'], case['width'])
    else:
        pool = problems.graph_pool()
        X = np.arange(problems.N_TRAIN)
        y = problems.graph_targets(pool)[:problems.N_TRAIN]
        kernel = pool_kernel
        rewriter = problems.PoolDraws(case['b'])
    gpr = GaussianProcessRegressor(kernel, alpha=GOLD['alpha'], device='cpu')
    gpr.fit(X, y)
    t = MCTSGraphTransformer(rewriter, gpr, exploration_bias=case['bias'],
                             precision=case['precision'], device='cpu')
    tree = t.seek(case['g0'], case['target'], maxiter=case['maxiter'],
                  return_tree=True, random_state=case['seed'])
    rows = list(problems.walk(t, tree, case['target']))
    assert len(rows) == len(case['rows'])
    for got, ref in zip(rows, case['rows']):
        assert (got['level'], got['g'], got['visits']) == \
            (ref['level'], ref['g'], ref['visits'])
    for col in problems.FLOAT_COLUMNS:
        np.testing.assert_allclose([r[col] for r in rows],
                                   [r[col] for r in case['rows']],
                                   rtol=1e-9, atol=0, err_msg=col)
    # the flat table: sorted by likelihood, best first, one row per node
    df = t.seek(case['g0'], case['target'], maxiter=case['maxiter'],
                random_state=case['seed'])
    assert len(df) == len(rows)
    assert list(df.columns) == ['level', 'g', 'visits', 'self_mean',
                                'tree_mean', 'self_std', 'tree_std', 'score',
                                'likelihood']
    assert (np.diff(df['likelihood'].to_numpy()) <= 0).all()


def test_any_other_surrogate_is_asked_for_the_covariance():
    asked = []

    class Surrogate:
        def predict(self, g, return_cov=False):
            asked.append(return_cov)
            x = np.asarray(g, dtype=float)
            return np.sin(x), np.diag(0.04 + 0.01 * np.cos(x)**2)

    t = MCTSGraphTransformer(problems.NormalSteps(3, 0.5), Surrogate(),
                             precision=0.3)
    df = t.seek(0.2, 0.8, maxiter=4, random_state=0)
    assert asked and all(a is True for a in asked)
    assert len(df) == 1 + 4 * 3


def test_device_argument():
    X, y = problems.scalar_problem()
    gpr = GaussianProcessRegressor(problems.RBF(0.5), alpha=1e-4,
                                   device='cpu').fit(X, y)
    rw = problems.NormalSteps(3, 0.5)
    with pytest.raises(ValueError):
        MCTSGraphTransformer(rw, gpr, device='gpu')
    with pytest.raises(RuntimeError):
        MCTSGraphTransformer(rw, gpr, device='cuda').seek(0.2, 0.8, maxiter=1)
    a = MCTSGraphTransformer(rw, gpr, device='auto', precision=0.3).seek(
        0.2, 0.8, maxiter=5, random_state=1)
    b = MCTSGraphTransformer(rw, gpr, device='cpu', precision=0.3).seek(
        0.2, 0.8, maxiter=5, random_state=1)
    assert a.equals(b)
    # 'auto' builds no device posterior for a training set this small
    t = MCTSGraphTransformer(rw, gpr, device='auto', precision=0.3)
    t.seek(0.2, 0.8, maxiter=1, random_state=1)
    assert t._posterior is None and t._predict[0] is gpr


def test_auto_dispatches_by_the_measured_sizes():
    from graphdot_amd.model.tree_search import graph_transformer as gt

    class Side:
        def __init__(self, name, n=0):
            self.name, self.Kinv = name, np.zeros((n, 1))

        def predict(self, Z, **kw):
            return self.name

    def which(n, b):
        post = Side('device')
        post.gpr = Side('host', n)
        return gt._BySize(post).predict([0] * b, return_std=True)
    assert which(1000, 1) == which(4000, 10) == 'device'
    assert which(250, 5) == which(500, 10) == 'device'
    assert which(250, 1) == which(500, 1) == which(999, 4) == 'host'


# -- DevicePosterior on the CPU ------------------------------------------------------------
def _fitted(normalize_y, regularization, masked):
    rng = np.random.default_rng(3)
    X = rng.uniform(-3, 3, 40)
    y = list(np.sin(X) + X / 3 + 2.0)
    if masked:
        y[5] = None
        y[20] = float('nan')
    gpr = GaussianProcessRegressor(
        problems.RBF(0.7), alpha=1e-3, normalize_y=normalize_y,
        regularization=regularization, device='cpu')
    return gpr.fit(X, y), rng.uniform(-3, 3, 7)


@pytest.mark.parametrize('normalize_y', [False, True])
@pytest.mark.parametrize('regularization', ['+', '*'])
@pytest.mark.parametrize('masked', [False, True])
def test_device_posterior_algebra_equals_predict(normalize_y, regularization,
                                                 masked):
    import torch
    gpr, Z = _fitted(normalize_y, regularization, masked)
    post = DevicePosterior(gpr)
    assert not post.available               # (no CUDA algebra here)
    assert len(post.X) == (38 if masked else 40)
    kernel = gpr.kernel
    for dtype in (torch.float64, torch.float32):
        Ks = torch.from_numpy(kernel(Z, post.X)).to(dtype)
        mean = post._predict_from(Ks)
        m2, std = post._predict_from(Ks, kss=torch.from_numpy(kernel.diag(Z)))
        m3, cov = post._predict_from(Ks, Kss=torch.from_numpy(kernel(Z)))
        if dtype == torch.float64:
            rm, rs = gpr.predict(Z, return_std=True)
            _, rc = gpr.predict(Z, return_cov=True)
        else:
            # (the float path predicts from the rounded cross kernel: the
            # arithmetic of `GaussianProcessRegressor.predict` on it)
            R = Ks.to(torch.float64).numpy()
            rm = (R @ gpr.Ky) * gpr._ystd + gpr._ymean
            rc = np.maximum(0, gpr._gramian(gpr.alpha, Z)
                            - R @ (gpr.Kinv @ R.T)) * gpr._ystd**2
            rs = np.sqrt(np.maximum(
                0, gpr._gramian(gpr.alpha, Z, diag=True)
                - np.einsum('ij,jk,ik->i', R, gpr.Kinv, R))) * gpr._ystd
        for got in (mean, m2, m3):
            assert got.dtype == np.float64
            np.testing.assert_allclose(got, rm, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(std**2, rs**2, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(cov, rc, rtol=1e-9, atol=1e-12)
        assert std.dtype == cov.dtype == np.float64
        assert cov.shape == (7, 7)


def test_unavailable_posterior_is_predict():
    gpr, Z = _fitted(True, '+', True)
    post = DevicePosterior(gpr)
    for kw in ({}, dict(return_std=True), dict(return_cov=True)):
        a, b = post.predict(Z, **kw), gpr.predict(Z, **kw)
        for x, y in zip(a if kw else (a,), b if kw else (b,)):
            np.testing.assert_array_equal(x, y)
    with pytest.raises(RuntimeError):
        DevicePosterior(GaussianProcessRegressor(problems.RBF(1.0)))
    with pytest.raises(TypeError):
        DevicePosterior(object())


def test_a_refit_is_not_served_from_stale_copies():
    import torch
    gpr, Z = _fitted(False, '+', False)
    post = DevicePosterior(gpr)
    before = post.Kinv
    X = np.linspace(-2, 2, 9)
    gpr.fit(X, np.cos(X))
    np.testing.assert_array_equal(post.predict(Z, return_std=True)[1],
                                  gpr.predict(Z, return_std=True)[1])
    assert post.Kinv is not before and tuple(post.Kinv.shape) == (9, 9)
    assert len(post.X) == 9
    Ks = torch.from_numpy(gpr.kernel(Z, post.X))
    post._current()
    np.testing.assert_allclose(post._predict_from(Ks), gpr.predict(Z),
                               rtol=1e-12)


def test_posterior_source_compiles_for_gfx950():
    from graphdot_amd.model.gaussian_process import _posterior
    path = _posterior.precompile()
    assert os.path.getsize(path) > 0
    src = _posterior.source()
    for t in ('f32', 'f64'):
        for kc in _posterior._CHUNKS:
            assert f'ROWS({"float" if t == "f32" else "double"}, {t}, {kc})' \
                in src
    assert _posterior.grid(1000, 5) == (8, 250, 1)
    assert _posterior.grid(65, 40) == (16, 17, 3)
    assert _posterior.grid(1, 1) == (1, 1, 1)


def test_posterior_torch_matches_numpy():
    import torch
    from graphdot_amd.model.gaussian_process import _posterior
    rng = np.random.default_rng(0)
    n, b = 33, 5
    A = rng.normal(size=(n, n))
    Kinv = A @ A.T / n + np.eye(n)
    Ks = rng.normal(size=(b, n))
    Ky, kss = rng.normal(size=n), rng.uniform(50, 60, b)
    out, T = _posterior.posterior_torch(
        torch.from_numpy(Kinv), torch.from_numpy(Ks), torch.from_numpy(Ky),
        torch.from_numpy(kss), 1.5, 2.0, return_T=True)
    np.testing.assert_allclose(T.numpy(), Kinv @ Ks.T, rtol=1e-12)
    np.testing.assert_allclose(out[:b].numpy(), 2.0 * Ks @ Ky + 1.5,
                               rtol=1e-12)
    q = np.einsum('ij,jk,ik->i', Ks, Kinv, Ks)
    np.testing.assert_allclose(out[b:].numpy(),
                               2.0 * np.sqrt(np.maximum(0, kss - q)),
                               rtol=1e-12)
    cm = _posterior.column_major(torch.from_numpy(Ks))
    assert cm.stride() == (1, b) and torch.equal(cm, torch.from_numpy(Ks))
